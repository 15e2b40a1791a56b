"""Child process of tests/test_hip_resident_rows.py: seeded multi-step decode runs at the bench head geometry (32 heads, head_dim 128)
under whatever EKV_RESIDENT_ROWS and EKV_FUSED_ORDER the parent put into the environment (the library reads both once per process),
everything they produced saved with torch.save.

    python -m tests.resident_rows_run LAYERS BUDGET STEPS OUT.pt POLICY:DTYPE [POLICY:DTYPE ...]"""
import sys

import torch

H, D, SEED = 32, 128, 777
PHASE_SLOT_ROWS = 16


def run(L, budget, steps, policy, dtype_name):
    from easykv_amd import KVBank, StepPlan
    dtype = {"fp16": torch.float16, "bf16": torch.bfloat16}[dtype_name]
    T = budget + 1
    g = torch.Generator(device="cuda").manual_seed(SEED)
    rnd = lambda *shape: torch.randn(*shape, generator=g, device="cuda").to(dtype)
    k0, v0 = rnd(L, H, budget, D), rnd(L, H, budget, D)
    warm = torch.rand(L, H, T, generator=g, device="cuda") * 1e-3
    qs, ks, vs = rnd(steps, L, H, 1, D), rnd(steps, L, H, 1, D), rnd(steps, L, H, 1, D)
    bank = KVBank(L, H, H, D, cap=T + 63, dtype=dtype)
    # scattered slot map: logical position j lives in physical row perm[j]; the free rows in between hold NaN / inf bit patterns
    perm = torch.argsort(torch.rand(L, H, bank.cap, generator=g, device="cuda"), dim=-1).int()
    bank.slot_of_pos.copy_(perm)
    bank.k.fill_(float("nan"))
    bank.v.fill_(float("inf"))
    bank.v[:, :, ::3] = float("nan")
    bank.k[:, :, 1::4] = float("-inf")
    bank.load_rows(k0, v0)                         # goes through the slot map
    bank.extent = [bank.cap] * L                   # the free list is not in library order: extent unknown
    bank.state_init(T, 0)
    bank.score_sum[:, :, :T] += warm
    bank.score_sq[:, :, :T] += warm ** 2
    plan = StepPlan(policy=policy, phase="decode", evict=True, score_off=0, budget=budget, n_split=1)
    info = bank.step_info(plan, 1, phases=PHASE_SLOT_ROWS)
    rows = bank.resident_rows(plan, phases=PHASE_SLOT_ROWS)
    outs, ids, n_slot = [], [], 0
    for i in range(steps):
        o, e = bank.attend(plan, qs[i], ks[i], vs[i])
        n_slot += int(all(bank._slot_rows))
        outs.append(o.clone())
        ids.append(e.clone())
    torch.cuda.synchronize()
    bits = lambda t: t.detach().cpu().contiguous().view(torch.int32)      # (bit patterns: NaN-proof equality)
    return dict(info=info, rows=rows, cap=bank.cap, n_slot=n_slot, n_slots=list(bank.n_slots), outs=torch.stack(outs).cpu().view(torch.int16),
                ids=torch.stack(ids).cpu(),
                # the raw slot-indexed state, read without converting the layers back
                S=bits(bank._score_sum), Q=bits(bank._score_sq), C0=bits(bank._score_cnt), birth=bank.birth.cpu(),
                slot_of_pos=bank._slot_of_pos.cpu(), slot_state=bits(bank.slot_state),
                k_sum=int(bank.k.view(torch.int16).long().sum()), v_sum=int(bank.v.view(torch.int16).long().sum()))


def main(L, budget, steps, out_path, *cases):
    res = {}
    for case in cases:
        policy, dtype = case.split(":")
        res[case] = run(int(L), int(budget), int(steps), policy, dtype)
    torch.save(res, out_path)


if __name__ == "__main__":
    main(*sys.argv[1:])
