"""Child process of tests/test_hip_fused_orders.py: one seeded multi-step decode run at the bench head geometry under whatever
EKV_FUSED_ORDER the parent put into the environment (the library reads it once per process), everything it produced saved with
torch.save.

    python -m tests.fused_orders_run POLICY DTYPE OUT.pt"""
import sys

import torch

L, H, D, BUDGET, STEPS, SEED = 18, 32, 128, 2048, 72, 4242      # 576 heads per launch: 4-wave workgroups, two or more per CU
PHASE_SLOT_ROWS = 16


def inputs(dtype):
    """The run's tensors, on the CPU (the parent builds the same ones for the oracle)."""
    g = torch.Generator().manual_seed(SEED)
    k0, v0 = torch.randn(L, H, BUDGET, D, generator=g).to(dtype), torch.randn(L, H, BUDGET, D, generator=g).to(dtype)
    warm = torch.rand(L, H, BUDGET + 1, generator=g) * 1e-3
    qs = torch.randn(STEPS, L, H, 1, D, generator=g).to(dtype)
    ks = torch.randn(STEPS, L, H, 1, D, generator=g).to(dtype)
    vs = torch.randn(STEPS, L, H, 1, D, generator=g).to(dtype)
    return k0, v0, warm, qs, ks, vs


def main(policy, dtype_name, out_path):
    from easykv_amd import KVBank, StepPlan
    dtype = {"fp16": torch.float16, "bf16": torch.bfloat16}[dtype_name]
    T = BUDGET + 1
    k0, v0, warm, qs, ks, vs = inputs(dtype)
    bank = KVBank(L, H, H, D, cap=T + 63, dtype=dtype)
    # scattered slot map: logical position j lives in physical row perm[j]; the free rows in between hold NaN / inf bit patterns
    gp = torch.Generator().manual_seed(SEED + 1)
    perm = torch.stack([torch.randperm(bank.cap, generator=gp) for _ in range(L * H)]).view(L, H, bank.cap).int().cuda()
    bank.slot_of_pos.copy_(perm)
    bank.k.fill_(float("nan"))
    bank.v.fill_(float("inf"))
    bank.v[:, :, ::3] = float("nan")
    bank.k[:, :, 1::4] = float("-inf")
    bank.load_rows(k0.cuda(), v0.cuda())          # goes through the slot map
    bank.extent = [bank.cap] * L                   # the free list is not in library order: extent unknown
    bank.state_init(T, 0)
    bank.score_sum[:, :, :T] += warm.cuda()
    bank.score_sq[:, :, :T] += (warm ** 2).cuda()
    plan = StepPlan(policy=policy, phase="decode", evict=True, score_off=0, budget=BUDGET, n_split=1)
    info = bank.step_info(plan, 1, phases=PHASE_SLOT_ROWS)
    outs, ids, n_slot = [], [], 0
    for i in range(STEPS):
        o, e = bank.attend(plan, qs[i].cuda(), ks[i].cuda(), vs[i].cuda())
        n_slot += int(all(bank._slot_rows))
        outs.append(o.cpu())
        ids.append(e.cpu())
    torch.cuda.synchronize()
    bits = lambda t: t.detach().cpu().contiguous().view(torch.int32)      # (bit patterns: NaN-proof equality)
    res = dict(info=info, n_slot=n_slot, n_slots=list(bank.n_slots), outs=torch.stack(outs).view(torch.int16), ids=torch.stack(ids),
               # the raw slot-indexed state, read without converting the layers back
               S=bits(bank._score_sum), Q=bits(bank._score_sq), C0=bits(bank._score_cnt), birth=bank.birth.cpu(),
               slot_of_pos=bank._slot_of_pos.cpu(), slot_state=bits(bank.slot_state),
               k_sum=int(bank.k.view(torch.int16).long().sum()), v_sum=int(bank.v.view(torch.int16).long().sum()))
    torch.save(res, out_path)


if __name__ == "__main__":
    main(*sys.argv[1:4])
