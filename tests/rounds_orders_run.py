"""Child process of tests/test_hip_rounds_orders.py and tests/test_hip_rounds_launch.py: seeded multi-step decode runs on the 8-wave
one-launch instance under whatever EKV_FUSED_NW / EKV_FUSED_ORDER / EKV_FUSED_ORDER_RULE the parent put into the environment (the
library reads them once per process), everything they produced saved with torch.save as {config name: result}.

    python -m tests.rounds_orders_run orders POLICY DTYPE OUT.pt      8 KV heads x 2 layers, every extent x resident-row setting
    python -m tests.rounds_orders_run launch POLICY DTYPE OUT.pt      17 layers x 32 heads at budget 64: a launch with a second round"""
import sys

import torch

D, SEED, STEPS = 128, 5150, 24
PHASE_SLOT_ROWS = 16
# physical extents around the 8-wave geometry (a workgroup iteration is 8 waves x 32 rows = 256 rows): the 5-column build holds 2304
# rows (5 x 512 thread-owned columns >= 2304), the 12-column build 6144
EXTENTS = (1, 255, 256, 257, 513, 2049, 2304, 2305, 2560)
RESIDENT = ("none", "one_unit", "all")      # resident rows 0, 32, >= the extent


def geometry(extent):
    """(live slots T of every step, cap) of an extent: up to 13 free rows inside [0, extent) — seeded with NaN / inf — and the rest of
    the free list behind it.  Extent 1 is the empty bank: T grows 1, 2, .. without evictions (a step of T = 1 has nothing to evict)."""
    t = 1 if extent == 1 else extent - min(13, extent - 2)
    up = lambda x: (x + 255) // 256 * 256
    if 2 * up(extent) > 3 * up(t):      # (the slot-indexed layout keeps two rows over [0, extent) where the ordered one keeps three over
        t = extent                      #  [0, T): at extent 257 only a full bank has the room, and the free rows all lie behind the extent)
    cap = max(16, (extent + 63 + 3) // 4 * 4)
    return t, cap


def inputs(L, H, n_rows, dtype, steps=STEPS, seed=SEED):
    g = torch.Generator().manual_seed(seed + n_rows)
    k0, v0 = torch.randn(L, H, max(n_rows, 1), D, generator=g).to(dtype), torch.randn(L, H, max(n_rows, 1), D, generator=g).to(dtype)
    warm = torch.rand(L, H, n_rows + 1, generator=g) * 1e-3
    qs, ks, vs = (torch.randn(steps, L, H, 1, D, generator=g).to(dtype) for _ in range(3))
    return k0[:, :, :n_rows], v0[:, :, :n_rows], warm, qs, ks, vs


def resident_bytes(which, heads, cap, policy):
    score_rows = 3 if policy == "roco" else 1
    score = heads * 4 * cap * (score_rows + 2)
    return {"none": 0, "one_unit": score + heads * 2 * 32 * 2 * D, "all": 1 << 40}[which]


def one_run(L, H, extent, policy, dtype, resident, steps=STEPS, t_cap=None):
    from easykv_amd import KVBank, StepPlan
    T, cap = t_cap or geometry(extent)
    n_rows = T - 1
    evict = n_rows > 0
    k0, v0, warm, qs, ks, vs = inputs(L, H, n_rows, dtype, steps)
    bank = KVBank(L, H, H, D, cap=cap, dtype=dtype)
    cap = bank.cap      # (the bank rounds its capacity up)
    bank.resident_bytes = resident_bytes(resident, L * H, cap, policy)
    # scattered slot map: the live rows and the first free rows are a permutation of [0, extent), the rest of the free list lies behind
    # it in address order (where a growing bank takes its rows from); every row that is not loaded holds NaN / inf bit patterns
    gp = torch.Generator().manual_seed(SEED + extent)
    perm = torch.stack([torch.cat([torch.randperm(extent, generator=gp), torch.arange(extent, cap)])
                        for _ in range(L * H)]).view(L, H, cap).int().cuda()
    bank.slot_of_pos.copy_(perm)
    bank.k.fill_(float("nan"))
    bank.v.fill_(float("inf"))
    bank.v[:, :, ::3] = float("nan")
    bank.k[:, :, 1::4] = float("-inf")
    if n_rows:
        bank.load_rows(k0.cuda(), v0.cuda())          # goes through the slot map
    bank.extent = [extent] * L
    bank.state_init(T, 0)
    if n_rows:
        bank.score_sum[:, :, :T] += warm.cuda()
        bank.score_sq[:, :, :T] += (warm ** 2).cuda()
    plan = StepPlan(policy=policy, phase="decode", evict=evict, score_off=0, budget=max(n_rows, steps + 1), n_split=1)
    info = bank.step_info(plan, 1, phases=PHASE_SLOT_ROWS)
    rows = bank.resident_rows(plan, phases=PHASE_SLOT_ROWS)
    outs, ids, n_slot = [], [], 0
    for i in range(steps):
        o, e = bank.attend(plan, qs[i].cuda(), ks[i].cuda(), vs[i].cuda())
        n_slot += int(all(bank._slot_rows))
        outs.append(o.cpu())
        if e is not None:
            ids.append(e.cpu())
    torch.cuda.synchronize()
    bits = lambda t: t.detach().cpu().contiguous().view(torch.int32)      # (bit patterns: NaN-proof equality)
    return dict(info=info, resident_rows=rows, n_slot=n_slot, n_slots=list(bank.n_slots), outs=torch.stack(outs).view(torch.int16),
                ids=torch.stack(ids) if ids else torch.zeros(0),
                S=bits(bank._score_sum), Q=bits(bank._score_sq), C0=bits(bank._score_cnt), birth=bank.birth.cpu(),
                slot_of_pos=bank._slot_of_pos.cpu(), slot_state=bits(bank.slot_state),
                k_sum=int(bank.k.view(torch.int16).long().sum()), v_sum=int(bank.v.view(torch.int16).long().sum()))


def main(what, policy, dtype_name, out_path):
    dtype = {"fp16": torch.float16, "bf16": torch.bfloat16}[dtype_name]
    res = {}
    if what == "orders":
        for extent in EXTENTS:
            for resident in RESIDENT:
                res[f"e{extent}_{resident}"] = one_run(2, 8, extent, policy, dtype, resident)
    else:      # 544 workgroups: 512 of them resident at once on 256 CUs, 32 dispatched as the first ones end
        res["launch"] = one_run(17, 32, 65 + 15, policy, dtype, "all", steps=3, t_cap=(65, 65 + 15))
    torch.save(res, out_path)


if __name__ == "__main__":
    main(*sys.argv[1:5])
