"""Cycle stamps of the fused decode step (headline shape) reduced to what the two-round launch is about: per CU, how long 0, 1 and
>= 2 of its workgroups are streaming K/V while the launch runs, the gap between the CU's last streamed byte and its end, and how many
heads each CU served.  Same -DEKV_TAIL_PROFILE build and stamps as exp_orderprof.py; the knobs (EKV_FUSED_NW, EKV_FUSED_ROUNDS,
EKV_FUSED_ORDER, EKV_FUSED_ORDER_RULE) come from the environment.

    tools/experiments/build_variant.sh tailprof "-DEKV_TAIL_PROFILE" ekv_attn_decode_d128_plain
    EASYKV_HIP_LIB=easykv_amd/csrc/variants/lib_tailprof.so EKV_FUSED_ROUNDS=1 python tools/experiments/exp_roundsprof.py LABEL [out.txt]"""
import json, os, sys, torch, numpy as np
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exp_orderprof as P


def reduce_cu(st, launch_us):
    xcc, cu = st[:, 7] & 0xF, (st[:, 6] >> 8) & 0xFF
    key = xcc * 256 + cu
    cus = np.unique(key)
    us = launch_us / float(np.median([st[key == c][:, 5].max() - st[key == c][:, 0].min() for c in cus]))
    rows = []
    for c in cus:
        s = st[key == c]
        ev = []                                      # (+1 / -1 at the ends of every streaming interval)
        for r in s:
            ev += [(r[0], 1), (r[1], -1)]
            if r[3] == 1:
                ev += [(r[2], 1), (r[5], -1)]
        ev.sort()
        a, b = int(s[:, 0].min()), int(s[:, 5].max())
        t = [0, 0, 0]
        cur, n = a, 0
        for x, d in ev:
            t[min(n, 2)] += x - cur
            cur, n = x, n + d
        t[0] += b - cur
        last = max(max(r[1], r[5] if r[3] == 1 else 0) for r in s)
        rows.append((t[0] * us, t[1] * us, t[2] * us, (b - last) * us, len(s), int((s[:, 3] == 1).sum())))
    return np.array(rows), us


def main(label, out=None):
    dev = torch.device("cuda")
    from easykv_amd import KVBank, StepPlan
    L = H = 32
    D, budget = 128, 2048
    T = budget + 1
    g = torch.Generator(device=dev).manual_seed(5)
    bank = KVBank(L, H, H, D, cap=T + 63, device=dev)
    bank.load_rows(torch.randn(L, H, budget, D, generator=g, device=dev).half(), torch.randn(L, H, budget, D, generator=g, device=dev).half())
    bank.slot_of_pos[:, :, :budget] = torch.argsort(torch.rand(L, H, budget, generator=g, device=dev), dim=-1).int()
    bank.state_init(T, 0)
    qs, ks, vs = (torch.randn(32, L, H, 1, D, generator=g, device=dev).half() for _ in range(3))
    o = torch.empty(L, H, 1, D, dtype=torch.float16, device=dev)
    ids = torch.empty(L, H, 1, dtype=torch.int32, device=dev)
    plan = StepPlan(policy="roco", phase="decode", evict=True, score_off=0, budget=budget)
    n = 0

    def step():
        nonlocal n
        bank.attend(plan, qs[n % 32], ks[n % 32], vs[n % 32], out=o, evict_ids=ids)
        n += 1
        if n % 64 == 0:
            torch.cuda.synchronize()
    for _ in range(4200):
        step()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(256):
        step()
    ev[1].record()
    torch.cuda.synchronize()
    launch_us = ev[0].elapsed_time(ev[1]) / 256 * 1e3
    lines = []
    for s in range(5):
        for _ in range(8):
            step()
        bank._ws.zero_()
        step()
        torch.cuda.synchronize()
        rows, us = reduce_cu(P.stamps_of(bank, L * H), launch_us)
        q = lambda i: "/".join(f"{x:.1f}" for x in np.percentile(rows[:, i], [10, 50, 90]))
        lines.append(f"{label} sample {s}: launch {launch_us:.1f} us, {len(rows)} CUs; per CU p10/p50/p90 us with 0 / 1 / >= 2 streaming workgroups: "
                     f"{q(0)} | {q(1)} | {q(2)}; end gap {q(3)}; heads per CU min/median/max {int(rows[:, 4].min())}/{int(np.median(rows[:, 4]))}/{int(rows[:, 4].max())}; "
                     f"order-K workgroups {int(rows[:, 5].sum())} of {int(rows[:, 4].sum())}")
        print(lines[-1], flush=True)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)) or ".", exist_ok=True)
        with open(out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(*sys.argv[1:3])
