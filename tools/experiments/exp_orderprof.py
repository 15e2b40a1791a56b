"""Cycle stamps of the fused decode step (headline shape) from a -DEKV_TAIL_PROFILE build of the ekv_attn_decode_d128_plain instance:
per CU, how long no resident workgroup is streaming K/V while the launch is still running (the exposed scorer tails).

    tools/experiments/build_variant.sh tailprof "-DEKV_TAIL_PROFILE" ekv_attn_decode_d128_plain
    EASYKV_HIP_LIB=easykv_amd/csrc/variants/lib_tailprof.so python tools/experiments/exp_orderprof.py [out.json]

Stamps per head (8 x u64 in the unused tova_row scratch): 0 start, 1 end of the first stream phase, 2 end of a mid-life tail (order K
only, else 0), 3 phase order (0 = F: K+V stream then tail, 1 = K: K stream, tail, V stream), 5 end, 6 HW_REG_HW_ID, 7 HW_REG_XCC_ID.
A workgroup streams during [0, 1] and, in order K, [2, 5].  Cycles are turned into microseconds with the event-timed launch duration
over the median per-CU span (only stamps of one CU are ever compared: the counters of different CUs are not aligned)."""
import json, os, sys, torch, numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from easykv_amd import KVBank, StepPlan
dev = torch.device("cuda")


def stamps_of(bank, n_heads):
    w = bank._ws[: bank._ws.numel() // 8 * 8].view(torch.int64).cpu().numpy()
    n = len(w) - 8
    ok = (w[:n] > 10**8) & (w[1:n + 1] >= w[:n]) & (w[4:n + 4] == 0) & (w[5:n + 5] >= w[1:n + 1]) & (w[6:n + 6] > 0) & (w[6:n + 6] < 2**32)
    i0 = int(np.nonzero(ok)[0][0])
    return w[i0:i0 + n_heads * 8].reshape(n_heads, 8).copy()


def analyse(st, launch_us):
    xcc = st[:, 7] & 0xF
    cu = (st[:, 6] >> 8) & 0xFF                      # CU_ID | SH_ID | SE_ID
    key = xcc * 256 + cu
    span_c = [st[key == c][:, 5].max() - st[key == c][:, 0].min() for c in np.unique(key)]
    us = launch_us / float(np.median(span_c))        # microseconds per cycle
    rows = []
    for x in np.unique(xcc):
        sx = st[xcc == x]
        for c in np.unique(cu[xcc == x]):
            s = sx[cu[xcc == x] == c]
            iv = []                                  # streaming intervals of the CU's workgroups
            for r in s:
                iv.append((r[0], r[1]))
                if r[3] == 1:
                    iv.append((r[2], r[5]))
            iv.sort()
            a, b = int(s[:, 0].min()), int(s[:, 5].max())
            covered, cur = 0, a
            for lo, hi in iv:
                lo = max(lo, cur)
                if hi > lo:
                    covered += hi - lo
                    cur = hi
            last_stream = max(hi for _, hi in iv)
            rows.append(dict(xcc=int(x), cu=int(c), wgs=len(s), order_k=int((s[:, 3] == 1).sum()),
                             tg_ids=sorted(int(v) for v in (s[:, 6] >> 16) & 0xF), wave_ids=sorted(int(v) for v in s[:, 6] & 0xF),
                             span_us=(b - a) * us, no_stream_us=(b - a - covered) * us, end_gap_us=(b - last_stream) * us,
                             finish_spread_us=(s[:, 5].max() - s[:, 5].min()) * us,
                             tail_us=float(np.mean(np.where(s[:, 3] == 1, s[:, 2] - s[:, 1], s[:, 5] - s[:, 1]))) * us))
    # per hardware workgroup slot (HW_ID.TG_ID): when its workgroup ends its first stream phase and when it ends, from the CU's first start
    t0 = np.zeros(len(st), dtype=np.int64)
    for c in np.unique(key):
        t0[key == c] = st[key == c][:, 0].min()
    tg = (st[:, 6] >> 16) & 0xF
    by_tg = {int(t): dict(n=int((tg == t).sum()), order_k=int((st[tg == t][:, 3] == 1).sum()),
                          start_us=round(float(np.mean(st[tg == t][:, 0] - t0[tg == t])) * us, 1),
                          stream1_end_us=round(float(np.mean(st[tg == t][:, 1] - t0[tg == t])) * us, 1),
                          end_us=round(float(np.mean(st[tg == t][:, 5] - t0[tg == t])) * us, 1)) for t in np.unique(tg)}
    return rows, us, by_tg


def run(policy="roco", L=32, Hq=32, H=32, D=128, budget=2048, prewarm=4200, samples=5, dtype=torch.float16):
    T = budget + 1
    g = torch.Generator(device=dev).manual_seed(5)
    bank = KVBank(L, Hq, H, D, cap=T + 63, device=dev, dtype=dtype) if dtype != torch.float16 else KVBank(L, Hq, H, D, cap=T + 63, device=dev)
    bank.load_rows(torch.randn(L, H, budget, D, generator=g, device=dev).to(dtype), torch.randn(L, H, budget, D, generator=g, device=dev).to(dtype))
    bank.slot_of_pos[:, :, :budget] = torch.argsort(torch.rand(L, H, budget, generator=g, device=dev), dim=-1).int()
    bank.state_init(T, 0)
    n_in = 32
    qs = torch.randn(n_in, L, Hq, 1, D, generator=g, device=dev).to(dtype)
    ks = torch.randn(n_in, L, H, 1, D, generator=g, device=dev).to(dtype)
    vs = torch.randn(n_in, L, H, 1, D, generator=g, device=dev).to(dtype)
    o = torch.empty(L, Hq, 1, D, dtype=dtype, device=dev)
    ids = torch.empty(L, H, 1, dtype=torch.int32, device=dev)
    plan = StepPlan(policy=policy, phase="decode", evict=True, score_off=0, budget=budget)
    n = 0
    for _ in range(prewarm):
        bank.attend(plan, qs[n % n_in], ks[n % n_in], vs[n % n_in], out=o, evict_ids=ids); n += 1
        if n % 64 == 0:
            torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(256):
        bank.attend(plan, qs[n % n_in], ks[n % n_in], vs[n % n_in], out=o, evict_ids=ids); n += 1
    ev[1].record(); torch.cuda.synchronize()
    launch_us = ev[0].elapsed_time(ev[1]) / 256 * 1e3
    out = []
    for s in range(samples):
        for _ in range(8):
            bank.attend(plan, qs[n % n_in], ks[n % n_in], vs[n % n_in], out=o, evict_ids=ids); n += 1
        bank._ws.zero_()
        bank.attend(plan, qs[n % n_in], ks[n % n_in], vs[n % n_in], out=o, evict_ids=ids); n += 1
        torch.cuda.synchronize()
        rows, us, by_tg = analyse(stamps_of(bank, L * H), launch_us)
        col = lambda k: np.array([r[k] for r in rows])
        q = lambda k: [round(float(x), 1) for x in np.percentile(col(k), [10, 50, 90])]
        mix = {}
        for r in rows:
            key = f"{r['order_k']}K+{r['wgs'] - r['order_k']}F"
            mix[key] = mix.get(key, 0) + 1
        hist = lambda k: {str(v): int(n) for v, n in zip(*np.unique([str(r[k]) for r in rows], return_counts=True))}
        summ = dict(sample=s, tg_ids_per_cu=hist("tg_ids"), wave0_ids_per_cu=hist("wave_ids"), by_tg_id=by_tg, policy=policy, launch_us=round(launch_us, 1), cycles_per_us=round(1 / us, 1), cus=len(rows),
                    wgs_per_cu={int(k): int((col("wgs") == k).sum()) for k in np.unique(col("wgs"))}, orders_per_cu=mix,
                    p10_p50_p90=dict(span_us=q("span_us"), no_stream_us=q("no_stream_us"), end_gap_us=q("end_gap_us"),
                                     finish_spread_us=q("finish_spread_us"), tail_us=q("tail_us")),
                    cus_with_end_gap_ge_6us=int((col("end_gap_us") >= 6).sum()))
        print(json.dumps(summ), flush=True)
        out.append(dict(summary=summ, per_cu=rows if s == samples - 1 else None))
    return out


if __name__ == "__main__":
    res = run(os.environ.get("POLICY", "roco"))
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as f:
            json.dump(res, f)
