"""fp16 K/V rows against FP8 rows with per-row scales (KVBank.quantize_fp8), in one process, timings interleaved (fp16 rep, fp8 rep,
fp16 rep, ...); writes profiles/kv8_bench.json and prints it as one JSON line.

  * the fused decode step at the north-star shape (L 32, H 32, D 128, budget 2048, roco; scattered slot map, warm score state,
    pre-warm steps) on the fp16 bank and on its quantised twin (same rows, same slot map, same score rows);
  * the same at head_dim 64;
  * the one-layer-per-call deferred form of a 32-layer stack (attend(defer=True) per layer + one flush()), per layer.

Per leg: µs per launch (median of per-rep means, HIP events on the launch stream), the fp16 leg's run-to-run spread, the algorithmic
bytes per launch computed from the shapes (K/V rows read once — 2 * D * 2 bytes per row pair, or 2 * D + 8 with FP8 codes and two
scales — + the appended row, q / out, and the score rows once in and once out), GB/s and the fraction of the 8 TB/s HBM peak.

--mxfp4 adds a third leg on MXFP4 rows (KVBank.quantize_mxfp4: head_dim + head_dim / 16 bytes per row pair) to the head_dim-128 runs,
interleaved with the other two in the same process on a third copy of the same rows, slot map and score state (fp16 rep, fp8 rep,
mxfp4 rep, ...), and writes profiles/kv4_bench.json instead: per leg the median, the run-to-run spread and the algorithmic bytes.

--mxfp6 adds the MXFP4 leg and a fourth leg on MXFP6 rows (KVBank.quantize_mxfp6: 3 * head_dim / 2 + head_dim / 16 bytes per row pair)
in the same way — fp16, fp8, mxfp4 and mxfp6 interleaved on copies of the same rows — and writes profiles/kv6_bench.json.

--fp8-mxfp4 adds the MXFP4 and MXFP6 legs and a fifth leg on FP8 keys with MXFP4 values (KVBank.quantize_fp8_mxfp4: 3 * head_dim / 2 + 4 +
head_dim / 32 bytes per row pair, MXFP6's 200 at head_dim 128) — fp16, fp8, mxfp4, mxfp6 and fp8_mxfp4 interleaved on copies of the same
rows — and writes profiles/kv84_bench.json.

--k16-mxfp4 runs four legs — fp16, fp8, fp8_mxfp4 and 16-bit keys with MXFP4 values (KVBank.quantize_k16_mxfp4: 2 * head_dim + head_dim / 2
+ head_dim / 32 bytes per row pair, 324 at head_dim 128) — interleaved on copies of the same rows, and writes profiles/kv164_bench.json.

Usage: python tools/bench_kv8.py [--reps 15] [--steps 20] [--warm 1000] [--mxfp4 | --mxfp6 | --fp8-mxfp4 | --k16-mxfp4] [--out profiles/kv8_bench.json]"""
from __future__ import annotations

import argparse
import gc
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.bench_common import HBM_PEAK_GBS, algorithmic_bytes  # noqa: E402


def step_bytes(kind, L, H, Hq, D, T, n_state=3):
    """Algorithmic bytes of one whole decode step over L layers (tools/bench_common.algorithmic_bytes for 16-bit rows)."""
    b = algorithmic_bytes(H, Hq, D, T, 1, n_state)
    if kind == "fp8":
        kv = H * T * (2 * D + 8)                  # codes of K and V + the two row scales, read once
        new = H * (2 * D + 8)                     # the appended row, as stored
        b = dict(total=kv + new + 2 * Hq * D * 2 + 2 * n_state * H * T * 4, kv=kv)
    elif kind == "mxfp4":
        kv = H * T * (D + D // 16)                # codes of K and V (half a byte per element) + one exponent byte per 32 elements
        new = H * (D + D // 16)
        b = dict(total=kv + new + 2 * Hq * D * 2 + 2 * n_state * H * T * 4, kv=kv)
    elif kind == "mxfp6":
        kv = H * T * (3 * D // 2 + D // 16)       # codes of K and V (six bits per element) + one exponent byte per 32 elements
        new = H * (3 * D // 2 + D // 16)
        b = dict(total=kv + new + 2 * Hq * D * 2 + 2 * n_state * H * T * 4, kv=kv)
    elif kind == "fp8_mxfp4":
        pair = 3 * D // 2 + 4 + D // 32           # K: one byte per element + the row scale; V: half a byte per element + one exponent byte per 32
        kv = H * T * pair
        b = dict(total=kv + H * pair + 2 * Hq * D * 2 + 2 * n_state * H * T * 4, kv=kv)
    elif kind == "k16_mxfp4":
        pair = 2 * D + D // 2 + D // 32           # K: the 16-bit row; V: half a byte per element + one exponent byte per 32
        kv = H * T * pair
        b = dict(total=kv + H * pair + 2 * Hq * D * 2 + 2 * n_state * H * T * 4, kv=kv)
    else:
        b = dict(total=b["total"], kv=2 * H * T * D * 2)
    return {k: v * L for k, v in b.items()}


def _time(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(steps):
        fn(i)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / steps


def _interleave(fns, reps, steps, warm):
    for f in fns.values():
        for i in range(warm):
            f(i)
    torch.cuda.synchronize()
    got = {k: [] for k in fns}
    for _ in range(reps):
        for k, f in fns.items():
            got[k].append(_time(f, steps))
    return {k: dict(us=round(statistics.median(v), 2), spread=round((max(v) - min(v)) / statistics.median(v), 4)) for k, v in got.items()}


def make_bank(kind, L, H, D, budget):
    from easykv_amd import KVBank
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(1234)
    T = budget + 1
    bank = KVBank(L, H, H, D, cap=T + 63, device=dev)
    for l0 in range(0, L, 8):
        bank.load_rows(torch.randn(8, H, budget, D, generator=g, device=dev).half(), torch.randn(8, H, budget, D, generator=g, device=dev).half(),
                       pos_begin=0, layer_begin=l0)
    bank.slot_of_pos[:, :, :budget] = torch.argsort(torch.rand(L, H, budget, generator=g, device=dev), dim=-1).int()      # scattered slot map
    bank.state_init(T, 0)
    warm = torch.rand(L, H, budget, generator=g, device=dev) * 1e-3                                                       # warm score state
    bank.score_sum[:, :, :budget] += warm
    bank.score_sq[:, :, :budget] += warm ** 2
    if kind == "fp8":
        bank.quantize_fp8()
    elif kind in ("mxfp4", "mxfp6", "fp8_mxfp4", "k16_mxfp4"):
        bank.quantize(kind)
    return bank, g


def fused_step(kind, L=32, H=32, D=128, budget=2048):
    from easykv_amd import StepPlan
    bank, g = make_bank(kind, L, H, D, budget)
    dev, n = bank.device, 64
    qs, ks, vs = (torch.randn(n, L, H, 1, D, generator=g, device=dev).half() for _ in range(3))
    out = torch.empty(L, H, 1, D, dtype=torch.float16, device=dev)
    ids = torch.empty(L, H, 1, dtype=torch.int32, device=dev)
    plan = StepPlan(policy="roco", phase="decode", evict=True, score_off=0, budget=budget)
    assert bank.step_plan(plan, 1, 0, L) == (1, True), (kind, bank.step_plan(plan, 1, 0, L))
    return lambda i: bank.attend(plan, qs[i % n], ks[i % n], vs[i % n], out=out, evict_ids=ids)


def deferred_step(kind, L=32, H=32, D=128, budget=2048):
    """One token of a decoder stack: one attend(defer=True) per layer (attention + fold), then one flush() (the scorer of all layers)."""
    from easykv_amd import StepPlan
    bank, g = make_bank(kind, L, H, D, budget)
    dev, n = bank.device, 16
    qs, ks, vs = (torch.randn(n, L, 1, H, 1, D, generator=g, device=dev).half() for _ in range(3))
    out = torch.empty(1, H, 1, D, dtype=torch.float16, device=dev)
    plan = StepPlan(policy="roco", phase="decode", evict=True, score_off=0, budget=budget)

    def forward(i):
        q, k, v = qs[i % n], ks[i % n], vs[i % n]
        for l in range(L):
            bank.attend(plan, q[l], k[l], v[l], layer_begin=l, defer=True, out=out)
        bank.flush()
    return forward


def leg(name, maker, shape, reps, steps, warm, per=1, kinds=("fp16", "fp8")):
    fns = {kind: maker(kind, **shape) for kind in kinds}
    t = _interleave(fns, reps, steps, warm)
    del fns
    gc.collect()
    torch.cuda.empty_cache()
    L, H, D, T = shape["L"], shape["H"], shape["D"], shape["budget"] + 1
    res = {}
    for kind in kinds:
        b = step_bytes(kind, L, H, H, D, T)
        us = t[kind]["us"] / per
        gbs = b["total"] / per / (us * 1e-6) / 1e9
        res[kind] = dict(us_per_launch=round(us, 2), run_to_run_spread=t[kind]["spread"], bytes_per_launch=b["total"] // per,
                         kv_bytes_per_launch=b["kv"] // per, gb_per_s=round(gbs, 1), frac_of_hbm_peak=round(gbs / HBM_PEAK_GBS, 4))
    res["time_ratio_fp8_over_fp16"] = round(res["fp8"]["us_per_launch"] / res["fp16"]["us_per_launch"], 4)
    res["byte_ratio_fp8_over_fp16"] = round(res["fp8"]["bytes_per_launch"] / res["fp16"]["bytes_per_launch"], 4)
    res["faster_by_more_than_the_fp16_spread"] = bool(1.0 - res["time_ratio_fp8_over_fp16"] > res["fp16"]["run_to_run_spread"])
    for mx in ("mxfp4", "mxfp6", "fp8_mxfp4", "k16_mxfp4"):
        if mx in kinds:
            for other in kinds[:kinds.index(mx)]:
                res[f"time_ratio_{mx}_over_{other}"] = round(res[mx]["us_per_launch"] / res[other]["us_per_launch"], 4)
                res[f"byte_ratio_{mx}_over_{other}"] = round(res[mx]["bytes_per_launch"] / res[other]["bytes_per_launch"], 4)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=1000)
    ap.add_argument("--mxfp4", action="store_true", help="add the MXFP4 leg to the head_dim-128 runs; the default --out becomes profiles/kv4_bench.json")
    ap.add_argument("--mxfp6", action="store_true", help="add the MXFP4 and MXFP6 legs to the head_dim-128 runs; the default --out becomes profiles/kv6_bench.json")
    ap.add_argument("--fp8-mxfp4", action="store_true", help="add the MXFP4, MXFP6 and FP8-key / MXFP4-value legs to the head_dim-128 runs; the default "
                    "--out becomes profiles/kv84_bench.json")
    ap.add_argument("--k16-mxfp4", action="store_true", help="the fp16, FP8, FP8-key / MXFP4-value and 16-bit-key / MXFP4-value legs of the head_dim-128 "
                    "runs; the default --out becomes profiles/kv164_bench.json")
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None, help="run one leg: fused_d128, fused_d64 or deferred_d128 (nothing is written)")
    args = ap.parse_args()
    name = "kv164_bench.json" if args.k16_mxfp4 else "kv84_bench.json" if args.fp8_mxfp4 else ("kv6_bench.json" if args.mxfp6 else ("kv4_bench.json" if args.mxfp4 else "kv8_bench.json"))
    out = args.out or os.path.join(ROOT, "profiles", name)
    kinds = ("fp16", "fp8", "mxfp4", "mxfp6") if args.mxfp6 else (("fp16", "fp8", "mxfp4") if args.mxfp4 else ("fp16", "fp8"))
    if args.fp8_mxfp4:
        kinds = ("fp16", "fp8", "mxfp4", "mxfp6", "fp8_mxfp4")
    if args.k16_mxfp4:
        kinds = ("fp16", "fp8", "fp8_mxfp4", "k16_mxfp4")
    torch.cuda.set_device(0)
    res = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "steps": args.steps, "warm": args.warm, "hbm_peak_gb_per_s": HBM_PEAK_GBS,
           "shape": "32 layers x 32 heads, budget 2048 (T = 2049), roco, scattered slot map, warm score state"}
    shape = dict(L=32, H=32, D=128, budget=2048)
    legs = {"fused_d128": lambda: leg("fused_d128", fused_step, shape, args.reps, args.steps, args.warm, kinds=kinds),
            "fused_d64": lambda: leg("fused_d64", fused_step, dict(shape, D=64), args.reps, args.steps, args.warm),
            # (per layer: one forward is 32 attention launches + the flush; bytes per layer likewise)
            "deferred_d128": lambda: leg("deferred_d128", deferred_step, shape, args.reps, max(4, args.steps // 4), max(20, args.warm // 32), per=32, kinds=kinds)}
    if args.mxfp4 or args.mxfp6 or args.fp8_mxfp4 or args.k16_mxfp4:
        del legs["fused_d64"]      # (MXFP4 / MXFP6 / FP8-key MXFP4-value rows are head_dim 128's)
    for name, run in legs.items():
        if args.only in (None, name):
            res[name] = run()
    if args.only is None:
        with open(out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
