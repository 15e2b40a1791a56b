"""fp16 against bf16 K/V banks, in one process, timings interleaved (fp16 rep, bf16 rep, fp16 rep, ...); prints one JSON line.

  * the fused decode step at the bench shape (L 32, H 32, D 128, T 2049, roco; scattered slot map, warm state, prewarm steps);
  * the configs[1] (stride 8 onto 2056 slots, 32 heads) and configs[2] (GQA 32 -> 8, stride 16 onto 1232 slots) chunk steps, in the
    oscillating steady state of the strided prefill;
  * per-layer HF-shaped calls of a 32-layer stack (BudgetedKVCache.attend, one layer per call): bf16 q / k / v as [1, H, n, D] views of
    a [1, n, H * D] projection, decode (n = 1) and stride 8, into the default fp16 bank (converted on the way in and out) and into a
    bf16 bank (read in place).

Medians of per-rep means (HIP events on the launch stream).  Usage: python tools/bench_dtype.py [--reps 15] [--steps 20]"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

DTYPES = {"fp16": torch.float16, "bf16": torch.bfloat16}


def _time(fn, steps):
    """Mean µs of `fn(i)` over `steps` calls (events around the whole run)."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(steps):
        fn(i)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / steps


def _interleave(makers, reps, steps, warm):
    """makers: name -> (step function); runs `warm` untimed steps each, then `reps` interleaved timed runs; -> name -> median µs."""
    fns = {k: m() for k, m in makers.items()}
    for f in fns.values():
        for i in range(warm):
            f(i)
    torch.cuda.synchronize()
    got = {k: [] for k in fns}
    for _ in range(reps):
        for k, f in fns.items():
            got[k].append(_time(f, steps))
    return {k: round(statistics.median(v), 2) for k, v in got.items()}


def decode_maker(dt, L=32, H=32, D=128, budget=2048):
    def make():
        from easykv_amd import KVBank, StepPlan
        dev = torch.device("cuda")
        g = torch.Generator(device=dev).manual_seed(1234)
        T = budget + 1
        bank = KVBank(L, H, H, D, cap=T + 63, device=dev, dtype=dt)
        for l0 in range(0, L, 8):
            bank.load_rows(torch.randn(8, H, budget, D, generator=g, device=dev).to(dt), torch.randn(8, H, budget, D, generator=g, device=dev).to(dt),
                           pos_begin=0, layer_begin=l0)
        bank.slot_of_pos[:, :, :budget] = torch.argsort(torch.rand(L, H, budget, generator=g, device=dev), dim=-1).int()
        bank.state_init(T, 0)
        n = 64
        qs, ks, vs = (torch.randn(n, L, H, 1, D, generator=g, device=dev).to(dt) for _ in range(3))
        out = torch.empty(L, H, 1, D, dtype=dt, device=dev)
        ids = torch.empty(L, H, 1, dtype=torch.int32, device=dev)
        plan = StepPlan(policy="roco", phase="decode", evict=True, score_off=0, budget=budget)
        assert bank.step_plan(plan, 1, 0, L)[1]
        return lambda i: bank.attend(plan, qs[i % n], ks[i % n], vs[i % n], out=out, evict_ids=ids)
    return make


def chunk_maker(dt, L, Hq, H, stride, t_prev, D=128):
    def make():
        from easykv_amd import KVBank, StepPlan
        dev = torch.device("cuda")
        g = torch.Generator(device=dev).manual_seed(99)
        W = t_prev + stride
        bank = KVBank(L, Hq, H, D, cap=W, device=dev, dtype=dt)
        for l0 in range(0, L, 8):
            bank.load_rows(torch.randn(8, H, t_prev, D, generator=g, device=dev).to(dt), torch.randn(8, H, t_prev, D, generator=g, device=dev).to(dt),
                           pos_begin=0, layer_begin=l0)
        bank.state_init(W, 2, stride)
        n = 16
        qs = torch.randn(n, L, Hq, stride, D, generator=g, device=dev).to(dt)
        ks, vs = (torch.randn(n, L, H, stride, D, generator=g, device=dev).to(dt) for _ in range(2))
        out = torch.empty(L, Hq, stride, D, dtype=dt, device=dev)
        ids = torch.empty(L, H, stride, dtype=torch.int32, device=dev)
        bp = t_prev
        plan = StepPlan(policy="roco", phase="prefill", accumulate=True, evict=True, budget=bp, recent=int(bp * 0.1), sink=4, stride=stride)
        return lambda i: bank.attend(plan, qs[i % n], ks[i % n], vs[i % n], out=out, evict_ids=ids)
    return make


def per_layer_maker(bank_dt, n, L=32, H=32, D=128, t_prev=2048):
    """One forward of a 32-layer stack, one attend() per layer, bf16 [1, H, n, D] views of [1, n, H * D] projections."""
    def make():
        from easykv_amd import BudgetedKVCache, StepPlan
        dev = torch.device("cuda")
        g = torch.Generator(device=dev).manual_seed(7)
        W = t_prev + n
        cache = BudgetedKVCache(L, H, H, D, W + 64, dev, dtype=bank_dt)
        for l0 in range(0, L, 8):
            cache.bank.load_rows(torch.randn(8, H, t_prev, D, generator=g, device=dev), torch.randn(8, H, t_prev, D, generator=g, device=dev),
                                 pos_begin=0, layer_begin=l0)
        if n == 1:
            cache.bank.state_init(W, 0)
            plan = StepPlan(policy="roco", phase="decode", evict=True, score_off=0, budget=t_prev)
        else:
            cache.bank.state_init(W, 2, n)
            plan = StepPlan(policy="roco", phase="prefill", accumulate=True, evict=True, budget=t_prev, recent=int(t_prev * 0.1), sink=4,
                            stride=n)
        proj = [tuple(torch.randn(1, n, H * D, generator=g, device=dev).to(torch.bfloat16).view(1, n, H, D).transpose(1, 2) for _ in range(3))
                for _ in range(4)]

        def forward(i):
            cache.begin_forward(plan)
            q, k, v = proj[i % 4]
            for l in range(L):      # (the HF seam hands the output back in the model's dtype: a conversion behind an fp16 bank)
                cache.attend(l, q, k, v).transpose(1, 2).to(torch.bfloat16)
        return forward
    return make


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=300)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    res = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "steps": args.steps}
    res["fused_decode_us"] = _interleave({k: decode_maker(dt) for k, dt in DTYPES.items()}, args.reps, args.steps, args.warm)
    res["configs1_chunk_us"] = _interleave({k: chunk_maker(dt, 32, 32, 32, 8, 2056) for k, dt in DTYPES.items()}, args.reps, args.steps, 50)
    res["configs2_chunk_us"] = _interleave({k: chunk_maker(dt, 32, 32, 8, 16, 1232) for k, dt in DTYPES.items()}, args.reps, args.steps, 50)
    for n, key in ((1, "per_layer_decode_us"), (8, "per_layer_stride8_us")):
        per_fwd = _interleave({"bf16_into_fp16_bank": per_layer_maker(torch.float16, n), "bf16_into_bf16_bank": per_layer_maker(torch.bfloat16, n)},
                              args.reps, max(4, args.steps // 4), 20)
        res[key] = {k: round(v / 32, 2) for k, v in per_fwd.items()}
    r = lambda leg, a="bf16", b="fp16": round(res[leg][a] / res[leg][b], 4)
    res["ratios"] = {"fused_decode": r("fused_decode_us"), "configs1": r("configs1_chunk_us"), "configs2": r("configs2_chunk_us"),
                     "per_layer_decode": r("per_layer_decode_us", "bf16_into_bf16_bank", "bf16_into_fp16_bank"),
                     "per_layer_stride8": r("per_layer_stride8_us", "bf16_into_bf16_bank", "bf16_into_fp16_bank")}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
