"""The long-row call family (KVBank(long_rows=True)) against the plain family, in one process, legs interleaved on copies of the same
rows (plain rep, long rep, attention-only rep, plain rep, ...); writes profiles/long_rows_bench.json and prints it as one JSON line.

  (i)  One layer of 32 heads, head_dim 128, roco, W = 30 000 score columns — a width both families serve: the plain call runs the
       generic scorer's wide-row build (one 1024-thread workgroup per head, keys in LDS), the long call sweep + select.  A decode step,
       a stride-16 chunk step (one pass, exported logits) and a stride-96 chunk step (two passes, column sums).  Per leg the whole step
       and, from the same run, the step's attention + fold alone (phases = 1 | 4 on a third copy of the rows): scorer time = whole step
       minus attention + fold.  The yardstick is the plain leg of the same run.
  (ii) The long family alone at T = 65 537 and 131 073 (decode step): whole step, attention + fold, scorer.  The sweep and the select are
       two kernels of one call; their split needs a kernel trace (--only long_65537 under a profiler) and is not taken here.

Per leg: microseconds per step (median of per-rep means, HIP events on the launch stream) and the run-to-run spread (max - min over the median).

Usage: python tools/bench_long.py [--reps 9] [--steps 10] [--warm 20] [--only NAME] [--out profiles/long_rows_bench.json]"""
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


def make_step(long_rows, phases, H, D, W, stride):
    """One steady-state step on its own bank: every call appends `stride` rows and evicts as many (stride 1: a budgeted decode step)."""
    from easykv_amd import KVBank, StepPlan
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(1234)
    n = stride
    bank = KVBank(1, H, H, D, cap=W + n + 63, device=dev, long_rows=long_rows)
    bank.load_rows(torch.randn(1, H, W, D, generator=g, device=dev).half(), torch.randn(1, H, W, D, generator=g, device=dev).half())
    if n == 1:
        bank.state_init(W + 1, 0)
        plan = StepPlan(policy="roco", phase="decode", evict=True, budget=W)
    else:
        bank.state_init(W + n, 2, n)
        plan = StepPlan(policy="roco", phase="prefill", accumulate=True, evict=True, budget=W, recent=int(W * 0.1), sink=4, stride=n)
    warm = torch.rand(1, H, W, generator=g, device=dev) * 1e-3
    bank.score_sum[:, :, :W] += warm
    bank.score_sq[:, :, :W] += warm ** 2
    m = 8
    qs, ks, vs = (torch.randn(m, 1, H, n, D, generator=g, device=dev).half() for _ in range(3))
    out = torch.empty(1, H, n, D, dtype=torch.float16, device=dev)
    ids = torch.empty(1, H, n, dtype=torch.int32, device=dev)
    info = bank.step_info(plan, n)
    if phases == 0:
        assert not info["fused"] and info.get("long_scorer", 0) == int(long_rows), info
    # (phases = 1 | 4: attention + fold only — the new rows land in the same free slots every call, the slot map is untouched)
    return (lambda i: bank.attend(plan, qs[i % m], ks[i % m], vs[i % m], out=out, evict_ids=ids, phases=phases)), info


def compare(H, D, W, stride, reps, steps, warm, plain=True):
    fns, infos = {}, {}
    for name, (long_rows, phases) in dict(plain=(False, 0), long=(True, 0), attention_fold=(True, 5)).items():
        if name == "plain" and not plain:
            continue
        fns[name], infos[name] = make_step(long_rows, phases, H, D, W, stride)
    t = _interleave(fns, reps, steps, warm)
    del fns
    gc.collect()
    torch.cuda.empty_cache()
    res = dict(shape=f"1 layer x {H} heads, head_dim {D}, roco, W = {W}, {stride} new rows per step",
               plan={k: infos["long"][k] for k in ("n_split", "two_pass", "wide", "n_launches", "long_tiles")})
    att = t["attention_fold"]["us"]
    for name in t:
        res[name] = dict(us_per_step=t[name]["us"], run_to_run_spread=t[name]["spread"])
        if name != "attention_fold":
            res[name]["scorer_us"] = round(t[name]["us"] - att, 2)
    if plain:
        res["step_time_long_over_plain"] = round(t["long"]["us"] / t["plain"]["us"], 4)
        res["scorer_time_long_over_plain"] = round(res["long"]["scorer_us"] / res["plain"]["scorer_us"], 4)
        res["differs_by_more_than_the_plain_spread"] = bool(abs(1.0 - res["step_time_long_over_plain"]) > t["plain"]["spread"])
    else:
        res["scorer_over_attention_fold"] = round(res["long"]["scorer_us"] / att, 4)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warm", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "long_rows_bench.json"))
    ap.add_argument("--only", default=None, help="run one leg (nothing is written): decode_w30000, chunk16_w30000, chunk96_w30000, long_65537, long_131073")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    a = (args.reps, args.steps, args.warm)
    legs = {"decode_w30000": lambda: compare(32, 128, 30000, 1, *a),
            "chunk16_w30000": lambda: compare(32, 128, 30000, 16, *a),
            "chunk96_w30000": lambda: compare(32, 128, 30000, 96, *a),
            "long_65537": lambda: compare(32, 128, 65536, 1, *a, plain=False),
            "long_131073": lambda: compare(32, 128, 131072, 1, *a, plain=False)}
    res = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "steps": args.steps, "warm": args.warm,
           "method": "legs interleaved in one process on copies of the same rows; scorer_us = whole step - attention + fold (phases 1 | 4) of the same run"}
    for name, run in legs.items():
        if args.only in (None, name):
            res[name] = run()
    if args.only is None:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
