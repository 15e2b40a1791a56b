"""Sink decode steps against their plain twins, in one process, the legs interleaved (sink rep, plain rep, ...) on banks filled with copies
of the same rows; writes profiles/sink_bench.json and prints it as one JSON line.

The fused decode step with attention sinks (N(0, 1) + 1 per head) against the plain step: gpt-oss's shape — head_dim 64, 64 query heads
over 8 KV heads, 24 layers — and head_dim 128 (32 heads x 32 layers), budget 2048 (T = 2049), roco, scattered slot map, warm score state,
heads unsplit (n_split = 1; a GQA x 8 step is then attention + scorer, two launches).  A sink decode step plans as the plain one except for the phase order and the resident rows, which the sink
instances are built without: the plain leg of the head_dim-128 pair runs with them, and `plan` records both legs' info.
Expectation: one extra exponential per query head and workgroup, inside the plain leg's run-to-run spread; there is no pass bar — the ratio
is recorded as it comes out.

Per leg: µs per launch (median of per-rep means, HIP events on the launch stream) and the run-to-run spread.

Usage: python tools/bench_sink.py [--reps 11] [--steps 20] [--warm 200] [--out profiles/sink_bench.json]"""
from __future__ import annotations

import argparse
import gc
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.bench_kv8 import _interleave  # noqa: E402

BUDGET = 2048


def fused_step(L, Hq, H, D, with_sinks):
    from easykv_amd import KVBank, StepPlan
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(1234)      # (the same rows in both legs of a pair)
    sinks = torch.randn(L, Hq, generator=torch.Generator().manual_seed(11)) + 1
    bank = KVBank(L, Hq, H, D, cap=BUDGET + 1 + 63, device=dev, **(dict(sinks=sinks) if with_sinks else {}))
    for l0 in range(0, L, 4):
        bank.load_rows(torch.randn(4, H, BUDGET, D, generator=g, device=dev).half(), torch.randn(4, H, BUDGET, D, generator=g, device=dev).half(),
                       pos_begin=0, layer_begin=l0)
    bank.slot_of_pos[:, :, :BUDGET] = torch.argsort(torch.rand(L, H, BUDGET, generator=g, device=dev), dim=-1).int()
    bank.state_init(BUDGET + 1, 0, 1)
    warm = torch.rand(L, H, BUDGET, generator=g, device=dev) * 1e-3
    bank.score_sum[:, :, :BUDGET] += warm
    bank.score_sq[:, :, :BUDGET] += warm ** 2
    n = 64
    qs = torch.randn(n, L, Hq, 1, D, generator=g, device=dev).half()
    ks, vs = (torch.randn(n, L, H, 1, D, generator=g, device=dev).half() for _ in range(2))
    out = torch.empty(L, Hq, 1, D, dtype=torch.float16, device=dev)
    ids = torch.empty(L, H, 1, dtype=torch.int32, device=dev)
    plan = StepPlan(policy="roco", phase="decode", evict=True, score_off=0, budget=BUDGET, n_split=1)
    info = bank.step_info(plan, 1, 0, L)
    return (lambda i: bank.attend(plan, qs[i % n], ks[i % n], vs[i % n], out=out, evict_ids=ids)), bank, info


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sink_bench.json"))
    args = ap.parse_args()
    torch.cuda.set_device(0)
    res = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "steps": args.steps, "warm": args.warm, "sinks": "N(0, 1) + 1 per (layer, query head)",
           "shape": f"budget {BUDGET} (T = {BUDGET + 1}), roco, scattered slot map, warm score state, n_split = 1"}
    res["fused_decode"] = {}
    for name, (L, Hq, H, D) in (("d64_64over8_x24", (24, 64, 8, 64)), ("d128_32x32", (32, 32, 32, 128))):
        made = {"sink": fused_step(L, Hq, H, D, True), "plain": fused_step(L, Hq, H, D, False)}
        t = _interleave({k: f for k, (f, _, _) in made.items()}, args.reps, args.steps, args.warm)
        row = {k: dict(us_per_launch=t[k]["us"], run_to_run_spread=t[k]["spread"], slot_indexed_rows=bool(all(made[k][1]._slot_rows)), plan=made[k][2])
               for k in made}
        row["time_ratio_sink_over_plain"] = round(t["sink"]["us"] / t["plain"]["us"], 4)
        res["fused_decode"][name] = row
        made.clear()
        gc.collect()
        torch.cuda.empty_cache()
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
