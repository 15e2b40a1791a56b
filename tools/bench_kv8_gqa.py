"""FP8 rows at GQA x 8 on the MFMA decode kernel (KVBank.quantize_fp8(grouped=True)) against the plain FP8 call, the 16-bit bank and
grouped MXFP4 rows, in one process over copies of the same rows, slot map and score state, timings interleaved (leg A rep, leg B rep,
...); writes profiles/kv8_gqa_bench.json and prints it as one JSON line.

  * shape: 64 query heads over 8 KV heads, T = 2049 (budget 2048), roco, scattered slot map, warm score state;
  * head_dim 128: all four legs; head_dim 64: grouped FP8 against plain FP8 (the other formats have no head_dim 64 build to compare);
  * forms: the 32-layer step (one attend over all layers), and the one-layer-per-call deferred form (attend(defer=True) per layer + one
    flush()), reported per layer.

Per leg: µs per step (median of per-rep means, HIP events), run-to-run spread, algorithmic bytes per step as tools/bench_kv4_gqa.py counts
them (the logits round trip of a split-path step included, the partials left out).

Usage: python tools/bench_kv8_gqa.py [--reps 15] [--steps 20] [--warm 300] [--out profiles/kv8_gqa_bench.json]"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools import bench_kv4_gqa as B  # noqa: E402

KINDS_128 = ("fp16", "fp8", "mxfp4_grouped", "fp8_grouped")
KINDS_64 = ("fp8", "fp8_grouped")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=300)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kv8_gqa_bench.json"))
    a = ap.parse_args()
    torch.cuda.set_device(0)
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "steps": a.steps, "warm": a.warm,
           "shape": "32 layers, 64 query / 8 KV heads, budget 2048 (T = 2049), roco, scattered slot map, warm score state"}
    for D, kinds in ((128, KINDS_128), (64, KINDS_64)):
        shape = dict(L=32, Hq=64, H=8, D=D, budget=2048)
        res[f"d{D}"] = {"step_32_layers": B.leg(B.whole_step, shape, kinds, a.reps, a.steps, a.warm),
                        "deferred_per_layer": B.leg(B.deferred_step, shape, kinds, a.reps, max(4, a.steps // 4), max(10, a.warm // 32), per=32)}
        # the claim to be shown: the grouped step beats the plain FP8 call by more than both legs' spreads
        for form, legs in list(res[f"d{D}"].items()):
            g, p = legs["fp8_grouped"], legs["fp8"]
            res[f"d{D}"][form + "_grouped_beats_plain_beyond_spreads"] = bool(
                g["us_per_step"] * (1 + g["run_to_run_spread"]) < p["us_per_step"] * (1 - p["run_to_run_spread"]))
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
