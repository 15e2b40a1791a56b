"""The fused decode step at head_dim 256 against head_dim 128 with twice the heads, in one process, timings interleaved (d256 rep, d128
rep, d256 rep, ...); writes profiles/d256_bench.json and prints it as one JSON line.

  * head_dim 256: 16 heads x 28 layers, budget 2048 (T = 2049), roco, scattered slot map, warm score state, pre-warm steps;
  * head_dim 128: 32 heads x 28 layers, everything else alike — the same K/V bytes, and the same score-row bytes per pair of heads.

Both legs keep their heads unsplit (n_split = 1: the one-launch step).  The launches differ in what the planner picks for their head
counts: 448 (head, layer) pairs run the 8-wave workgroups, 896 pairs the 4-wave ones; the head_dim-128 leg also has the phase orders and
the resident rows of the flagship instances, which no head_dim-256 instance has.  The yardstick of the head_dim-256 leg is the
head_dim-128 leg of the same run: per leg µs per launch (median of per-rep means, HIP events on the launch stream), the run-to-run
spread, the algorithmic bytes (tools/bench_common.algorithmic_bytes), GB/s and the fraction of the 8 TB/s HBM peak.

One figure per mode of the head_dim-256 chunk kernel at one shape (a stride-16 chunk step onto 2048 cached rows of the same bank
shape): the one-pass step (mode 0) and the two-pass step (modes 1 + 2, two launches timed together).  Nothing is compared with them.

Usage: python tools/bench_d256.py [--reps 15] [--steps 20] [--warm 300] [--out profiles/d256_bench.json]"""
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

from tools.bench_common import HBM_PEAK_GBS, algorithmic_bytes  # noqa: E402
from tools.bench_kv8 import _interleave, _time  # noqa: E402

LAYERS, BUDGET = 28, 2048


def make_bank(L, H, D, rows, cap, width, mode, stride=1):
    from easykv_amd import KVBank
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(1234)
    bank = KVBank(L, H, H, D, cap=cap, device=dev)
    for l0 in range(0, L, 4):
        bank.load_rows(torch.randn(4, H, rows, D, generator=g, device=dev).half(), torch.randn(4, H, rows, D, generator=g, device=dev).half(),
                       pos_begin=0, layer_begin=l0)
    bank.slot_of_pos[:, :, :rows] = torch.argsort(torch.rand(L, H, rows, generator=g, device=dev), dim=-1).int()      # scattered slot map
    bank.state_init(width, mode, stride)
    warm = torch.rand(L, H, rows, generator=g, device=dev) * 1e-3                                                     # warm score state
    bank.score_sum[:, :, :rows] += warm
    bank.score_sq[:, :, :rows] += warm ** 2
    return bank, g


def fused_step(H, D):
    from easykv_amd import StepPlan
    bank, g = make_bank(LAYERS, H, D, BUDGET, BUDGET + 1 + 63, BUDGET + 1, 0)
    dev, n = bank.device, 64
    qs, ks, vs = (torch.randn(n, LAYERS, H, 1, D, generator=g, device=dev).half() for _ in range(3))
    out = torch.empty(LAYERS, H, 1, D, dtype=torch.float16, device=dev)
    ids = torch.empty(LAYERS, H, 1, dtype=torch.int32, device=dev)
    plan = StepPlan(policy="roco", phase="decode", evict=True, score_off=0, budget=BUDGET, n_split=1)
    info = bank.step_info(plan, 1, 0, LAYERS)
    assert info["fused"] == 1 and info["n_launches"] == 1, (D, info)
    return (lambda i: bank.attend(plan, qs[i % n], ks[i % n], vs[i % n], out=out, evict_ids=ids)), bank


def chunk_step(H, D, stride, two_pass):
    """An evicting chunk step of the encoding rule onto BUDGET cached rows: the cache length is the same before and after."""
    from easykv_amd import StepPlan
    bank, g = make_bank(LAYERS, H, D, BUDGET, BUDGET + stride, BUDGET + stride, 2, stride)
    dev, n = bank.device, 8
    qs, ks, vs = (torch.randn(n, LAYERS, H, stride, D, generator=g, device=dev).half() for _ in range(3))
    plan = StepPlan(policy="roco", phase="prefill", accumulate=True, evict=True, budget=BUDGET, recent=BUDGET // 10, sink=4, stride=stride, two_pass=two_pass)
    info = bank.step_info(plan, stride, 0, LAYERS)
    assert info["wide"] == 0 and info["two_pass"] == (1 if two_pass == 1 else 0), info
    return (lambda i: bank.attend(plan, qs[i % n], ks[i % n], vs[i % n])), info


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=300)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "d256_bench.json"))
    args = ap.parse_args()
    torch.cuda.set_device(0)
    res = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "steps": args.steps, "warm": args.warm, "hbm_peak_gb_per_s": HBM_PEAK_GBS,
           "shape": f"{LAYERS} layers, budget {BUDGET} (T = {BUDGET + 1}), roco, scattered slot map, warm score state, heads unsplit (n_split = 1)"}
    legs = {"d256": (16, 256), "d128": (32, 128)}
    made = {k: fused_step(*hd) for k, hd in legs.items()}
    t = _interleave({k: f for k, (f, _) in made.items()}, args.reps, args.steps, args.warm)
    fused = {}
    for k, (H, D) in legs.items():
        bank = made[k][1]
        b = algorithmic_bytes(H, H, D, BUDGET + 1, 1, 3)["total"] * LAYERS
        gbs = b / (t[k]["us"] * 1e-6) / 1e9
        fused[k] = dict(heads=H, head_dim=D, head_layer_pairs=H * LAYERS, slot_indexed_rows=bool(all(bank._slot_rows)), us_per_launch=t[k]["us"],
                        run_to_run_spread=t[k]["spread"], bytes_per_launch=b, gb_per_s=round(gbs, 1), frac_of_hbm_peak=round(gbs / HBM_PEAK_GBS, 4))
    fused["time_ratio_d256_over_d128"] = round(fused["d256"]["us_per_launch"] / fused["d128"]["us_per_launch"], 4)
    fused["byte_ratio_d256_over_d128"] = round(fused["d256"]["bytes_per_launch"] / fused["d128"]["bytes_per_launch"], 4)
    res["fused_decode"] = fused
    del made
    gc.collect()
    torch.cuda.empty_cache()
    res["chunk_d256"] = {}
    for name, two_pass in (("one_pass_mode0", -1), ("two_pass_modes1_2", 1)):
        fn, info = chunk_step(16, 256, 16, two_pass)
        for i in range(5):
            fn(i)
        torch.cuda.synchronize()
        us = sorted(_time(fn, 10) for _ in range(5))[2]
        res["chunk_d256"][name] = dict(stride=16, cached_rows=BUDGET, heads=16, layers=LAYERS, us_per_step=round(us, 1), n_launches=info["n_launches"],
                                       n_split=info["n_split"], n_qblocks=info["n_qblocks"])
        del fn
        gc.collect()
        torch.cuda.empty_cache()
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
