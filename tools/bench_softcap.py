"""Soft-capped steps against their uncapped twins, in one process, the legs interleaved (capped rep, uncapped rep, ...) on banks filled
with copies of the same rows; writes profiles/softcap_bench.json and prints it as one JSON line.

  * the fused decode step, capped (cap 50) against uncapped: head_dim 256 (16 heads x 28 layers) and head_dim 128 (32 heads x 32 layers),
    budget 2048 (T = 2049), roco, scattered slot map, warm score state, heads unsplit (n_split = 1).  Both legs of a pair run the same
    plan (a capped decode step plans as the uncapped one); the yardstick of the capped leg is the uncapped leg of the same run;
  * one chunk step per scheme of the capped 16x16 kernel (one pass: mode 0 + scorer; two passes: modes 1 + 2), stride 16 onto 2048 cached
    rows, against the uncapped step of the same bank shape under the same forced scheme, at head_dim 256 and 128.  `same_plan` says
    whether the two legs report the same plan (at this stride the uncapped step of either head_dim runs the 16x16 kernel as well); a pair
    whose plans differ is reported as what it is.

Per leg: µs per launch / step (median of per-rep means, HIP events on the launch stream) and the run-to-run spread.

Usage: python tools/bench_softcap.py [--reps 11] [--steps 20] [--warm 200] [--out profiles/softcap_bench.json]"""
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

BUDGET, CAP = 2048, 50.0


def make_bank(L, H, D, rows, cap_rows, width, mode, stride, logit_cap):
    from easykv_amd import KVBank
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(1234)      # (the same rows in both legs of a pair)
    bank = KVBank(L, H, H, D, cap=cap_rows, device=dev, **(dict(logit_cap=logit_cap) if logit_cap else {}))
    for l0 in range(0, L, 4):
        bank.load_rows(torch.randn(4, H, rows, D, generator=g, device=dev).half(), torch.randn(4, H, rows, D, generator=g, device=dev).half(),
                       pos_begin=0, layer_begin=l0)
    bank.slot_of_pos[:, :, :rows] = torch.argsort(torch.rand(L, H, rows, generator=g, device=dev), dim=-1).int()
    bank.state_init(width, mode, stride)
    warm = torch.rand(L, H, rows, generator=g, device=dev) * 1e-3
    bank.score_sum[:, :, :rows] += warm
    bank.score_sq[:, :, :rows] += warm ** 2
    return bank, g


def fused_step(L, H, D, logit_cap):
    from easykv_amd import StepPlan
    bank, g = make_bank(L, H, D, BUDGET, BUDGET + 1 + 63, BUDGET + 1, 0, 1, logit_cap)
    dev, n = bank.device, 64
    qs, ks, vs = (torch.randn(n, L, H, 1, D, generator=g, device=dev).half() for _ in range(3))
    out = torch.empty(L, H, 1, D, dtype=torch.float16, device=dev)
    ids = torch.empty(L, H, 1, dtype=torch.int32, device=dev)
    plan = StepPlan(policy="roco", phase="decode", evict=True, score_off=0, budget=BUDGET, n_split=1)
    info = bank.step_info(plan, 1, 0, L)
    assert info["fused"] == 1 and info["n_launches"] == 1, (D, info)
    return (lambda i: bank.attend(plan, qs[i % n], ks[i % n], vs[i % n], out=out, evict_ids=ids)), bank


def chunk_step(L, H, D, stride, two_pass, logit_cap):
    from easykv_amd import StepPlan
    bank, g = make_bank(L, H, D, BUDGET, BUDGET + stride, BUDGET + stride, 2, stride, logit_cap)
    dev, n = bank.device, 8
    qs, ks, vs = (torch.randn(n, L, H, stride, D, generator=g, device=dev).half() for _ in range(3))
    plan = StepPlan(policy="roco", phase="prefill", accumulate=True, evict=True, budget=BUDGET, recent=BUDGET // 10, sink=4, stride=stride, two_pass=two_pass)
    info = bank.step_info(plan, stride, 0, L)
    return (lambda i: bank.attend(plan, qs[i % n], ks[i % n], vs[i % n])), info


def _free(*objs):
    del objs
    gc.collect()
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "softcap_bench.json"))
    args = ap.parse_args()
    torch.cuda.set_device(0)
    res = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "steps": args.steps, "warm": args.warm, "logit_cap": CAP,
           "shape": f"budget {BUDGET} (T = {BUDGET + 1}), roco, scattered slot map, warm score state"}
    res["fused_decode"] = {}
    for name, (L, H, D) in (("d256_16x28", (28, 16, 256)), ("d128_32x32", (32, 32, 128))):
        made = {"capped": fused_step(L, H, D, CAP), "uncapped": fused_step(L, H, D, None)}
        t = _interleave({k: f for k, (f, _) in made.items()}, args.reps, args.steps, args.warm)
        res["fused_decode"][name] = {k: dict(us_per_launch=t[k]["us"], run_to_run_spread=t[k]["spread"], slot_indexed_rows=bool(all(made[k][1]._slot_rows)))
                                     for k in made}
        res["fused_decode"][name]["time_ratio_capped_over_uncapped"] = round(t["capped"]["us"] / t["uncapped"]["us"], 4)
        made.clear()
        _free()
    res["chunk_step"] = {}
    for name, (L, H, D, two_pass) in (("d256_one_pass", (28, 16, 256, -1)), ("d256_two_pass", (28, 16, 256, 1)),
                                      ("d128_one_pass", (32, 32, 128, -1)), ("d128_two_pass", (32, 32, 128, 1))):
        made = {"capped": chunk_step(L, H, D, 16, two_pass, CAP), "uncapped": chunk_step(L, H, D, 16, two_pass, None)}
        t = _interleave({k: f for k, (f, _) in made.items()}, max(3, args.reps // 2), max(4, args.steps // 2), 10)
        same = all(made["capped"][1][k] == made["uncapped"][1][k] for k in ("wide", "two_pass", "n_qblocks", "qb_rows", "n_split", "n_launches", "fused"))
        res["chunk_step"][name] = {k: dict(us_per_step=t[k]["us"], run_to_run_spread=t[k]["spread"], plan=made[k][1]) for k in made}
        res["chunk_step"][name]["same_plan"] = same
        res["chunk_step"][name]["time_ratio_capped_over_uncapped"] = round(t["capped"]["us"] / t["uncapped"]["us"], 4)
        made.clear()
        _free()
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
