"""MXFP4 rows at GQA x 8 on the MFMA decode kernel (KVBank.quantize_mxfp4(grouped=True)) against FP8 rows, FP8-key / MXFP4-value rows and
the 16-bit bank, in one process over copies of the same rows, slot map and score state, timings interleaved (leg A rep, leg B rep, ...);
writes profiles/kv4_gqa_bench.json and prints it as one JSON line.

  * shape: 64 query heads over 8 KV heads, head_dim 128, T = 2049 (budget 2048), roco, scattered slot map, warm score state;
  * forms: the 32-layer step (one attend over all layers), and the one-layer-per-call deferred form (attend(defer=True) per layer + one
    flush()), reported per layer.

Per leg: µs per step (median of per-rep means, HIP events), run-to-run spread, algorithmic bytes per step (tools/bench_kv8.step_bytes:
K/V rows once, the appended row, q / out, the score rows once in and once out).  A leg that is not one launch also writes its fp32 logits
to the workspace and reads them back in the scorer — Hq * t_pad * 4 bytes per layer, each way — which `logit_bytes_per_step` states and
`bytes_per_step` includes; the (m, l, o) partials (Hq * n_split * 130 floats per layer) are left out.

Usage: python tools/bench_kv4_gqa.py [--reps 15] [--steps 20] [--warm 300] [--out profiles/kv4_gqa_bench.json]"""
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

from tools.bench_kv8 import _interleave, step_bytes  # noqa: E402

KINDS = ("fp16", "fp8", "fp8_mxfp4", "mxfp4_grouped")
# the grouped legs (tools/bench_kv8_gqa.py runs the second): the row format whose rows and bytes they are
GROUPED = {"mxfp4_grouped": "mxfp4", "fp8_grouped": "fp8"}


def make_bank(kind, L, Hq, H, D, budget):
    from easykv_amd import KVBank
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(1234)
    T = budget + 1
    bank = KVBank(L, Hq, H, D, cap=T + 63, device=dev)
    bank.load_rows(torch.randn(L, H, budget, D, generator=g, device=dev).half(), torch.randn(L, H, budget, D, generator=g, device=dev).half())
    bank.slot_of_pos[:, :, :budget] = torch.argsort(torch.rand(L, H, budget, generator=g, device=dev), dim=-1).int()      # scattered slot map
    bank.state_init(T, 0)
    warm = torch.rand(L, H, budget, generator=g, device=dev) * 1e-3
    bank.score_sum[:, :, :budget] += warm
    bank.score_sq[:, :, :budget] += warm ** 2
    if kind in GROUPED:
        (bank.quantize_mxfp4 if GROUPED[kind] == "mxfp4" else bank.quantize_fp8)(grouped=True)
    elif kind != "fp16":
        bank.quantize(kind)
    return bank, g


def whole_step(kind, L, Hq, H, D, budget):
    from easykv_amd import StepPlan
    bank, g = make_bank(kind, L, Hq, H, D, budget)
    n = 16
    qs = torch.randn(n, L, Hq, 1, D, generator=g, device=bank.device).half()
    ks, vs = (torch.randn(n, L, H, 1, D, generator=g, device=bank.device).half() for _ in range(2))
    out = torch.empty(L, Hq, 1, D, dtype=torch.float16, device=bank.device)
    ids = torch.empty(L, H, 1, dtype=torch.int32, device=bank.device)
    plan = StepPlan(policy="roco", phase="decode", evict=True, score_off=0, budget=budget)
    fn = lambda i: bank.attend(plan, qs[i % n], ks[i % n], vs[i % n], out=out, evict_ids=ids)
    fn.info = bank.step_info(plan, 1, 0, L)
    return fn


def deferred_step(kind, L, Hq, H, D, budget):
    from easykv_amd import StepPlan
    bank, g = make_bank(kind, L, Hq, H, D, budget)
    n = 8
    qs = torch.randn(n, L, 1, Hq, 1, D, generator=g, device=bank.device).half()
    ks, vs = (torch.randn(n, L, 1, H, 1, D, generator=g, device=bank.device).half() for _ in range(2))
    out = torch.empty(1, Hq, 1, D, dtype=torch.float16, device=bank.device)
    plan = StepPlan(policy="roco", phase="decode", evict=True, score_off=0, budget=budget)

    def forward(i):
        for l in range(L):
            bank.attend(plan, qs[i % n][l], ks[i % n][l], vs[i % n][l], layer_begin=l, defer=True, out=out)
        bank.flush()
    forward.info = bank.step_info(plan, 1, 0, 1, phases=5)
    return forward


def leg(maker, shape, kinds, reps, steps, warm, per=1):
    fns = {k: maker(k, **shape) for k in kinds}
    plans = {k: f.info for k, f in fns.items()}
    t = _interleave(fns, reps, steps, warm)
    del fns
    gc.collect()
    torch.cuda.empty_cache()
    res = {}
    for k in kinds:
        T = shape["budget"] + 1
        b = step_bytes(GROUPED.get(k, k), shape["L"], shape["H"], shape["Hq"], shape["D"], T)
        # (a split-path step: the logits go through the workspace, written by the attention kernel and read by the scorer; t_pad = T rounded to 64)
        logit = 0 if plans[k]["fused"] else 2 * shape["L"] * shape["Hq"] * ((T + 63) // 64 * 64) * 4
        res[k] = dict(us_per_step=round(t[k]["us"] / per, 2), run_to_run_spread=t[k]["spread"], bytes_per_step=(b["total"] + logit) // per,
                      kv_bytes_per_step=b["kv"] // per, logit_bytes_per_step=logit // per, n_split=plans[k]["n_split"], one_launch=plans[k]["fused"], launches=plans[k]["n_launches"])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=300)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kv4_gqa_bench.json"))
    a = ap.parse_args()
    torch.cuda.set_device(0)
    shape = dict(L=32, Hq=64, H=8, D=128, budget=2048)
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "steps": a.steps, "warm": a.warm,
           "shape": "32 layers, 64 query / 8 KV heads, head_dim 128, budget 2048 (T = 2049), roco, scattered slot map, warm score state",
           "step_32_layers": leg(whole_step, shape, KINDS, a.reps, a.steps, a.warm),
           "deferred_per_layer": leg(deferred_step, shape, KINDS, a.reps, max(4, a.steps // 4), max(10, a.warm // 32), per=32)}
    g8 = res["step_32_layers"]
    res["mxfp4_faster_than_fp8_at_gqa8"] = bool(g8["mxfp4_grouped"]["us_per_step"] < g8["fp8"]["us_per_step"])
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
