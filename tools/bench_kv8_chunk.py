"""Steady-state chunk steps (strided prefill with eviction: T stays at the budget) on 16-bit rows against FP8 rows
(KVBank(kv_quant='fp8', quant_chunks=True): ekv_chunk8_kernel), interleaved in one process on the same rows, slot map and score state
(fp16 rep, fp8 rep, fp16 rep, ...); writes profiles/kv8_chunk_bench.json and prints it as one JSON line.

  * llama7b_s8: the chunk step per 32-layer launch at the Llama2-7B shape (32 KV heads, GQA 1, head_dim 128), stride 8, budget 2048 —
    the 16-bit leg runs the one-launch logits-in-LDS kernel there, the FP8 leg the new kernel;
  * mistral_s16: 32 layers x 8 KV heads, GQA 4, head_dim 128, stride 16;
  * llama7b_s8_per_layer: the one-layer-per-call form of a 32-layer stack (attend per layer as a decoder stack issues it: deferred +
    one flush where the cache defers, else whole steps), per layer.

Every leg runs in a child process of its own under a time limit; the parent starts nothing more after a child that did not end
normally.  Per leg and row format: us per launch (median of per-rep means, HIP events), run-to-run spread, K/V bytes and algorithmic
bytes per launch from the shapes (K/V rows read once, the chunk's rows, q / out, the score rows once in and once out, the exported
logits once out and once in where the step exports them), what the library planned (ekv_step_info), and whether the difference is
outside the spread.

Usage: python tools/bench_kv8_chunk.py [--reps 9] [--steps 20] [--warm 60] [--timeout 240] [--out profiles/kv8_chunk_bench.json]"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

LEGS = {"llama7b_s8": dict(L=32, H=32, rep=1, D=128, budget=2048, stride=8, per_layer=False),
        "mistral_s16": dict(L=32, H=8, rep=4, D=128, budget=2048, stride=16, per_layer=False),
        "llama7b_s8_per_layer": dict(L=32, H=32, rep=1, D=128, budget=2048, stride=8, per_layer=True)}


def step_bytes(kind, info, L, H, rep, D, T, n):
    """Algorithmic bytes of one chunk step over L layers: T rows after the append, n of them the chunk's own."""
    pair = 2 * D + 8 if kind == "fp8" else 4 * D
    kv = H * (T - n) * pair
    in_lds = kind == "fp16" and info["fused"] and not info["two_pass"] and rep * n <= 8      # (the logits-in-LDS kernel; two passes: column sums instead)
    logits = 0 if in_lds else (2 * 2 * H * T * 4 if info["two_pass"] else 2 * H * rep * n * T * 4)
    total = kv + H * n * (4 * D + pair) + 2 * H * rep * n * D * 2 + 2 * 3 * H * T * 4 + logits
    return dict(kv=kv * L, total=total * L)


def make_bank(kind, L, H, rep, D, budget, stride):
    import torch
    from easykv_amd import KVBank
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(1234)
    bank = KVBank(L, H * rep, H, D, cap=budget + stride + 56, device=dev)
    for l0 in range(0, L, 8):
        bank.load_rows(torch.randn(8, H, budget, D, generator=g, device=dev).half(), torch.randn(8, H, budget, D, generator=g, device=dev).half(),
                       pos_begin=0, layer_begin=l0)
    bank.slot_of_pos[:, :, :budget] = torch.argsort(torch.rand(L, H, budget, generator=g, device=dev), dim=-1).int()      # scattered slot map
    bank.state_init(budget + stride, 2, stride)
    warm = torch.rand(L, H, budget, generator=g, device=dev) * 1e-3
    bank.score_sum[:, :, :budget] += warm
    bank.score_sq[:, :, :budget] += warm ** 2
    if kind == "fp8":
        bank.quantize_fp8(chunks=True)
    return bank, g


def make_step(kind, L, H, rep, D, budget, stride, per_layer):
    import torch
    from easykv_amd import StepPlan
    bank, g = make_bank(kind, L, H, rep, D, budget, stride)
    dev, m = bank.device, 8
    plan = StepPlan(policy="roco", phase="prefill", accumulate=True, evict=True, budget=budget, recent=budget // 10, sink=4, stride=stride)
    info = bank.step_info(plan, stride, 0, 1 if per_layer else L)
    if not per_layer:
        qs, ks, vs = (torch.randn(m, L, hh, stride, D, generator=g, device=dev).half() for hh in (H * rep, H, H))
        out = torch.empty(L, H * rep, stride, D, dtype=torch.float16, device=dev)
        return (lambda i: bank.attend(plan, qs[i % m], ks[i % m], vs[i % m], out=out, evict_ids=False)), info
    qs, ks, vs = (torch.randn(m, L, 1, hh, stride, D, generator=g, device=dev).half() for hh in (H * rep, H, H))
    out = torch.empty(1, H * rep, stride, D, dtype=torch.float16, device=dev)
    defer = not info["fused"]      # (what BudgetedKVCache does: a step that is one launch already is not deferred)

    def forward(i):
        q, k, v = qs[i % m], ks[i % m], vs[i % m]
        for l in range(L):
            bank.attend(plan, q[l], k[l], v[l], layer_begin=l, out=out, **(dict(defer=True) if defer else dict(evict_ids=False)))
        if defer:
            bank.flush()
    info = dict(info, deferred=defer)
    return forward, info


def run_leg(name, reps, steps, warm):
    import torch
    torch.cuda.set_device(0)
    shape = LEGS[name]
    fns, infos = {}, {}
    for kind in ("fp16", "fp8"):
        fns[kind], infos[kind] = make_step(kind, **shape)
    for f in fns.values():
        for i in range(warm):
            f(i)
    torch.cuda.synchronize()
    got = {k: [] for k in fns}
    for _ in range(reps):
        for k, f in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for i in range(steps):
                f(i)
            b.record()
            b.synchronize()
            got[k].append(a.elapsed_time(b) * 1e3 / steps)
    per = shape["L"] if shape["per_layer"] else 1
    res = {}
    for kind, v in got.items():
        med = statistics.median(v)
        b = step_bytes(kind, infos[kind], shape["L"], shape["H"], shape["rep"], shape["D"], shape["budget"] + shape["stride"], shape["stride"])
        res[kind] = dict(us_per_launch=round(med / per, 2), run_to_run_spread=round((max(v) - min(v)) / med, 4), kv_bytes_per_launch=b["kv"] // per,
                         bytes_per_launch=b["total"] // per, gb_per_s=round(b["total"] / (med * 1e-6) / 1e9, 1),
                         plan={k: infos[kind][k] for k in ("n_split", "fused", "two_pass", "wide", "n_qblocks", "n_launches")} | ({"deferred": infos[kind]["deferred"]} if "deferred" in infos[kind] else {}))
    ratio = res["fp8"]["us_per_launch"] / res["fp16"]["us_per_launch"]
    res["time_ratio_fp8_over_fp16"] = round(ratio, 4)
    res["kv_byte_ratio_fp8_over_fp16"] = round(res["fp8"]["kv_bytes_per_launch"] / res["fp16"]["kv_bytes_per_launch"], 4)
    res["byte_ratio_fp8_over_fp16"] = round(res["fp8"]["bytes_per_launch"] / res["fp16"]["bytes_per_launch"], 4)
    res["outside_the_spread"] = bool(abs(1.0 - ratio) > max(res["fp16"]["run_to_run_spread"], res["fp8"]["run_to_run_spread"]))
    res["shape"] = shape
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=60)
    ap.add_argument("--timeout", type=int, default=240, help="seconds a leg's child process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kv8_chunk_bench.json"))
    ap.add_argument("--leg", default=None, help="(child) run this leg and print its JSON")
    args = ap.parse_args()
    if args.leg is not None:
        print("LEG " + json.dumps(run_leg(args.leg, args.reps, args.steps, args.warm)))
        return 0
    res = dict(reps=args.reps, steps=args.steps, warm=args.warm)
    for name in LEGS:
        cmd = [sys.executable, os.path.abspath(__file__), "--leg", name, "--reps", str(args.reps), "--steps", str(args.steps), "--warm", str(args.warm)]
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout, cwd=ROOT)
        except subprocess.TimeoutExpired:
            res[name] = dict(error=f"no result within {args.timeout} s")
            break
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("LEG ")]
        if p.returncode != 0 or not line:      # (a leg that did not end normally: nothing more is started on the device)
            res[name] = dict(error=f"exit status {p.returncode}", stderr=p.stderr[-2000:])
            break
        res[name] = json.loads(line[0][4:])
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))
    return 0 if all("error" not in v for v in res.values() if isinstance(v, dict)) else 1


if __name__ == "__main__":
    sys.exit(main())
