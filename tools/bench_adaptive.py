"""Adaptive head budgets: the selection step against the pooled step, and the decode call over heads of different lengths against the
deferred per-layer call of a uniform bank, in one process with the legs interleaved; writes profiles/adaptive_bench.json (or --out) and
prints it as one JSON line.

(1) The selection (`selection`).  One observation step of the Llama2-7B shape — 32 layers x 32 heads, head_dim 128, 32 queries over T = 4096
    keys, h2o_head, n_evict = 2048, sink 4, kernel size 7 (radius 3) — through the pooled call and through the adaptive call with the
    driver's bounds (floor 0.2, ceiling 2.0 of the uniform candidate keep) and with degenerate bounds.  Every repetition restores the
    bank's length and re-initialises the score rows (tools/bench_oneshot.py's leg), so a leg is state_init + attention + its ending; the
    legs differ in the ending alone: one pooled scorer launch against rank + allot + select.  µs per step: median of per-rep means (HIP
    events) with the run-to-run spread.
(2) The three launches (`kernels`).  One adaptive and one pooled step under torch.profiler: device µs of the rank and select launches (the
    two launches of the EKV_ADA scorer kernel, in launch order), of the allot kernel and of the pooled scorer kernel.  A profiler that
    records no device kernels leaves the entry saying so.
(3) The decode call (`decode`).  32 layers x 32 heads at a mean of 2048 rows per head: a bank whose heads alternate 1024 / 3072 rows, one
    evicting h2o_head decode step = 32 calls of the batched call on the bank seen as L * H one-head layers, against a uniform bank of
    2048 rows per head stepped one layer per call with the scorer deferred to one flush.  Same total rows, legs interleaved.
    A third, interleaved leg steps the same ragged bank one layer per call through the heads family (ekv_heads_*: attend(defer=True) per
    layer, one flush); the three legs, their spreads and the ratios deferred / view and deferred / uniform also go to profiles/heads_bench.json
    (--heads-out).  Both deferred legs take a fresh StepPlan every token, as the driver does.
(4) The prefill (`prefill`, --model-layers > 0).  tools/bench_oneshot.py's Llama2-7B-shaped random-init HF model through the seam, a
    4096-token prompt cut to 2048 in encoding mode with h2o_head, one-shot (obs_window 32, score_pool 7), max_new_tokens = 1 (one decode
    forward in either leg): without the key and with generation_config['head_budgets'] = 'adaptive'.  Wall seconds per generate call,
    host-synchronised, legs interleaved.

--parts picks the parts that run (default: all of selection,decode,prefill).  A run of some parts only leaves profiles/adaptive_bench.json,
the record of all of them, alone unless --out names a file.

Usage: python tools/bench_adaptive.py [--reps 7] [--steps 5] [--warm 3] [--model-layers 32] [--prefill-reps 3] [--parts selection,decode,prefill]
       [--out profiles/adaptive_bench.json] [--heads-out profiles/heads_bench.json]"""
from __future__ import annotations

import argparse
import dataclasses
import json
import math
import os
import re
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.bench_kv8 import _interleave  # noqa: E402
from tools.bench_oneshot import D, H, L, N_EVICT, OBS, SINK, T, wall  # noqa: E402


def bounds(floor=0.2, ceil=2.0):
    C = T - OBS - SINK
    K = C - N_EVICT
    return max(0, C - math.ceil(ceil * K)), C - math.floor(floor * K)


def selection_leg(adaptive):
    from easykv_amd import KVBank, StepPlan
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(1234)      # (the same rows in every leg)
    bank = KVBank(L, H, H, D, cap=T + 8, device=dev)
    for l0 in range(0, L, 4):
        bank.load_rows(torch.randn(4, H, T - OBS, D, generator=g, device=dev).half(), torch.randn(4, H, T - OBS, D, generator=g, device=dev).half(),
                       pos_begin=0, layer_begin=l0)
    # queries scaled by head, so that the heads' shares differ (peaked heads give more rows)
    scale = (2.0 ** torch.linspace(-4, 3, H, device=dev)).reshape(1, H, 1, 1)
    q = (torch.randn(L, H, OBS, D, generator=g, device=dev) * scale).half()
    k, v = (torch.randn(L, H, OBS, D, generator=g, device=dev).half() for _ in range(2))
    out = torch.empty(L, H, OBS, D, dtype=torch.float16, device=dev)
    ids = torch.full((L, H, adaptive[1] if adaptive else N_EVICT), -1, dtype=torch.int32, device=dev)
    plan = StepPlan(policy="h2o_head", phase="prefill", accumulate=True, evict=True, budget=T, recent=OBS, sink=SINK, stride=OBS, n_evict=N_EVICT,
                    pool=7, pool_op="max", head_adaptive=adaptive)
    info = bank.step_info(plan, OBS, 0, L)

    def step(i):
        bank.n_slots[:] = [T - OBS] * L      # (the rows of the last repetition's victims are free rows again: any permutation serves)
        bank.head_slots = None
        bank.state_init(T, 2, OBS)
        bank.attend(plan, q, k, v, out=out, evict_ids=ids)
    return step, bank, info


def kernel_split(legs):
    """Device µs of the scorer kernels of one step of each leg, by kernel name, in launch order."""
    from torch.profiler import ProfilerActivity, profile
    found = {}
    for name, step in legs.items():
        step(0)
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            step(0)
            torch.cuda.synchronize()
        ev = sorted((e for e in prof.events() if "ekv_score" in e.name), key=lambda e: e.time_range.start)
        found[name] = [dict(kernel=re.search(r"ekv_score\w+", e.name).group(0), us=round(float(getattr(e, "device_time", 0) or getattr(e, "cuda_time", 0)), 2)) for e in ev]
    return found


def decode_legs(budget=2048):
    from easykv_amd import KVBank, StepPlan
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(99)
    lens = [budget // 2 if h % 2 == 0 else budget + budget // 2 for h in range(H)]
    rows = max(lens)
    plan = StepPlan(policy="h2o_head", phase="decode", evict=True, score_off=0, budget=budget // 2, n_split=0)
    q = torch.randn(L, H, 1, D, generator=g, device=dev).half()
    k, v = (torch.randn(L, H, 1, D, generator=g, device=dev).half() for _ in range(2))

    def make(n):
        bank = KVBank(L, H, H, D, cap=n + 8, device=dev)
        bank.use_slot_rows = False
        for l0 in range(0, L, 4):
            bank.load_rows(torch.randn(4, H, n, D, generator=g, device=dev).half(), torch.randn(4, H, n, D, generator=g, device=dev).half(),
                           pos_begin=0, layer_begin=l0)
        bank.score_sum[:, :, :n] = torch.rand(L, H, n, generator=g, device=dev) + 0.5
        return bank
    ragged, uniform = make(rows), make(budget)
    for h, t in enumerate(lens):
        ragged.score_sum[:, h, t:] = 0
    ragged.head_slots = [list(lens) for _ in range(L)]
    ragged.n_slots = [rows] * L

    def step_ragged(i):
        for l in range(L):
            ragged.attend(plan, q[l:l + 1], k[l:l + 1], v[l:l + 1], layer_begin=l, evict_ids=False)

    def step_uniform(i):
        p = dataclasses.replace(plan)
        for l in range(L):
            uniform.attend(p, q[l:l + 1], k[l:l + 1], v[l:l + 1], layer_begin=l, defer=True)
        uniform.flush()

    def step_heads(i):
        p = dataclasses.replace(plan)
        for l in range(L):
            ragged.attend(p, q[l:l + 1], k[l:l + 1], v[l:l + 1], layer_begin=l, defer=True)
        ragged.flush()
    return {"ragged_view_per_layer": step_ragged, "uniform_deferred_per_layer": step_uniform, "ragged_heads_deferred_per_layer": step_heads}, lens, ragged


def prefill_legs(layers, prompt, budget):
    import contextlib
    import io
    from transformers import LlamaConfig, LlamaForCausalLM
    import easykv_amd
    from easykv_amd import hf

    class Tok:
        eos_token_id = -1

        def decode(self, ids, skip_special_tokens=True):
            return " ".join(map(str, ids))
    cfg = LlamaConfig(vocab_size=32000, hidden_size=4096, intermediate_size=11008, num_hidden_layers=layers, num_attention_heads=32,
                      num_key_value_heads=32, max_position_embeddings=8192, attn_implementation="sdpa")
    torch.manual_seed(0)
    with torch.device("cuda"):
        model = LlamaForCausalLM(cfg).half().eval()
    hf.patch_model(model)
    ids = torch.randint(0, 32000, (1, prompt), device="cuda", generator=torch.Generator("cuda").manual_seed(5))
    base = dict(budget=budget, kv_policy="h2o_head", max_new_tokens=1, eos_token_ids=[-1], temperature=1e-6, prefill="one_shot", obs_window=32, score_pool=7)

    def leg(extra):
        def run(_):
            easykv_amd.enable_fixed_kv(model, Tok(), mode="encoding", stride=8)
            with contextlib.redirect_stdout(io.StringIO()):
                model.easykv_generate(input_ids=ids, generation_config=dict(base, **extra))
        return run
    return {"one_shot_uniform": leg({}), "one_shot_adaptive": leg(dict(head_budgets="adaptive"))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--model-layers", type=int, default=32)
    ap.add_argument("--prefill-reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--heads-out", default=os.path.join(ROOT, "profiles", "heads_bench.json"))
    ap.add_argument("--parts", default="selection,decode,prefill")
    args = ap.parse_args()
    parts = set(args.parts.split(","))
    if args.out is None and parts >= {"selection", "decode", "prefill"}:
        args.out = os.path.join(ROOT, "profiles", "adaptive_bench.json")
    torch.cuda.set_device(0)
    res = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "steps": args.steps, "warm": args.warm}
    if "selection" in parts:
        selection_part(args, res)
    if "decode" in parts:
        decode_part(args, res)
    if "prefill" in parts and args.model_layers > 0:
        w = wall(prefill_legs(args.model_layers, 4096, 2048), args.prefill_reps)
        res["prefill"] = {"shape": f"Llama2-7B-shaped random-init HF model, {args.model_layers} layers, 4096-token prompt, budget 2048, encoding mode, h2o_head, "
                                   "one-shot (obs_window 32, score_pool 7), max_new_tokens 1; wall seconds per generate call", **w}
        res["prefill"]["adaptive_over_uniform"] = round(w["one_shot_adaptive"]["seconds"] / w["one_shot_uniform"]["seconds"], 4)
    if args.out is not None:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


def selection_part(args, res):
    lo, hi = bounds()
    made = {"pooled_max_7": selection_leg(None), "adaptive_floor_0.2_ceil_2.0": selection_leg((lo, hi)), "adaptive_degenerate": selection_leg((N_EVICT, N_EVICT))}
    t = _interleave({k: f for k, (f, _, _) in made.items()}, args.reps, args.steps, args.warm)
    res["selection"] = {"shape": f"{L} layers x {H} heads, head_dim {D}, {OBS} queries over T = {T}, h2o_head, n_evict = {N_EVICT}, sink {SINK}, kernel size 7; "
                                 f"bounds ({lo}, {hi}); a leg is state_init + attention + its ending",
                        **{k: dict(us_per_step=t[k]["us"], run_to_run_spread=t[k]["spread"], plan=made[k][2]) for k in made}}
    for k in list(made)[1:]:
        res["selection"][k]["us_over_pooled"] = round(t[k]["us"] - t["pooled_max_7"]["us"], 2)
    bank = made["adaptive_floor_0.2_ceil_2.0"][1]
    res["selection"]["adaptive_floor_0.2_ceil_2.0"]["rows_per_head_layer0"] = list(bank.head_slots[0])
    try:
        res["kernels"] = kernel_split({k: f for k, (f, _, _) in list(made.items())[:2]})
    except Exception as e:      # (the timings above do not depend on the profiler)
        res["kernels"] = {"unavailable": repr(e)[:200]}
    made.clear()
    torch.cuda.empty_cache()


def decode_part(args, res):
    legs, lens, ragged = decode_legs()
    t = _interleave(legs, args.reps, args.steps, args.warm)
    res["decode"] = {"shape": f"{L} layers x {H} heads, head_dim {D}, h2o_head evicting decode step; ragged: heads alternate {lens[0]} / {lens[1]} rows, "
                              "one batched call on the one-head view per layer, or one deferred call of the heads family per layer + one flush; "
                              "uniform: 2048 rows per head, one deferred call per layer + one flush",
                     **{k: dict(us_per_token_step=t[k]["us"], run_to_run_spread=t[k]["spread"]) for k in legs}}
    view, uni, heads = (t[k]["us"] for k in ("ragged_view_per_layer", "uniform_deferred_per_layer", "ragged_heads_deferred_per_layer"))
    res["decode"]["ragged_over_uniform"] = round(view / uni, 4)
    res["decode"]["deferred_over_view"] = round(heads / view, 4)
    res["decode"]["deferred_over_uniform"] = round(heads / uni, 4)
    # an improvement only when the deferred median is below the view's by more than both legs' spreads
    margin = view * t["ragged_view_per_layer"]["spread"] + heads * t["ragged_heads_deferred_per_layer"]["spread"]
    res["decode"]["deferred_faster_than_view_beyond_both_spreads"] = bool(view - heads > margin)
    res["decode"]["head_table_uploads"] = ragged.head_table_uploads
    os.makedirs(os.path.dirname(os.path.abspath(args.heads_out)), exist_ok=True)
    with open(args.heads_out, "w") as f:
        json.dump({k: res[k] for k in ("device", "reps", "steps", "warm", "decode")}, f, indent=1)
    legs.clear()
    del ragged
    torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
