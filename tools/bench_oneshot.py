"""One-shot prompt compression against the strided prefill, and the pooled scorer against the unpooled generic scorer, in one process with
the legs interleaved; writes profiles/oneshot_bench.json (or --out) and prints it as one JSON line.

(1) The scorer (`scorer`).  One observation step of the Llama2-7B shape — 32 layers x 32 heads, head_dim 128, 32 queries over T = 4096 keys
    (W = 4096 score columns), h2o_head, n_evict = 2048, sink 4 — through three calls of the same step: the pooled call with max and with
    avg (kernel size 7), and the plain call asked for "attention, then the generic scorer" (phases = 1 | 2), which is launch for launch the
    pooled plan with the unpooled scorer.  Every repetition restores the bank's length and re-initialises the score rows (in every leg
    alike), so a leg is state_init + attention + scorer; the legs differ in the scorer alone.  µs per step: median of per-rep means (HIP
    events), with the run-to-run spread.
(2) The prefill (`prefill`, --model-layers > 0).  A Llama2-7B-shaped, randomly initialised HF model through the seam; a 4096-token prompt
    cut to 2048 in encoding mode with h2o_head, max_new_tokens = 1 (one decode forward in every leg): generation_config['prefill'] =
    'one_shot' (obs_window 32, score_pool 7) against the strided prefill at stride 8 and stride 64 with generation_config['hipgraph'].
    Wall seconds per generate call, host-synchronised, legs interleaved, median and spread over --prefill-reps calls after one warm call
    per leg.

Usage: python tools/bench_oneshot.py [--reps 7] [--steps 5] [--warm 3] [--model-layers 32] [--prefill-reps 3] [--out profiles/oneshot_bench.json]"""
from __future__ import annotations

import argparse
import contextlib
import gc
import io
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.bench_kv8 import _interleave  # noqa: E402

L, H, D, T, OBS, SINK, N_EVICT = 32, 32, 128, 4096, 32, 4, 2048


def scorer_leg(pool, op, phases):
    from easykv_amd import KVBank, StepPlan
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(1234)      # (the same rows in every leg)
    bank = KVBank(L, H, H, D, cap=T + 8, device=dev)
    for l0 in range(0, L, 4):
        bank.load_rows(torch.randn(4, H, T - OBS, D, generator=g, device=dev).half(), torch.randn(4, H, T - OBS, D, generator=g, device=dev).half(),
                       pos_begin=0, layer_begin=l0)
    q = torch.randn(L, H, OBS, D, generator=g, device=dev).half()
    k, v = (torch.randn(L, H, OBS, D, generator=g, device=dev).half() for _ in range(2))
    out = torch.empty(L, H, OBS, D, dtype=torch.float16, device=dev)
    ids = torch.empty(L, H, N_EVICT, dtype=torch.int32, device=dev)
    plan = StepPlan(policy="h2o_head", phase="prefill", accumulate=True, evict=True, budget=T, recent=OBS, sink=SINK, stride=OBS, n_evict=N_EVICT,
                    pool=pool, pool_op=op)
    info = bank.step_info(plan, OBS, 0, L, phases)

    def step(i):
        bank.n_slots[:] = [T - OBS] * L      # (the rows of the last repetition's victims are free rows again: any permutation serves)
        bank.state_init(T, 2, OBS)
        bank.attend(plan, q, k, v, out=out, evict_ids=ids, phases=phases)
    return step, bank, info


def prefill_legs(layers, prompt, budget):
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
    base = dict(budget=budget, kv_policy="h2o_head", max_new_tokens=1, eos_token_ids=[-1], temperature=1e-6)

    def leg(stride, extra):
        def run(_):
            easykv_amd.enable_fixed_kv(model, Tok(), mode="encoding", stride=stride)
            with contextlib.redirect_stdout(io.StringIO()):
                model.easykv_generate(input_ids=ids, generation_config=dict(base, **extra))
        return run
    return {"one_shot_obs32_pool7": leg(8, dict(prefill="one_shot", obs_window=32, score_pool=7)),
            "strided_8_hipgraph": leg(8, dict(hipgraph=True)), "strided_64_hipgraph": leg(64, dict(hipgraph=True))}


def wall(fns, reps):
    for f in fns.values():
        f(0)
    torch.cuda.synchronize()
    got = {k: [] for k in fns}
    for _ in range(reps):
        for k, f in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f(0)
            torch.cuda.synchronize()
            got[k].append(time.perf_counter() - t0)
    return {k: dict(seconds=round(statistics.median(v), 4), spread=round((max(v) - min(v)) / statistics.median(v), 4), runs=[round(x, 4) for x in v])
            for k, v in got.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--model-layers", type=int, default=32)
    ap.add_argument("--prefill-reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "oneshot_bench.json"))
    args = ap.parse_args()
    torch.cuda.set_device(0)
    res = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "steps": args.steps, "warm": args.warm}
    made = {"pooled_max_7": scorer_leg(7, "max", 0), "pooled_avg_7": scorer_leg(7, "avg", 0), "unpooled_generic": scorer_leg(1, "max", 3)}
    t = _interleave({k: f for k, (f, _, _) in made.items()}, args.reps, args.steps, args.warm)
    res["scorer"] = {"shape": f"{L} layers x {H} heads, head_dim {D}, {OBS} queries over T = {T}, h2o_head, n_evict = {N_EVICT}, sink {SINK}; a leg is "
                              "state_init + attention + scorer",
                     **{k: dict(us_per_step=t[k]["us"], run_to_run_spread=t[k]["spread"], plan=made[k][2]) for k in made}}
    for k in ("pooled_max_7", "pooled_avg_7"):
        res["scorer"][k]["us_over_unpooled"] = round(t[k]["us"] - t["unpooled_generic"]["us"], 2)
        res["scorer"][k]["time_ratio_over_unpooled"] = round(t[k]["us"] / t["unpooled_generic"]["us"], 4)
    made.clear()
    gc.collect()
    torch.cuda.empty_cache()
    if args.model_layers > 0:
        w = wall(prefill_legs(args.model_layers, 4096, 2048), args.prefill_reps)
        res["prefill"] = {"shape": f"Llama2-7B-shaped random-init HF model, {args.model_layers} layers, 4096-token prompt, budget 2048, encoding mode, h2o_head, "
                                   "max_new_tokens 1; wall seconds per generate call", **w}
        res["prefill"]["one_shot_over_strided_64"] = round(w["one_shot_obs32_pool7"]["seconds"] / w["strided_64_hipgraph"]["seconds"], 4)
        res["prefill"]["one_shot_over_strided_8"] = round(w["one_shot_obs32_pool7"]["seconds"] / w["strided_8_hipgraph"]["seconds"], 4)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
