"""Window decode steps against their twins, in one process, the legs interleaved (window rep, twin rep, ...) on banks filled with copies of
the same rows; writes profiles/window_bench.json and prints it as one JSON line.

Two pairs, budget 2048 (T = 2049), roco, scattered slot map, warm score state, heads unsplit (n_split = 1), windows alternating 128 / 0
over the layers (gpt-oss's layer_types):
  * gpt-oss's shape — head_dim 64, 64 query heads over 8 KV heads, 24 layers: the window + sink step against the sink step;
  * head_dim 128, 32 heads x 32 layers: the window-alone step against the plain step forced to phase order F (EKV_FUSED_ORDER=0, set
    here before the library loads) without resident rows — what the window instances are built as.
A window step plans as its twin (`plan` records both legs' info).  What it adds per iteration of a lane group: one 4-byte load of a
token position per lane, one compare and one ballot; a masked row is still streamed.  The yardstick is the twin leg of the same run;
there is no pass bar — the ratio is recorded as it comes out, next to each leg's run-to-run spread.

Per leg: µs per launch (median of per-rep means, HIP events on the launch stream) and the run-to-run spread.

Usage: python tools/bench_window.py [--reps 11] [--steps 20] [--warm 200] [--out profiles/window_bench.json]"""
from __future__ import annotations

import argparse
import gc
import json
import os
import sys

os.environ.setdefault("EKV_FUSED_ORDER", "0")      # (read once by the planner: the plain twin runs order F, as every other leg does by build)

import torch  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.bench_kv8 import _interleave  # noqa: E402

BUDGET = 2048
WINDOW = 128


def fused_step(L, Hq, H, D, with_sinks, with_windows):
    from easykv_amd import KVBank, StepPlan
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(1234)      # (the same rows in both legs of a pair)
    kw = {}
    if with_sinks:
        kw["sinks"] = torch.randn(L, Hq, generator=torch.Generator().manual_seed(11)) + 1
    if with_windows:
        kw["windows"] = [WINDOW if l % 2 == 0 else 0 for l in range(L)]
    bank = KVBank(L, Hq, H, D, cap=BUDGET + 1 + 63, device=dev, **kw)
    bank.resident_bytes = 0
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "window_bench.json"))
    args = ap.parse_args()
    torch.cuda.set_device(0)
    res = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "steps": args.steps, "warm": args.warm,
           "windows": f"{WINDOW} on even layers, 0 on odd ones", "EKV_FUSED_ORDER": os.environ["EKV_FUSED_ORDER"],
           "shape": f"budget {BUDGET} (T = {BUDGET + 1}), roco, scattered slot map, warm score state, n_split = 1, no resident rows"}
    res["fused_decode"] = {}
    for name, (L, Hq, H, D), sinks in (("d64_64over8_x24_sink_window_vs_sink", (24, 64, 8, 64), True), ("d128_32x32_window_vs_plain_order_f", (32, 32, 32, 128), False)):
        made = {"window": fused_step(L, Hq, H, D, sinks, True), "twin": fused_step(L, Hq, H, D, sinks, False)}
        t = _interleave({k: f for k, (f, _, _) in made.items()}, args.reps, args.steps, args.warm)
        row = {k: dict(us_per_launch=t[k]["us"], run_to_run_spread=t[k]["spread"], slot_indexed_rows=bool(all(made[k][1]._slot_rows)), plan=made[k][2])
               for k in made}
        row["time_ratio_window_over_twin"] = round(t["window"]["us"] / t["twin"]["us"], 4)
        res["fused_decode"][name] = row
        made.clear()
        gc.collect()
        torch.cuda.empty_cache()
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
