"""Resident rows of the one-launch decode step (include/easykv_hip.h, "resident rows"): does a share of the K/V rows read with
default-policy loads stay in the 256 MiB Infinity Cache from one decode step to the next, behind ~0.9 GB of non-temporal stream?

    python tools/experiments/exp_resident.py sweep    [--out profiles/resident_sweep.json] [--values 0,64,...] [--rounds 4]
    python tools/experiments/exp_resident.py harm     [--out profiles/resident_harm.json] [--mb 224] [--fill-mb 320] [--rounds 3]
    python tools/experiments/exp_resident.py headline --parent-tree DIR [--out profiles/resident_headline_bench.json] [--runs 4]
    python tools/experiments/exp_resident.py child    (what the first two start: one process per knob value, the library reads it once)

sweep: the bench shape (KVBank, 32 layers x 32 heads x 2049 rows of 128, roco, scattered slot map, 4096 pre-warm steps as bench.py), one
child process per value of EKV_RESIDENT_MB, the values interleaved in every round; us per step (one HIP event pair around blocks of
back-to-back launches), median and spread per value.
harm: the same loop with a torch fill of --fill-mb between two steps (what a model's weights do to the cache), only the step's launch
between the events, resident rows on and off.
headline: `python bench.py` of this tree and of a built checkout of the parent commit in turn, then `--dump-outputs` of both at 16 steps
and at the default length: attn_out and evict_ids must be equal arrays.
Every child runs under a timeout; the first one that fails or times out ends the experiment (nothing more is started on the GPU)."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
L, H, D, BUDGET = 32, 32, 128, 2048
CHILD_TIMEOUT = 240


def child(a):
    import torch
    from easykv_amd import KVBank, StepPlan
    dev = torch.device("cuda")
    T = BUDGET + 1
    gen = torch.Generator(device=dev).manual_seed(1234)
    bank = KVBank(L, H, H, D, cap=T + 63, device=dev)
    for l0 in range(0, L, 8):
        bank.load_rows(torch.randn(8, H, BUDGET, D, generator=gen, device=dev).half(), torch.randn(8, H, BUDGET, D, generator=gen, device=dev).half(),
                       pos_begin=0, layer_begin=l0)
    bank.slot_of_pos[:, :, :BUDGET] = torch.argsort(torch.rand(L, H, BUDGET, generator=gen, device=dev), dim=-1).int()
    bank.state_init(T, 0)
    n_in = 64
    qs, ks, vs = (torch.randn(n_in, L, H, 1, D, generator=gen, device=dev).half() for _ in range(3))
    out = torch.empty(L, H, 1, D, dtype=torch.float16, device=dev)
    ids = torch.full((L, H, 1), -1, dtype=torch.int32, device=dev)
    plan = StepPlan(policy="roco", phase="decode", evict=True, score_off=0, budget=BUDGET)
    fill = torch.empty(a.fill_mb << 20, dtype=torch.uint8, device=dev) if a.fill_mb else None

    def step(i):
        bank.attend(plan, qs[i % n_in], ks[i % n_in], vs[i % n_in], out=out, evict_ids=ids)

    for i in range(a.prewarm):
        step(i)
        if i % 16 == 15:
            torch.cuda.synchronize()
    torch.cuda.synchronize()
    rows = bank.resident_rows(plan, phases=16 if all(bank._slot_rows) else 0)
    blocks = []
    for b in range(a.blocks):
        if fill is None:
            e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            e[0].record()
            for i in range(a.steps):
                step(i)
            e[1].record()
            torch.cuda.synchronize()
            blocks.append(e[0].elapsed_time(e[1]) / a.steps * 1e3)
        else:
            ev = [[torch.cuda.Event(enable_timing=True) for _ in range(2)] for _ in range(a.steps)]
            for i in range(a.steps):
                fill.fill_(i & 127)
                ev[i][0].record()
                step(i)
                ev[i][1].record()
            torch.cuda.synchronize()
            blocks.append(statistics.median(x.elapsed_time(y) for x, y in ev) * 1e3)
    print(json.dumps(dict(us_per_step=statistics.median(blocks), blocks=[round(x, 3) for x in blocks], resident_rows=rows,
                          slot_rows=bool(all(bank._slot_rows)))))


def run_child(mb, extra, env_extra=None):
    env = dict(os.environ, EKV_RESIDENT_MB=str(mb))
    env.pop("EKV_RESIDENT_ROWS", None)
    env.update(env_extra or {})
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "child"] + extra, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=CHILD_TIMEOUT)
    if r.returncode != 0:
        raise RuntimeError(f"child EKV_RESIDENT_MB={mb} ended with status {r.returncode}: {r.stderr[-1500:]}")
    return json.loads(r.stdout.splitlines()[-1])


def summary(samples):
    return {str(k): dict(us=[round(x, 2) for x in v], median=round(statistics.median(v), 2), min=round(min(v), 2), max=round(max(v), 2),
                         spread_pct=round((max(v) - min(v)) / statistics.median(v) * 100, 2)) for k, v in samples.items()}


def write(path, doc):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc), flush=True)


def sweep(a):
    values = [int(x) for x in a.values.split(",")]
    samples, rows, err = {v: [] for v in values}, {}, None
    try:
        for rnd in range(a.rounds):
            for v in (values if rnd % 2 == 0 else values[::-1]):
                got = run_child(v, ["--steps", str(a.steps), "--blocks", str(a.blocks)])
                samples[v].append(got["us_per_step"])
                rows[str(v)] = got["resident_rows"]
                print(f"[sweep] round {rnd} EKV_RESIDENT_MB={v}: {got}", flush=True)
    except (RuntimeError, subprocess.TimeoutExpired) as e:
        err = str(e)[-2000:]
    doc = dict(what="us per one-launch decode step, bench shape (32 layers x 32 heads x 2049 rows x 128, roco, scattered slot map, 4096 pre-warm steps), "
                    "one child process per value of EKV_RESIDENT_MB (MiB), values interleaved per round; per child the median of its blocks of "
                    f"{a.steps} back-to-back launches under one HIP event pair",
               rounds=a.rounds, resident_rows=rows, values=summary({k: v for k, v in samples.items() if v}), error=err)
    write(a.out, doc)
    return 1 if err else 0


def harm(a):
    samples, rows, err = {}, {}, None
    extra = ["--steps", str(a.steps), "--blocks", "3", "--fill-mb", str(a.fill_mb)]
    try:
        for rnd in range(a.rounds):
            for v in ((0, a.mb) if rnd % 2 == 0 else (a.mb, 0)):
                got = run_child(v, extra)
                samples.setdefault(v, []).append(got["us_per_step"])
                rows[str(v)] = got["resident_rows"]
                print(f"[harm] round {rnd} EKV_RESIDENT_MB={v}: {got}", flush=True)
    except (RuntimeError, subprocess.TimeoutExpired) as e:
        err = str(e)[-2000:]
    doc = dict(what=f"us per decode step (median over steps, HIP events around the step's launch alone) with a torch fill of {a.fill_mb} MiB between "
                    "two steps: resident rows off (0) and on",
               rounds=a.rounds, fill_mb=a.fill_mb, resident_rows=rows, values=summary(samples), error=err)
    write(a.out, doc)
    return 1 if err else 0


def bench_once(tree, extra=(), env_extra=None):
    env = {k: v for k, v in os.environ.items() if k not in ("EKV_RESIDENT_MB", "EKV_RESIDENT_ROWS", "EASYKV_HIP_LIB")}
    env.update(env_extra or {})
    r = subprocess.run([sys.executable, os.path.join(tree, "bench.py"), "--gpus", "1", *extra], cwd=tree, env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=CHILD_TIMEOUT)
    if r.returncode != 0:
        raise RuntimeError(f"bench.py of {tree} ended with status {r.returncode}: {r.stderr[-1500:]}")
    line = json.loads(r.stdout.splitlines()[-1])
    return dict(tokens_per_s=round(line["value"], 1), avg_launch_us=round(line["roofline"]["avg_launch_us"], 2))


def headline(a):
    import numpy as np
    trees = dict(parent=os.path.abspath(a.parent_tree), new=ROOT)
    a.dump_dir = os.path.abspath(a.dump_dir or tempfile.mkdtemp(prefix="resident_dumps_"))      # (each bench.py runs in its own tree)
    # third leg: this tree with the budget at 0 — the resident instances' code with every load non-temporal, against the parent's code
    legs = dict(parent=(trees["parent"], None), new=(ROOT, None), new_budget0=(ROOT, {"EKV_RESIDENT_MB": "0"}))
    runs, equal, err = {k: [] for k in legs}, {}, None
    try:
        for i in range(a.runs):
            for name in (list(legs) if i % 2 == 0 else list(legs)[::-1]):
                runs[name].append(bench_once(legs[name][0], env_extra=legs[name][1]))
                print(f"[headline] run {i} {name}: {runs[name][-1]}", flush=True)
        for label, extra in (("steps16", ["--steps", "16"]), ("default", [])):
            dirs = {}
            for name, tree in trees.items():
                dirs[name] = os.path.join(a.dump_dir, f"{label}_{name}")
                bench_once(tree, [*extra, "--dump-outputs", dirs[name]])
            equal[label] = {n: bool(np.array_equal(np.load(os.path.join(dirs["parent"], n + ".npy")), np.load(os.path.join(dirs["new"], n + ".npy"))))
                            for n in ("attn_out", "evict_ids")}
            print(f"[headline] outputs {label}: {equal[label]}", flush=True)
    except (RuntimeError, subprocess.TimeoutExpired) as e:
        err = str(e)[-2000:]
    doc = dict(what="python bench.py --gpus 1 (2048 steps, 8 warmup, 4096 pre-warm) of the parent commit's build, of this tree and of this tree under "
                    "EKV_RESIDENT_MB=0, in turn, one session",
               runs=runs, error=err, outputs_equal=equal)
    if all(len(v) >= 2 for v in runs.values()):
        us = {k: [r["avg_launch_us"] for r in v] for k, v in runs.items()}
        spread = (max(us["parent"]) - min(us["parent"])) / statistics.median(us["parent"]) * 100
        gain = (statistics.median(us["parent"]) - statistics.median(us["new"])) / statistics.median(us["parent"]) * 100
        doc["summary"] = dict(parent_us=[min(us["parent"]), statistics.median(us["parent"]), max(us["parent"])],
                              new_us=[min(us["new"]), statistics.median(us["new"]), max(us["new"])], parent_spread_pct=round(spread, 2),
                              median_gain_pct=round(gain, 2), new_slowest_beats_parent_fastest=max(us["new"]) < min(us["parent"]),
                              gain_exceeds_twice_the_spread=gain > 2 * spread,
                              new_budget0_us=[min(us["new_budget0"]), statistics.median(us["new_budget0"]), max(us["new_budget0"])],
                              budget0_over_parent_pct=round((statistics.median(us["new_budget0"]) / statistics.median(us["parent"]) - 1) * 100, 2))
    write(a.out, doc)
    return 1 if err else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("sweep", "harm", "headline", "child"))
    ap.add_argument("--out", default=None)
    ap.add_argument("--values", default="0,64,128,160,192,224,256")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--steps", type=int, default=1024)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--prewarm", type=int, default=4096)
    ap.add_argument("--fill-mb", type=int, default=0)
    ap.add_argument("--mb", type=int, default=224)
    ap.add_argument("--runs", type=int, default=4)
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--dump-dir", default=None, help="headline: where the --dump-outputs arrays go (default: a temporary directory)")
    a = ap.parse_args()
    if a.mode == "child":
        return child(a) or 0
    a.out = a.out or os.path.join(ROOT, "profiles", {"sweep": "resident_sweep.json", "harm": "resident_harm.json", "headline": "resident_headline_bench.json"}[a.mode])
    if a.mode == "harm":
        a.fill_mb = a.fill_mb or 320
        a.steps = min(a.steps, 256)
        return harm(a)
    if a.mode == "headline":
        if not a.parent_tree:
            ap.error("headline needs --parent-tree: a built checkout of the parent commit")
        return headline(a)
    return sweep(a)


if __name__ == "__main__":
    sys.exit(main())
