"""Twin banks: the same 24 evicting decode steps of the benched state (Llama2-7B head shape, budget 2048, scattered slot map, roco,
slot-indexed score rows; 64 heads, one launch) on the 4-wave and on the 8-wave one-launch instance (EKV_FUSED_NW = 4 / 8, one child
process each: the library reads the knob once).  The 8-wave child runs every workgroup in order K (EKV_FUSED_ORDER = 2), the order the
planner ships on that instance; the 4-wave child of 64 heads runs order F.

The two instances sum their wave partials in different orders (four and eight partials, another column ownership in the tail), so
their outputs may differ in rounding; each child therefore holds its own run to the oracle with the bars of
tests/test_hip_lockstep.py — outputs within tests/golden_util.out_close, every decision equal to the oracle's or in its tolerance
class (one of the oracle's own answers under a +-2e-5 perturbation of its scores), at least 98 % equal, the final state as there.
Here: both children passed, both ran every step as one launch on the slot-indexed layout, and wherever the twins evict different
rows each of the two decisions was shown to be in the oracle's tolerance class by its own child — a tie by the existing rule."""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_four_and_eight_wave_instances_follow_the_oracle(tmp_path):
    procs = {}
    for nw in (4, 8):
        env = {k: v for k, v in os.environ.items() if not k.startswith("EKV_FUSED")}
        env["EKV_FUSED_NW"] = str(nw)
        if nw == 8:
            env["EKV_FUSED_ORDER"] = "2"      # (order K, what the planner ships on this instance; 64 heads plan order F otherwise)
        path = tmp_path / f"nw{nw}.pt"
        procs[nw] = (path, subprocess.Popen([sys.executable, "-m", "tests.twin_bank_run", str(path)], cwd=ROOT, env=env,
                                            stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
    runs = {}
    try:
        for nw, (path, p) in procs.items():
            _, err = p.communicate(timeout=300)
            assert p.returncode == 0, (nw, p.returncode, err[-3000:])      # (the child's own oracle bars)
            runs[nw] = torch.load(str(path))
    finally:      # (nothing stays on the GPU behind a child that failed or ran too long)
        for _, p in procs.values():
            if p.poll() is None:
                p.kill()
                p.communicate()
    for nw, r in runs.items():
        assert r["info"]["fused"] == 1 and r["n_dec"] == r["steps"] * 64 and r["n_exact"] + r["n_class"] == r["n_dec"], (nw, r["info"], r["n_dec"])
        print(f"[twin] {nw} waves: {r['n_exact']} exact + {r['n_class']} in the tolerance class of {r['n_dec']}; {r['n_slot_steps']}/{r['steps']} steps on the slot-indexed layout")
    a, b = runs[4], runs[8]
    differ = int((a["ids"] != b["ids"]).sum())
    out_bits = int((a["outs"].view(torch.int16) != b["outs"].view(torch.int16)).sum())
    print(f"[twin] decisions that differ between the twins: {differ} of {a['ids'].numel()}; output elements that differ: {out_bits} of {a['outs'].numel()}, "
          f"max |difference| {float((a['outs'].float() - b['outs'].float()).abs().max()):.3g}")
    # The first decision on which the twins differ is one on which at least one of them differed from the oracle: it was bound to the
    # tolerance class there, or that child would have failed (after it the twins hold different rows, and later decisions may differ
    # freely).  So twins that both equalled the oracle throughout made the same decisions.
    if a["n_class"] + b["n_class"] == 0:
        assert differ == 0, differ
