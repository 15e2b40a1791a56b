"""The 8-wave one-launch decode instance (ekv_decode_fused_kernel<128, 1, false, 5 | 12, 8, true>) computes the same bits in both
phase orders and under the rule by dispatch round (ekv_attn_decode.inc, rule source 3).

The instance is forced with EKV_FUSED_NW = 8 on 8 KV heads x 2 layers (16 workgroups), head_dim 128.  The same seeded runs — 24
evicting steps on a scattered slot map whose free rows, inside and behind the extent, hold NaN / inf bit patterns — are executed
with EKV_FUSED_ORDER = 0 (all F), 2 (all K) and 1 under EKV_FUSED_ORDER_RULE = 3,0,1,1 (order K from workgroup 8 on: both orders in one
launch), one child process each because the library reads the knobs once.  Per (policy, element type) a child runs every physical
extent around the 8-wave geometry (a workgroup iteration is 256 rows; 1 .. 2304 rows on the 5-column build, 2305 and 2560 on the
12-column one) with 0, 32 and all rows resident.  Extent 1 is the empty bank, where nothing can be evicted: its 24 steps grow the bank
row by row instead (extents 1 .. 24).

Attention outputs of every step, evicted ids, the raw slot-indexed S / Q / C0 / birth rows, the slot map, the per-head state and the
checksums of the K / V planes must be bit-equal across the three modes: equality is by construction (same floating-point operations
in the same order), so there is no tolerance and no excluded case."""
import os
import subprocess
import sys

import pytest
import torch

from tests import rounds_orders_run as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("outs", "ids", "S", "Q", "C0", "birth", "slot_of_pos", "slot_state")
MODES = {0: None, 2: None, 1: "3,0,1,1"}      # EKV_FUSED_ORDER -> EKV_FUSED_ORDER_RULE


def children(what, policy, dtype, tmp_path, modes=MODES, nw="8"):
    """{key: results} of one child per entry of `modes` (key -> rule, the mode being the key's first character), run side by side."""
    procs = {}
    for key, rule in modes.items():
        mode = int(str(key)[0])
        env = {k: v for k, v in os.environ.items() if not k.startswith("EKV_FUSED")}
        env.update(EKV_FUSED_ORDER=str(mode))
        if nw:
            env["EKV_FUSED_NW"] = nw
        if rule:
            env["EKV_FUSED_ORDER_RULE"] = rule
        path = tmp_path / f"{what}_m{key}.pt"
        procs[key] = (path, subprocess.Popen([sys.executable, "-m", "tests.rounds_orders_run", what, policy, dtype, str(path)], cwd=ROOT, env=env,
                                              stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
    runs = {}
    try:
        for mode, (path, p) in procs.items():
            _, err = p.communicate(timeout=300)
            assert p.returncode == 0, (mode, p.returncode, err[-2000:])
            runs[mode] = torch.load(str(path))
    finally:      # (a child that failed or ran too long takes its siblings with it: nothing stays on the GPU)
        for _, p in procs.values():
            if p.poll() is None:
                p.kill()
                p.communicate()
    return runs


def same_bits(runs, base=0):
    for mode, run in runs.items():
        if mode == base:
            continue
        assert run.keys() == runs[base].keys()
        for name, r in run.items():
            b = runs[base][name]
            for key in KEYS:
                assert torch.equal(b[key], r[key]), (mode, name, key, int((b[key] != r[key]).sum()))
            assert (b["k_sum"], b["v_sum"]) == (r["k_sum"], r["v_sum"]), (mode, name)


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("policy", ["roco", "h2o_head", "tova"])
def test_eight_wave_orders_compute_the_same_bits(policy, dtype, tmp_path):
    runs = children("orders", policy, dtype, tmp_path)
    for mode, run in runs.items():
        assert len(run) == len(R.EXTENTS) * len(R.RESIDENT)
        for extent in R.EXTENTS:
            for resident in R.RESIDENT:
                r = run[f"e{extent}_{resident}"]
                # every step ran as ONE launch on the slot-indexed layout, in the order mode asked for (else F would be compared with
                # itself), with the resident rows the case is about
                assert r["n_slot"] == R.STEPS, (mode, extent, resident, r["n_slot"])
                assert r["info"]["fused"] == 1 and r["info"]["fused_order"] == mode, (mode, extent, resident, r["info"])
                ext32 = (max(extent, R.geometry(extent)[0]) + 31) // 32 * 32
                assert r["resident_rows"] == {"none": 0, "one_unit": 32, "all": ext32}[resident], (extent, resident, r["resident_rows"])
                t = R.geometry(extent)[0]
                assert r["n_slots"] == [R.STEPS if extent == 1 else t - 1] * 2
                assert len(r["ids"]) == (0 if extent == 1 else R.STEPS)
    same_bits(runs)
