"""The resident rows of the one-launch decode step (include/easykv_hip.h, "resident rows") change the load policy of a K/V row and
nothing else: whatever share of the rows is read with default-policy loads, every bit the step produces is the same.

The same seeded run — 32 heads of head_dim 128, 17 layers (544 heads: the 4-wave flagship instance), budget 327 (T = 328, a bank of 448
rows per head whose extent is unknown, so 448 physical rows = three and a half 128-row workgroup blocks are streamed), a scattered slot
map with NaN / inf bit patterns in the free rows, 12 evicting steps — is executed with EKV_RESIDENT_ROWS = 0 (none resident), 32, 96
(boundaries inside the first block), 128 (a block edge), 160, 352 (inside the second and third block), 416 (inside the partial last
block), 448 (all rows) and a value past the extent, each under EKV_FUSED_ORDER 0 and 2 (both phase orders), with roco and h2o_head on
fp16 rows and roco on bf16 rows; one child process per setting, because the library reads the knobs once.  Outputs of every step,
evicted ids, the raw slot-indexed S / Q / C0 / birth rows, the slot map, the per-head state and the K/V checksums must be equal to the
run with no resident rows in order F: equality is by construction (the same arithmetic on the same bytes), so there is no tolerance.
The 8-wave build (9 layers = 288 heads) and the 24- / 12-column builds (budget 2400, 4 and 8 waves) get one setting each."""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("outs", "ids", "S", "Q", "C0", "birth", "slot_of_pos", "slot_state")
CASES = ("roco:fp16", "h2o_head:fp16", "roco:bf16")
L, BUDGET, STEPS = 17, 327, 12
ROWS = (32, 96, 128, 160, 352, 416, 448, 4096)
KNOBS = ("EKV_RESIDENT_ROWS", "EKV_RESIDENT_MB", "EKV_FUSED_ORDER", "EKV_FUSED_ORDER_RULE", "EKV_FUSED_NW")


def _child(rows, order, path, layers=L, budget=BUDGET, steps=STEPS, cases=CASES):
    env = {k: v for k, v in os.environ.items() if k not in KNOBS}
    env.update(EKV_RESIDENT_ROWS=str(rows), EKV_FUSED_ORDER=str(order))
    r = subprocess.run([sys.executable, "-m", "tests.resident_rows_run", str(layers), str(budget), str(steps), str(path), *cases], cwd=ROOT, env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0, (rows, order, r.returncode, r.stderr[-2000:])
    return torch.load(str(path))


def _same(ref, got, rows, order, steps=STEPS, layers=L, budget=BUDGET):
    for case, r in got.items():
        # the steps ran as ONE launch on the slot-indexed layout, in the order asked for, with the resident rows asked for
        assert r["n_slot"] == steps and r["info"]["fused"] == 1 and r["info"]["fused_order"] == order, (case, r["n_slot"], r["info"])
        assert r["rows"] == min(rows // 32 * 32, (r["cap"] + 31) // 32 * 32), (case, rows, r["rows"], r["cap"])
        assert r["n_slots"] == [budget] * layers
        for key in KEYS:
            assert torch.equal(ref[case][key], r[key]), (case, rows, order, key, int((ref[case][key] != r[key]).sum()))
        assert (ref[case]["k_sum"], ref[case]["v_sum"]) == (r["k_sum"], r["v_sum"]), (case, rows, order)


@pytest.fixture(scope="module")
def no_resident(tmp_path_factory):
    """The run with every K/V load non-temporal, order F: what every other setting must reproduce."""
    ref = _child(0, 0, tmp_path_factory.mktemp("resident") / "ref.pt")
    _same(ref, ref, 0, 0)
    assert ref["roco:fp16"]["cap"] == 448
    return ref


@pytest.mark.parametrize("order", [0, 2])
@pytest.mark.parametrize("rows", ROWS)
def test_resident_rows_compute_the_same_bits(no_resident, rows, order, tmp_path):
    _same(no_resident, _child(rows, order, tmp_path / "run.pt"), rows, order)


def test_no_resident_rows_in_order_k(no_resident, tmp_path):
    _same(no_resident, _child(0, 2, tmp_path / "run.pt"), 0, 2)


@pytest.mark.parametrize("layers,budget,rows", [(9, 327, 96), (17, 2400, 1120), (9, 2400, 2272)], ids=["8-wave", "24-column", "8-wave-12-column"])
def test_other_builds(layers, budget, rows, tmp_path):
    kw = dict(layers=layers, budget=budget, steps=4, cases=("roco:fp16",))
    ref = _child(0, 0, tmp_path / "ref.pt", **kw)
    got = _child(rows, 0, tmp_path / "run.pt", **kw)
    for r in (ref, got):
        assert r["roco:fp16"]["cap"] == (budget + 1 + 63 + 63) // 64 * 64
    _same(ref, ref, 0, 0, kw["steps"], layers, budget)
    _same(ref, got, rows, 0, kw["steps"], layers, budget)
