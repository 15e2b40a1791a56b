"""One launch of the 8-wave one-launch decode instance that really runs in two dispatch rounds: 17 layers x 32 heads = 544 workgroups
of eight waves (at most 512 are resident on 256 CUs), budget 64, three evicting steps, with EKV_FUSED_NW = 8.

Four runs, one child process each: all F (EKV_FUSED_ORDER = 0), all K (2), the mixed mode under the planner's own rule word (1: rule
source 3 with the default threshold, 0 — every workgroup decides by the rule and takes order K), and the mixed mode under
EKV_FUSED_ORDER_RULE = 3,4,0,1 (threshold 512: the first round, workgroups 0 .. 511, runs order F and the second, 512 .. 543 — layer 16 —
order K, so both orders meet in one launch that has a second round).  Outputs, evicted ids, score rows, slot map and head state must
be bit-equal to the all-F run, as in tests/test_hip_rounds_orders.py."""
import pytest

from tests.test_hip_rounds_orders import children, same_bits

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("policy", ["roco", "h2o_head", "tova"])
def test_second_round_runs_order_k_with_the_same_bits(policy, tmp_path):
    runs = children("launch", policy, "fp16", tmp_path, modes={0: None, 1: None, 2: None, "1_second_round": "3,4,0,1"})
    for key, run in runs.items():
        r = run["launch"]
        assert r["n_slot"] == 3 and r["info"]["fused"] == 1 and r["info"]["fused_order"] == int(str(key)[0]), (key, r["n_slot"], r["info"])
        assert r["n_slots"] == [64] * 17 and len(r["ids"]) == 3
    same_bits(runs)
