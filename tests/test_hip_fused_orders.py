"""The two phase orders of the one-launch decode step (ekv_attn_decode.inc: order F streams K+V and then runs the scorer tail, order
K streams K, runs the tail, streams V and replays the online softmax from the logits in LDS) compute the same bits.

The same seeded run — bench head geometry (D = 128, 32 heads, T = 2049, cap 2112), a scattered slot map with NaN / inf bit patterns in
the free K/V rows, 18 layers (576 heads per launch, so the planner picks the mixed mode by itself), 72 evicting steps — is executed
with EKV_FUSED_ORDER = 0 (all F), 1 (mixed per CU, by a hardware-derived number) and 2 (all K), one child process each because the
library reads the knob once.  Attention outputs of every step, evicted ids, the raw slot-indexed S / Q / C0 / birth rows, the slot map
and the per-head state must be bit-equal across the three; equality is by construction (same floating-point operations in the same
order), so there is no tolerance and no excluded case.

Mode 0 is also held to the oracle on the first two layers with the bars of the existing parity tests: fp16 as
tests/test_hip_fullsize.py (outputs within 1e-3, every decision the +-2e-5 probe calls well defined equal to the oracle's, >= 95 % of
the decisions well defined; a head leaves the comparison after its first ill-defined decision), bf16 outputs with the bar of
tests/test_hip_bf16.py (|o - ref| <= 2^-8 (|ref| + pv) + 1e-6 pv)."""
import os
import subprocess
import sys

import pytest
import torch

from tests import fused_orders_run as R
from tests.golden_util import out_close

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("outs", "ids", "S", "Q", "C0", "birth", "slot_of_pos", "slot_state")


def _child(mode, policy, dtype, path):
    env = dict(os.environ, EKV_FUSED_ORDER=str(mode))
    env.pop("EKV_FUSED_ORDER_RULE", None)
    r = subprocess.run([sys.executable, "-m", "tests.fused_orders_run", policy, dtype, str(path)], cwd=ROOT, env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, (mode, r.returncode, r.stderr[-2000:])
    return torch.load(str(path))


def _oracle_bars(res, policy, dtype):
    from oracle import easykv_oracle as O
    from tests.test_hip_bf16 import _check_out, _pv
    from tests.test_hip_fullsize import Probe
    tdt = {"fp16": torch.float16, "bf16": torch.bfloat16}[dtype]
    k0, v0, warm, qs, ks, vs = R.inputs(tdt)
    H, T, n_check = R.H, R.BUDGET + 1, 2
    outs = res["outs"].view(tdt)
    states = []
    for l in range(n_check):
        st = O.LayerState(k=k0[l:l + 1].float(), v=v0[l:l + 1].float())
        st.s, st.q, st.c = O.init_state_decoding((H,), R.BUDGET)
        st.s += warm[l]
        st.q += warm[l] ** 2
        states.append(st)
    oplan = O.StepPlan(policy=policy, phase="decode", evict=True, score_off=0, budget=R.BUDGET)
    alive = torch.ones(n_check, H, dtype=torch.bool)
    n_dec = n_stable = 0
    probe = Probe()
    O.SELECT_HOOK = probe
    try:
        for i in range(R.STEPS):
            for l in range(n_check):
                st = states[l]
                q, k, v = qs[i, l:l + 1].float(), ks[i, l:l + 1].float(), vs[i, l:l + 1].float()
                if dtype == "bf16":
                    k_all, v_all = torch.cat([st.k[0], k[0]], 1), torch.cat([st.v[0], v[0]], 1)
                    pv = _pv(q[0], k_all, v_all, k_all.shape[1] - 1)
                o_ref, ids_ref = O.layer_step(st, q, k, v, oplan)
                unstable = probe.last_unstable
                got = res["ids"][i, l, :, 0].long()
                same = got == ids_ref[:, 0]
                n_dec += int(alive[l].sum())
                n_stable += int((alive[l] & ~unstable).sum())
                assert bool(same[alive[l] & ~unstable].all()), (policy, dtype, i, l)
                m = alive[l]                      # (heads still on the oracle's trajectory BEFORE this decision: their outputs count)
                if dtype == "bf16":
                    _check_out(outs[i, l][m], o_ref[0][m], pv[m], (policy, i, l))
                else:
                    assert out_close(outs[i, l][m].float(), o_ref[0][m]), (policy, i, l)
                alive[l] &= ~unstable & same
    finally:
        O.SELECT_HOOK = None
    print(f"[fused-orders] {policy} {dtype}: {n_stable} of {n_dec} decisions well defined, {int(alive.sum())} of {alive.numel()} heads compared to the end")
    assert n_stable >= 0.95 * n_dec, (n_stable, n_dec)


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("policy", ["roco", "h2o_head", "tova"])
def test_phase_orders_compute_the_same_bits(policy, dtype, tmp_path):
    runs = {mode: _child(mode, policy, dtype, tmp_path / f"m{mode}.pt") for mode in (0, 1, 2)}
    for mode, r in runs.items():
        # the steps ran as ONE launch on the slot-indexed layout, in the order mode asked for (else F would be compared with itself)
        assert r["n_slot"] == R.STEPS, (mode, r["n_slot"])
        assert r["info"]["fused"] == 1 and r["info"]["fused_order"] == mode, (mode, r["info"])
        assert r["n_slots"] == [R.BUDGET] * R.L
    for mode in (1, 2):
        for key in KEYS:
            assert torch.equal(runs[0][key], runs[mode][key]), (mode, key, int((runs[0][key] != runs[mode][key]).sum()))
        assert (runs[0]["k_sum"], runs[0]["v_sum"]) == (runs[mode]["k_sum"], runs[mode]["v_sum"]), mode
    _oracle_bars(runs[0], policy, dtype)
