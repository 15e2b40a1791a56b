"""The free softmax scale on every kernel family: uncapped banks with sm_scale = 144 ** -0.5 at head_dim 128 (Gemma 2 27B's
query_pre_attn_scalar) against the oracle with a scaled `attention_core` (tests/softcap_ref.py), one small case per family.  Every
kernel reads ekv_step.sm_div; before, KVBank.make_step pinned it to sqrt(head_dim).  The runners are those of tests/test_hip_softcap.py
(outputs under out_close, victims exact where the probe calls the decision stable, at least 10 decisions and half of a case's triples,
and a distance of at least ten times the output bound to the standard-scale oracle: each case fails on a bank that ignores the scale)."""
import ctypes as C

import pytest
import torch

import tests.test_hip_softcap as TS
from tests.golden_util import out_close
from tests.softcap_ref import patched
from tests.test_hip_fullsize import Probe

pytestmark = pytest.mark.gpu
D, SCALE = 128, 144 ** -0.5


def test_one_launch_decode_step():
    TS.run_decode_case((1, 4, 2, 70, 1, "roco", True), D, "scale_only", SCALE, 1)


def test_split_decode_path():
    TS.run_decode_case((4, 2, 2, 200, 3, "tova", None), D, "scale_only", SCALE, 2)


def test_rope_on_read_decode_step():
    TS.run_decode_case((2, 2, 2, 75, 1, "h2o_head", True), D, "scale_only", SCALE, 3, stream=True)


CHUNKS = [
    # id, (rep, H, stride, idx, policy, two_pass, n_split), the step_info fields that name the kernel
    ("chunk_lds", (1, 3, 8, 210, "roco", 0, 0), dict(fused=1, wide=0, two_pass=0, n_launches=1)),
    ("16x16", (1, 3, 16, 300, "roco", -1, 0), dict(wide=0, two_pass=0)),
    ("resident_16x300", (1, 3, 16, 284, "roco", 0, 0), dict(fused=1, wide=1, two_pass=1, n_launches=1)),
    ("wide_stride48", (1, 2, 48, 400, "h2o_head", 1, 0), dict(fused=0, wide=1, two_pass=1)),
]


@pytest.mark.parametrize("name,shape,expect", CHUNKS, ids=[c[0] for c in CHUNKS])
def test_chunk_step_kernels(name, shape, expect):
    TS.run_chunk_case(shape, D, "scale_only", 4 + [c[0] for c in CHUNKS].index(name), sm_scale=SCALE, expect=expect)


def test_dense_prefix():
    from easykv_amd import KVBank, StepPlan
    from oracle import easykv_oracle as O
    L, H, n = 2, 2, 200
    g = torch.Generator().manual_seed(33100)
    q, k, v = TS._mk(L, H, n, g, D), TS._mk(L, H, n, g, D), TS._mk(L, H, n, g, D)
    bank = KVBank(L, H, H, D, cap=n + 64, sm_scale=SCALE)
    kw = dict(policy="full", phase="prefill", accumulate=False, evict=False, stride=n)
    assert bank.step_info(StepPlan(**kw), n)["wide"] == 1
    out, _ = bank.attend(StepPlan(**kw), q.cuda(), k.cuda(), v.cuda())
    dist = [0.0]
    with patched(None, SCALE, dist):
        for l in range(L):
            st = O.LayerState(k=torch.zeros(1, H, 0, D), v=torch.zeros(1, H, 0, D))
            o_ref, _ = O.layer_step(st, q[l:l + 1].float(), k[l:l + 1].float(), v[l:l + 1].float(), O.StepPlan(**kw))
            assert out_close(out[l].float().cpu(), o_ref[0]), (l, float((out[l].float().cpu() - o_ref[0]).abs().max()))
    assert dist[0] >= 10 * TS.OUT_BOUND, dist[0]


@pytest.mark.parametrize("n_split", [1, 3], ids=["one_launch", "split"])
def test_uniform_batch_step(n_split):
    """A KVBankBatch(sm_scale=...) step over three sequences of one length: the batch kernels read sm_div from the shared step."""
    import tests.test_hip_batch as TB
    from easykv_amd import KVBankBatch, StepPlan
    from oracle import easykv_oracle as O
    from tests.test_hip_lockstep import Hook
    Hq, H, B, T, policy = 4, 2, 3, 300, "roco"
    g = torch.Generator().manual_seed(33200)
    bat = KVBankBatch(B, 1, Hq, H, D, cap=T + 40, sm_scale=SCALE)
    kw = dict(policy=policy, phase="decode", evict=True, score_off=0, budget=T - 1, range_start=-1)
    for i in range(B):
        TB._fill(bat.bank, i, T - 1, g, T)
    plans, oplans = [StepPlan(**kw) for _ in range(B)], [O.StepPlan(**kw) for _ in range(B)]
    info = bat.step_info(plans, 0, None, n_split)
    assert bool(info["fused"]) == (n_split == 1), info
    seqs = [bat.sequence(i) for i in range(B)]
    hook = Hook()
    O.SELECT_HOOK = hook
    dist, n_dec = [0.0], 0
    try:
        with patched(None, SCALE, dist):
            for step in range(3):
                states = [TB._oracle_state(seqs[i], T) for i in range(B)]
                q, k, v = (TS._mk(B, hh, 1, g, D) for hh in (Hq, H, H))
                out, ids = bat.attend(plans, q.cuda(), k.cuda(), v.cuda(), 0, n_split=n_split)
                for i in range(B):
                    o_ref, ids_ref = O.layer_step(states[i], q[i:i + 1].float(), k[i:i + 1].float(), v[i:i + 1].float(), oplans[i])
                    nd, _ = TB._check_entry(("sm_scale", n_split, step, i), hook, policy, o_ref, ids_ref, out[i], ids[i], seqs[i], states[i], T, True, -1)
                    n_dec += nd
    finally:
        O.SELECT_HOOK = None
    assert n_dec == 3 * B * H and dist[0] >= 10 * TS.OUT_BOUND, (n_dec, dist[0])


def test_fp8_decode_step():
    """Decode steps of an FP8 bank with a free scale, held to the bar of tests/test_hip_kv8.py on the bank's own dequantised contents."""
    import tests.test_hip_kv8 as TK
    from easykv_amd import KVBank, StepPlan
    from oracle import easykv_oracle as O
    from tests import kv8_ref as R
    L, hq, h, budget, policy, steps = 4, 8, 4, 96, "roco", 30
    T = budget + 1
    g = torch.Generator().manual_seed(33300)
    bank = KVBank(L, hq, h, D, cap=T + 8, sm_scale=SCALE)
    bank.load_rows(torch.randn(L, h, budget, D, generator=g).half().cuda(), torch.randn(L, h, budget, D, generator=g).half().cuda())
    bank.state_init(T, 0)
    warm = torch.rand(L, h, budget, generator=g) * 1e-3
    bank.score_sum[:, :, :budget] += warm.cuda()
    bank.score_sq[:, :, :budget] += (warm ** 2).cuda()
    bank.quantize_fp8()
    layers = [0, L - 1]
    states = TK._oracle_states(bank, T, layers)
    kw = dict(policy=policy, phase="decode", evict=True, accumulate=True, score_off=0, budget=budget)
    plan = StepPlan(n_split=1, **kw)
    assert bank.step_info(plan, 1)["fused"] == 1
    probe = Probe()
    O.SELECT_HOOK = probe
    rows = torch.arange(h)
    dist, n_dec, n_stable = [0.0], 0, 0
    try:
        with patched(None, SCALE, dist):
            for i in range(steps):
                q, k, v = (torch.randn(L, hh, 1, D, generator=g).half() for hh in (hq, h, h))
                new_row = torch.stack([bank._slot_of_pos[l, :, bank.n_slots[l]] for l in layers]).cpu().long()
                out, ids = bank.attend(plan, q.cuda(), k.cuda(), v.cuda())
                reseed = []
                for j, l in enumerate(layers):
                    for given, codes, sc in ((k[l, :, 0], bank.k8[l], bank.k_scale[l]), (v[l, :, 0], bank.v8[l], bank.v_scale[l])):
                        R.check_rows(given, codes[rows, new_row[j]], sc[rows, new_row[j]], (i, l))
                    kd, vd = bank.dequantized_rows(l)
                    kq, vq = kd[rows, new_row[j]].cpu().view(1, h, 1, D), vd[rows, new_row[j]].cpu().view(1, h, 1, D)
                    o_ref, ids_ref = O.layer_step(states[l], q[l:l + 1].float(), kq, vq, O.StepPlan(**kw))
                    assert out_close(out[l].float().cpu(), o_ref[0]), (i, l, float((out[l].float().cpu() - o_ref[0]).abs().max()))
                    unstable = probe.last_unstable
                    same = ids[l, :, 0].cpu().long() == ids_ref[:, 0]
                    n_dec += h
                    n_stable += int((~unstable).sum())
                    assert bool(same[~unstable].all()), (i, l)
                    if not bool(same.all()):
                        reseed.append(l)
                if reseed:
                    states.update(TK._oracle_states(bank, T, reseed))
                    bank._slot_short = 0
    finally:
        O.SELECT_HOOK = None
    assert n_stable >= 0.9 * n_dec and dist[0] >= 10 * TS.OUT_BOUND, (n_stable, n_dec, dist[0])


def test_the_step_without_a_scale_is_byte_identical():
    """sm_scale=None: the ekv_step a bank builds is what it built before the scale existed (sm_div = sqrt(head_dim) in fp32)."""
    import math
    from easykv_amd import KVBank, StepPlan
    plan = StepPlan(policy="roco", phase="decode", evict=True, budget=64)
    a, b = KVBank(2, 4, 2, D, cap=128), KVBank(2, 4, 2, D, cap=128, sm_scale=SCALE)
    for bank in (a, b):
        bank.n_slots, bank.extent = [70, 70], [70, 70]
    sa, sb = a.make_step(plan, 1, 0, 2), b.make_step(plan, 1, 0, 2)
    ref = bytes(sa)
    sa.sm_div = math.sqrt(D)
    assert bytes(sa) == ref and C.c_float(math.sqrt(D)).value == sa.sm_div
    assert sb.sm_div == 12.0
    sb.sm_div = sa.sm_div
    assert bytes(sb) == ref
