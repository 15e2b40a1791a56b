"""Every decode instance of easykv_amd/csrc/ekv_instances.def is reached through its table entry and computes its own variant.

Parametrised from the manifest's EKV_DECODE lines (a future line is run without editing this file) x two head layouts: hq = h = 2,
and hq = 8, h = 2 (GQA 4: the rep = 4 build).  Per case one roco decode step with one victim on a 2-layer bank of cap 192, through

  * the one-launch kernel (n_split = 1) at n_slots = 100: more than one 64-row tile, not a multiple of 64;
  * a requested 2-way split at the same 100 slots.  The planner gives a decode split whole 128-row units, so at 100 slots this request
    is still ONE key range and the step is again the one-launch kernel (asserted: the dry run says so) — which is why the next shape
    is here: without it no case would reach an instance's split launcher;
  * a 2-way split at n_slots = 164 (two key ranges, the second one partial): split attention kernel + fast scorer.

A batch instance takes two entries, of that length and of 37 slots, in one call.

What is compared is what the existing tests of each variant compare against, with their helpers and bars:
  * fp16, 16-bit rows (plain and RoPE-on-read keys): the fp32 oracle; outputs under tests.golden_util.out_close, victims equal or in the
    oracle's own tolerance class (tests.test_hip_bf16._check_ids);
  * bf16, 16-bit rows: the fp32 oracle on .float() of the bf16 values; tests.test_hip_bf16._check_out / _check_ids;
  * kv8: the oracle on the bank's own dequantised contents and the appended row checked against the rule's torch restatement
    (tests/kv8_ref.py), as tests/test_hip_kv8.py does: out_close, victims identical wherever tests.test_hip_fullsize.Probe calls
    the decision well defined;
  * kv4: the same scheme with the MXFP4 rule (tests/kv4_ref.py) and the helpers of tests/test_hip_kv4.py;
  * batch: every entry against the uniform step of a twin bank that holds the entry's rows alone (tests/test_hip_batch.py's _fill /
    _copy_layer): identical victims, outputs under out_close — the bar tests/test_hip_decode_parity.py holds two kernels of one step to
    (the twin of a short entry runs the one-launch kernel where the batch runs the envelope's split).  A batch line on quantised rows
    quantises the batch bank and the twins alike (quantize(kind)) once they are filled, so the call launches the line's own instance.
bf16 cases draw V at 1/4 scale for the reason tests/test_hip_kv8.py gives: the flat 1e-3 bar then applies to a bf16 output too.

A table entry wired to another head_dim or element type misses these bars by orders of magnitude or fails to launch."""
import pytest
import torch

from tests import kv8_ref as R
from tests.golden_util import out_close

pytestmark = pytest.mark.gpu
BF, F16 = torch.bfloat16, torch.float16
L, CAP = 2, 192
# (n_slots of the step, requested n_split, the dry run's answer: one launch?)
PATHS = [(100, 1, True), (100, 2, True), (164, 2, False)]
SHORT = 37      # the second entry of a batch
KIND = {"kv16": None, "kv8": "fp8", "kv4": "mxfp4"}      # the manifest's `rows` word -> KVBank.quantize(kind)
# Instances the planner cannot reach at these shapes, by object name, with the reason.  (None: RoPE-on-read decode steps get their
# tables from the oracle's rope_tables.)
EXCLUDED = {}


def _decode_lines():
    from easykv_amd import _build
    out = []
    for fam, words in _build.instances():
        if fam == "EKV_DECODE":
            name = _build.FAMILIES[fam](*words)[1]
            if name not in EXCLUDED:
                out.append(pytest.param(*words, id=name))
    return out


def _bank(hq, h, D, dtype, rows, g, rope):
    """A 2-layer bank of `rows` live rows per head (scattered slot map) with a warm decoding score state of width rows + 1."""
    from easykv_amd import KVBank
    from tests.test_hip_batch import _fill
    bank = KVBank(L, hq, h, D, cap=CAP, dtype=dtype)
    if rope is not None:
        bank.set_rope(*rope)
    bank.k.zero_(), bank.v.zero_()
    for l in range(L):
        _fill(bank, l, rows, g, rows + 1)
    if dtype is BF:
        bank.v.mul_(0.25)      # (exact: see the module docstring)
    return bank


def _tokens(n, hq, h, D, dtype, g):
    vs = 0.25 if dtype is BF else 1.0      # (see the module docstring)
    return (torch.randn(n, hq, 1, D, generator=g).to(dtype), torch.randn(n, h, 1, D, generator=g).to(dtype),
            (torch.randn(n, h, 1, D, generator=g) * vs).to(dtype))


def _check_16bit(tag, bank, plan, oplan, dtype, rope, g):
    from oracle import easykv_oracle as O
    from tests.test_hip_bf16 import _check_ids, _check_out, _pv, _seed
    from tests.test_hip_lockstep import Hook
    hq, h, D = bank.n_q_heads, bank.n_kv_heads, bank.head_dim
    states = _seed(bank, plan.budget + 1)
    q, k, v = _tokens(L, hq, h, D, dtype, g)
    out, ids = bank.attend(plan, q.cuda(), k.cuda(), v.cuda())
    assert out.dtype == dtype
    hook = Hook()
    O.SELECT_HOOK = hook
    try:
        for l in range(L):
            st = states[l]
            k_all, v_all = torch.cat([st.k[0], k[l].float()], 1), torch.cat([st.v[0], v[l].float()], 1)
            o_ref, ids_ref = O.layer_step(st, q[l:l + 1].float(), k[l:l + 1].float(), v[l:l + 1].float(), oplan, *(rope or ()))
            err = float((out[l].float().cpu() - o_ref[0]).abs().max())
            print(f"[instances] {tag} layer {l}: max |o - ref| = {err:.3e}")
            if dtype is BF:
                _check_out(out[l], o_ref[0], _pv(q[l].float(), k_all, v_all, k_all.shape[1] - 1), (tag, l))
            else:
                assert out_close(out[l].float().cpu(), o_ref[0]), (tag, l, err)
            _check_ids(hook, ids[l].cpu(), ids_ref.view(h, -1), (tag, l))
    finally:
        O.SELECT_HOOK = None


def _check_kv8(tag, bank, plan, oplan, dtype, g):
    from oracle import easykv_oracle as O
    from tests.test_hip_fullsize import Probe
    from tests.test_hip_kv8 import _oracle_states
    hq, h, D = bank.n_q_heads, bank.n_kv_heads, bank.head_dim
    states = _oracle_states(bank, plan.budget + 1, range(L))
    q, k, v = _tokens(L, hq, h, D, dtype, g)
    rows = torch.arange(h)
    new_row = torch.stack([bank._slot_of_pos[l, :, bank.n_slots[l]] for l in range(L)]).cpu().long()
    out, ids = bank.attend(plan, q.cuda(), k.cuda(), v.cuda())
    assert out.dtype == dtype
    probe = Probe()
    O.SELECT_HOOK = probe
    try:
        for l in range(L):
            for given, codes, sc in ((k[l, :, 0], bank.k8[l], bank.k_scale[l]), (v[l, :, 0], bank.v8[l], bank.v_scale[l])):
                R.check_rows(given, codes[rows, new_row[l]], sc[rows, new_row[l]], (tag, l))
            kd, vd = bank.dequantized_rows(l)
            kq, vq = kd[rows, new_row[l]].cpu().view(1, h, 1, D), vd[rows, new_row[l]].cpu().view(1, h, 1, D)
            o_ref, ids_ref = O.layer_step(states[l], q[l:l + 1].float(), kq, vq, oplan)
            err = float((out[l].float().cpu() - o_ref[0]).abs().max())
            print(f"[instances] {tag} layer {l}: max |o - ref| = {err:.3e}")
            assert out_close(out[l].float().cpu(), o_ref[0]), (tag, l, err)
            same = ids[l, :, 0].cpu().long() == ids_ref[:, 0]
            assert bool(same[~probe.last_unstable].all()), (tag, l)
    finally:
        O.SELECT_HOOK = None


def _check_kv4(tag, bank, plan, oplan, dtype, g):
    from oracle import easykv_oracle as O
    from tests.test_hip_fullsize import Probe
    from tests.test_hip_kv4 import _appended_rows_are_the_rules, _oracle_states
    hq, h, D = bank.n_q_heads, bank.n_kv_heads, bank.head_dim
    states = _oracle_states(bank, plan.budget + 1, range(L))
    q, k, v = _tokens(L, hq, h, D, dtype, g)
    rows = torch.arange(h)
    new_row = torch.stack([bank._slot_of_pos[l, :, bank.n_slots[l]] for l in range(L)]).cpu().long()
    out, ids = bank.attend(plan, q.cuda(), k.cuda(), v.cuda())
    assert out.dtype == dtype
    probe = Probe()
    O.SELECT_HOOK = probe
    try:
        for l in range(L):
            _appended_rows_are_the_rules(bank, l, rows, new_row[l], k[l, :, 0], v[l, :, 0], (tag, l))
            kd, vd = bank.dequantized_rows(l)
            kq, vq = kd[rows, new_row[l]].cpu().view(1, h, 1, D), vd[rows, new_row[l]].cpu().view(1, h, 1, D)
            o_ref, ids_ref = O.layer_step(states[l], q[l:l + 1].float(), kq, vq, oplan)
            err = float((out[l].float().cpu() - o_ref[0]).abs().max())
            print(f"[instances] {tag} layer {l}: max |o - ref| = {err:.3e}")
            assert out_close(out[l].float().cpu(), o_ref[0]), (tag, l, err)
            same = ids[l, :, 0].cpu().long() == ids_ref[:, 0]
            assert bool(same[~probe.last_unstable].all()), (tag, l)
    finally:
        O.SELECT_HOOK = None


def _check_batch(tag, hq, h, D, dtype, rows, T, n_split, one_launch, g):
    """Entries of T and SHORT slots in one call, each against the uniform step of a twin bank that holds its rows alone."""
    from easykv_amd import KVBank, KVBankBatch, StepPlan
    from tests.test_hip_batch import _copy_layer, _fill
    lens = (T, SHORT)
    bat = KVBankBatch(len(lens), 1, hq, h, D, cap=CAP, dtype=dtype)
    bat.bank.k.zero_(), bat.bank.v.zero_()
    twins, plans = [], []
    for i, t in enumerate(lens):
        _fill(bat.bank, i, t - 1, g, t)
        if dtype is BF:
            bat.bank.v[i].mul_(0.25)      # (exact: see the module docstring)
        twin = KVBank(1, hq, h, D, cap=CAP, dtype=dtype)
        twin.use_slot_rows = False      # like against like: a batch runs the ordered score-row layout
        _copy_layer(bat.bank, i, twin, 0)
        twins.append(twin)
        plans.append(StepPlan(policy="roco", phase="decode", evict=True, score_off=0, budget=t - 1, n_split=n_split))
    if KIND[rows] is not None:      # the line's own row format: the same conversion of the same rows on both sides
        for b in [bat] + twins:
            b.quantize(KIND[rows])
        assert bat.kv_quant == KIND[rows]
    info = bat.step_info(plans, 0, None, n_split)
    assert bool(info["fused"]) == one_launch and (info["n_split"] > 1) == (not one_launch), (tag, info)
    q, k, v = (x.cuda() for x in _tokens(len(lens), hq, h, D, dtype, g))
    out, ids = bat.attend(plans, q, k, v, 0, n_split=n_split)
    assert out.dtype == dtype
    for i, t in enumerate(lens):
        o_ref, ids_ref = twins[i].attend(plans[i], q[i:i + 1], k[i:i + 1], v[i:i + 1])
        err = float((out[i].float() - o_ref[0].float()).abs().max())
        print(f"[instances] {tag} entry of {t} slots: max |o - uniform| = {err:.3e}")
        assert torch.equal(ids[i], ids_ref[0]), (tag, t)
        assert out_close(out[i].float(), o_ref[0].float()), (tag, t, err)
        assert bat.n_slots(i) == t - 1


@pytest.mark.parametrize("hq,h", [(2, 2), (8, 2)], ids=["mha", "gqa4"])
@pytest.mark.parametrize("head_dim,keys,element,rows,batching", _decode_lines())
def test_instance_runs_its_own_variant(head_dim, keys, element, rows, batching, hq, h):
    from easykv_amd import StepPlan
    from oracle import easykv_oracle as O
    D, dtype = int(head_dim), {"f16": F16, "bf16": BF}[element]
    rope = O.rope_tables(CAP + 8, D) if keys == "rope" else None
    g = torch.Generator().manual_seed(D * 100 + hq)
    for T, n_split, one_launch in PATHS:
        tag = (f"d{D} {keys} {element} {rows} {batching} hq={hq}", T, n_split)
        if batching == "batch":
            _check_batch(tag, hq, h, D, dtype, rows, T, n_split, one_launch, g)
            continue
        bank = _bank(hq, h, D, dtype, T - 1, g, rope)
        if KIND[rows] is not None:
            bank.quantize(KIND[rows])
        kw = dict(policy="roco", phase="decode", evict=True, score_off=0, budget=T - 1, streaming=keys == "rope")
        plan = StepPlan(n_split=n_split, **kw)
        info = bank.step_info(plan, 1)
        assert bool(info["fused"]) == one_launch and (info["n_split"] > 1) == (not one_launch), (tag, info)
        if rows == "kv8":
            _check_kv8(tag, bank, plan, O.StepPlan(**kw), dtype, g)
        elif rows == "kv4":
            _check_kv4(tag, bank, plan, O.StepPlan(**kw), dtype, g)
        else:
            _check_16bit(tag, bank, plan, O.StepPlan(**kw), dtype, rope, g)


def test_every_decode_line_is_covered_or_excluded_by_name():
    from easykv_amd import _build
    names = [_build.FAMILIES[fam](*words)[1] for fam, words in _build.instances() if fam == "EKV_DECODE"]
    assert set(EXCLUDED) <= set(names) and all(n.endswith("_rope") for n in EXCLUDED), EXCLUDED
    assert len(_decode_lines()) + len(EXCLUDED) == len(names) >= 24
