"""The chunk step on FP8 rows (ekv_attn_chunk8.inc) at its geometry edges, on the GPU: the cases of tests/kv8_chunk_edge_cases.py — new rows
that straddle a key-range split, empty (split, query block) pairs, short last blocks and idle query waves, GQA factors that do not divide
32, one- and two-query blocks, ranges that end next to a 32- or 64-position boundary, a layer sub-range — which tests/test_kv8_chunk_edges_cpu.py
holds to what they claim to reach.

(a) every case against the CPU oracle in float64 ON THE BANK'S OWN CONTENTS, exactly as tests/test_hip_kv8_chunk.py compares its six shapes
    (outputs under out_close, appended rows under kv8_ref.check_rows, victims by _exact_heads with at least one exact head, score rows at
    rtol 1e-3 / atol 1e-5), (b) with every physical row no step names bit-equal afterwards; three cases also accumulate-only, where no
    selection is involved and every head's score rows are compared;
(c) HF-style views of q / k_new / v_new and a token-major `out` against dense copies on a twin bank, bit for bit, immediate and deferred;
(d) the deferred form (one attend(defer=True) per layer, then flush()) against float64, and against an immediate one-call twin;
(e) two evicting steps in a row: the second reads the rows the first one's prologue stored, through the slot map its compaction changed.

Every bank has its physical rows scattered (kv8_chunk_edge_cases.scatter_rows), so a position is never its own physical row."""
import pytest
import torch

from tests import kv8_chunk_edge_cases as E
from tests import kv8_ref as R
from tests.golden_util import out_close
from tests.test_hip_d256 import _ProbeAndCapture
from tests.test_hip_kv8 import _oracle_states
from tests.test_hip_kv8_chunk import _exact_heads, _f64

pytestmark = pytest.mark.gpu
PLANES = ("k8", "v8", "k_scale", "v_scale")


def _snapshot(bank):
    return {name: getattr(bank, name).clone() for name in PLANES}


def _check_untouched(bank, snap, lb, new_rows, what):
    """(b) every physical row other than new_rows [layers from lb, H, n] is bit-equal to the snapshot, in every layer and head."""
    touched = torch.zeros(bank.n_layers, bank.n_kv_heads, bank.cap, dtype=torch.bool, device=new_rows.device)
    touched[lb:lb + new_rows.shape[0]].scatter_(2, new_rows, True)
    assert int(touched.sum()) == new_rows.numel(), what
    for name, before in snap.items():
        after = getattr(bank, name)
        assert torch.equal(before[~touched], after[~touched]), (what, name, "a row no step names has changed")


def _check_appended(case, bank, k, v, lb, new_rows, what):
    heads = torch.arange(case.H).unsqueeze(-1)
    for ll in range(new_rows.shape[0]):
        rows = new_rows[ll].cpu()
        for given, codes, sc in ((k[ll], bank.k8[lb + ll], bank.k_scale[lb + ll]), (v[ll], bank.v8[lb + ll], bank.v_scale[lb + ll])):
            R.check_rows(given, codes.cpu()[heads, rows], sc.cpu()[heads, rows], what)


def _against_float64(case, bank, states, tokens, out, ids, lb, T, kw, what, need_exact=True):
    """Outputs, victims and score rows of the stepping layers against the oracle's float64 step from `states` (seeded from the bank before
    the step).  Returns the largest |out - ref| and, per layer, the heads the probe calls stable."""
    from oracle import easykv_oracle as O
    q, k, v = tokens
    n, evicting, scored = case.n, kw["evict"], kw["accumulate"]
    kq, vq = (R.dequant(*R.quantize(x)).double() for x in (k, v))      # new rows as the rule quantises them
    worst, stable = 0.0, []
    for ll in range(q.shape[0]):
        l = lb + ll
        st = states[l] if states else O.LayerState(k=torch.zeros(1, case.H, 0, case.D), v=torch.zeros(1, case.H, 0, case.D))
        hook = _ProbeAndCapture()
        O.SELECT_HOOK = hook
        try:
            o_ref, ids_ref = O.layer_step(_f64(st), q[ll:ll + 1].double(), kq[ll:ll + 1], vq[ll:ll + 1], O.StepPlan(**kw))
        finally:
            O.SELECT_HOOK = None
        err = float((out[ll].double().cpu() - o_ref[0]).abs().max())
        worst = max(worst, err)
        assert out_close(out[ll].float().cpu(), o_ref[0].float()), (what, l, err)
        if not scored:
            continue
        heads, width = range(case.H), T + n      # accumulate-only: no selection, every head, every column
        if evicting:
            heads, _ = _exact_heads(hook, case.policy, ids[ll], ids_ref, max(T - kw["recent"] - kw["sink"], n), kw["sink"], n)
            assert heads or not need_exact, (what, l, "no head of this case was compared exactly: pick another seed")
            width = T
            stable.append(~hook.probe.last_unstable)
        for h in heads:      # the score rows the exported logits were accumulated into, after the same compaction
            for got, ref in ((bank.score_sum, st.s), (bank.score_sq, st.q)):
                assert torch.allclose(got[l, h, :width].cpu().double(), ref[h, :width], rtol=1e-3, atol=1e-5), (what, l, h)
    print(f"[kv8-chunk-edges] {what} {case.dtype}: max |out - ref| = {worst:.3e}")
    return worst, stable


def _one_step(case, bank, tokens, evict=True, what="", need_exact=True):
    """(a) + (b) for one immediate step of `case` on `bank`."""
    from easykv_amd import StepPlan
    lb, L, n = case.layer_begin, case.L, case.n
    T = bank.n_slots[lb]
    kw = E.plan_kw(case, evict)
    plan = StepPlan(n_split=case.n_split, **kw)
    info = bank.step_info(plan, n, lb, L - lb)
    assert info["n_launches"] > 0 and info["two_pass"] == 0 and info["wide"] == 0, info
    assert (info["n_split"], info["n_qblocks"], info["qb_rows"]) == case.expect, info
    states = _oracle_states(bank, T + n, range(lb, L)) if T else None
    new_rows = bank.slot_of_pos[lb:L, :, T:T + n].long().clone()      # the front of the free list
    snap = _snapshot(bank)
    idle = [x[:lb].clone() for x in (bank.slot_of_pos, bank.score_sum, bank.score_sq, bank.score_cnt)]
    q, k, v = tokens
    ws = bank._ws
    out, ids = bank.attend(plan, q.cuda(), k.cuda(), v.cuda(), layer_begin=lb)
    assert out.dtype == case.dtype and bank.k is None and bank.v is None and bank._ws is ws      # (the workspace build_bank filled)
    assert bank.n_slots == [T] * lb + [T if kw["evict"] else T + n] * (L - lb)
    _check_untouched(bank, snap, lb, new_rows, what)
    for before, after in zip(idle, (bank.slot_of_pos, bank.score_sum, bank.score_sq, bank.score_cnt)):      # the layers that do not step
        assert torch.equal(before, after[:lb]), what
    _check_appended(case, bank, k, v, lb, new_rows, what)
    return _against_float64(case, bank, states, tokens, out, ids, lb, T, kw, what, need_exact)


@pytest.mark.parametrize("case", E.CASES, ids=lambda c: c.name)
def test_edge_case_against_float64(case):
    d = E.draw(case)
    bank = E.build_bank(case, d)
    assert bank.k is None and bank.v is None and bank.n_slots == [case.T0] * case.L
    _one_step(case, bank, d["tokens"][0], what=case.name)


@pytest.mark.parametrize("name", E.NON_EVICTING)
def test_edge_case_accumulate_only(name):
    """accumulate=True, evict=False: no selection is involved, so EVERY head's score rows are compared over all T + n columns."""
    case = E.BY_NAME[name]
    d = E.draw(case)
    _one_step(case, E.build_bank(case, d), d["tokens"][0], evict=False, what=name + " accumulate-only")


@pytest.mark.parametrize("name", E.TWO_STEPS)
def test_two_steps_in_a_row(name):
    """(e) the second step's cache rows include the ones the first step's prologue stored, and its slot map is the one the first step's
    compaction left (the first step's victims' rows are the second step's free list).  Which heads of the second step are stable depends
    on the first step's victims, so only the first step is required to have an exact head."""
    case = E.BY_NAME[name]
    d = E.draw(case, steps=2)
    bank = E.build_bank(case, d)
    for i, tokens in enumerate(d["tokens"]):
        _one_step(case, bank, tokens, what=f"{name} step {i}", need_exact=i == 0)
    assert bank.n_slots == [case.T0] * case.L
    m = bank.slot_of_pos.cpu()
    assert all(torch.equal(torch.sort(m[l, h])[0], torch.arange(bank.cap, dtype=m.dtype)) for l in range(case.L) for h in range(case.H))


def _hf_view(x):
    """x [L, heads, n, D] on the CPU -> the same values on the GPU as [L, n, heads * D] storage seen as [L, heads, n, D]."""
    L, heads, n, D = x.shape
    view = x.transpose(1, 2).contiguous().view(L, n, heads * D).cuda().view(L, n, heads, D).transpose(1, 2)
    assert not view.is_contiguous() and view.stride(2) == heads * D and view.stride(1) == D
    return view


def _run(case, bank, q, k, v, defer, strided, n_split=None):
    """One step of all layers, immediate (one call) or deferred (one call per layer, then flush()).  Returns (out, ids)."""
    from easykv_amd import StepPlan
    L, n, Hq = case.L, case.n, case.H * case.rep
    plan = StepPlan(n_split=case.n_split if n_split is None else n_split, **E.plan_kw(case))
    o = torch.empty(L, n, Hq, case.D, dtype=case.dtype, device="cuda").transpose(1, 2) if strided else \
        torch.empty(L, Hq, n, case.D, dtype=case.dtype, device="cuda")
    ws = bank._ws
    if defer:
        for l in range(L):
            bank.attend(plan, q[l:l + 1], k[l:l + 1], v[l:l + 1], layer_begin=l, defer=True, out=o[l:l + 1])
        ids = bank.flush()
    else:
        got, ids = bank.attend(plan, q, k, v, out=o)
        assert got is o
    assert bank._ws is ws      # (the workspace build_bank filled)
    if strided:
        assert o.stride(2) == Hq * case.D and o.stride(1) == case.D and o.transpose(1, 2).is_contiguous()
    return o, ids


@pytest.mark.parametrize("defer", [False, True], ids=["immediate", "deferred"])
@pytest.mark.parametrize("name", E.VIEWS)
def test_views_equal_dense_copies(name, defer):
    """(c) twin banks, one fed dense tensors, one the views a HF attention module hands over: everything the step leaves is bit-equal."""
    case = E.with_layers(E.BY_NAME[name], 3 if defer else 1)
    d = E.draw(case)
    q, k, v = d["tokens"][0]
    a, b = E.build_bank(case, d), E.build_bank(case, d)
    (oa, ia), (ob, ib) = _run(case, a, q.cuda(), k.cuda(), v.cuda(), defer, False), _run(case, b, _hf_view(q), _hf_view(k), _hf_view(v), defer, True)
    assert torch.equal(oa, ob), (name, float((oa.float() - ob.float()).abs().max()))
    assert torch.equal(ia, ib) and a.n_slots == b.n_slots == [case.T0] * case.L
    assert torch.equal(a.slot_of_pos, b.slot_of_pos)
    t = case.T0
    assert torch.equal(a.score_sum[:, :, :t], b.score_sum[:, :, :t]) and torch.equal(a.score_sq[:, :, :t], b.score_sq[:, :, :t])
    assert torch.equal(a.score_cnt[:, :, :t], b.score_cnt[:, :, :t])
    for name_ in PLANES:
        assert torch.equal(getattr(a, name_), getattr(b, name_)), name_


@pytest.mark.parametrize("name", E.VIEWS)
def test_deferred_form_against_float64_and_an_immediate_twin(name):
    """(d) the deferred run of three layers on dense inputs: every layer against float64 as in (a), untouched rows as in (b); then an
    immediate one-call twin with n_split pinned to the deferred plan's: victims identical on stable heads, outputs bit-equal.  Both plans
    run the same attention and the same fold arithmetic: an unsplit head is folded inside the attention kernel in both forms (the immediate
    one-block step merely has the scorer as that kernel's tail); a split head's key-range partials are folded by the fold launch behind the
    attention kernel (deferred, phases 1 | 4) or by the generic scorer's first stage (immediate) — two launches, one function
    (ekv_fold_partials, ekv_common.h, whose result does not depend on the batch width) over the same partials."""
    case = E.with_layers(E.BY_NAME[name], 3)
    d = E.draw(case)
    q, k, v = d["tokens"][0]
    T, n, kw = case.T0, case.n, E.plan_kw(case)
    bank = E.build_bank(case, d)
    states = _oracle_states(bank, T + n, range(case.L))
    new_rows = bank.slot_of_pos[:, :, T:T + n].long().clone()
    snap = _snapshot(bank)
    out, ids = _run(case, bank, q.cuda(), k.cuda(), v.cuda(), True, False)
    n_split = bank._defer["st"].n_split      # what the deferred plan ran with
    assert n_split == case.expect[0] and bank.n_slots == [T] * case.L
    _check_untouched(bank, snap, 0, new_rows, name)
    _check_appended(case, bank, k, v, 0, new_rows, name)
    _, stable = _against_float64(case, bank, states, (q, k, v), out, ids, 0, T, kw, name + " deferred")
    twin = E.build_bank(case, d)
    out2, ids2 = _run(case, twin, q.cuda(), k.cuda(), v.cuda(), False, False, n_split=n_split)
    for l in range(case.L):
        ok = stable[l]
        assert bool(ok.any()) and torch.equal(torch.sort(ids[l].cpu()[ok], dim=-1)[0], torch.sort(ids2[l].cpu()[ok], dim=-1)[0]), (name, l)
    assert torch.equal(out, out2), (name, n_split, float((out.float() - out2.float()).abs().max()))
