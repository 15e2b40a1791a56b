"""One-shot prompt compression with pooled observation-window scores on the GPU (include/easykv_hip.h, "pooled selection" and "one-shot
prefill") against tests/oneshot_ref.py, the oracle's primitives with torch's pooling in front of its topk.

(a) A pooled step against the reference: L = 2; head_dim 128 with 4 / 2 heads and head_dim 64 with 16 / 2; fp16 and bf16; h2o_head and
    tova; max and avg; kernel sizes 3 and 7; sink 4, obs 8 and 32; T = 300 (one key range) and 1500 with n_split = 2 (partials folded);
    n_evict = T - 64 and T / 2; immediate and deferred.  Every value is visited by every (shape, dtype, policy, op) case through four
    inner configurations.  Outputs under out_close (bf16: the bar of tests/test_hip_sink.py); victims under the tolerance class of
    tests/oneshot_ref.py; the score rows, the slot map (through ordered_kv) and the lengths as the unpooled scorer leaves them FOR THE
    DEVICE'S OWN victims (rtol 2e-5, atol 1e-7 on the score rows, the K/V rows exactly).
(b) one case past the LDS row, on the scratch path; (c) one refusal just past the pooled width; (d) pool = 1: an argument error through
    ekv_pool_*, the plain call bit for bit through the engine; (e) an unpooled one-shot step with roco and n_evict = T - 64 under the
    class rule of tests/select_rule.py; (f) the hand-over; (g) generate with the key against the test-side driver, a stock tiny HF Llama
    and a tiny sink + window gpt-oss with score_pool = 1; (h) generate_batch with the key: every sequence equals its solo run.

The seeds are chosen so that the reference alone meets the class's cap (at least 90 % of a row's candidate columns and at least 10 of its
victims decided): test_reference_rows_meet_the_cap checks that without a GPU."""
import contextlib
import ctypes
import io

import numpy as np
import pytest
import torch

from tests import oneshot_ref as R
from tests.golden_util import out_close

gpu = pytest.mark.gpu
BF = torch.bfloat16
SINK = 4
SHAPES = {"d128_gqa2": (128, 4, 2), "d64_gqa8": (64, 16, 2)}
# kernel size, obs, T, victims, n_split, deferred
INNER = [(3, 8, 300, "most", 1, False), (7, 32, 1500, "half", 2, True), (7, 8, 1500, "most", 2, False), (3, 32, 300, "half", 1, True)]
CASES = [(s, dt, pol, op) for s in SHAPES for dt in ("f16", "bf16") for pol in ("h2o_head", "tova") for op in ("max", "avg")]


def _mk(L, H, n, g, d, dtype):
    return torch.randn(L, H, n, d, generator=g).to(dtype)


def _n_evict(T, kind):
    return T - 64 if kind == "most" else T // 2


def _data(shape, dt, T, obs, seed):
    D, Hq, H = SHAPES[shape]
    dtype = BF if dt == "bf16" else torch.float16
    g = torch.Generator().manual_seed(seed)
    L = 2
    return dict(D=D, Hq=Hq, H=H, L=L, dtype=dtype, k0=_mk(L, H, T - obs, g, D, dtype), v0=_mk(L, H, T - obs, g, D, dtype),
                q=_mk(L, Hq, obs, g, D, dtype), k=_mk(L, H, obs, g, D, dtype), v=_mk(L, H, obs, g, D, dtype))


def _seed(shape, dt, pol, op, i):
    return 71000 + 97 * CASES.index((shape, dt, pol, op)) + i


def _reference(d, T, obs, policy, n_evict, pool, op):
    """Per layer: (o, ids, ranking rows, the accumulated state BEFORE compaction, p.|V| for the bf16 bar)."""
    from oracle import easykv_oracle as O
    out = []
    for l in range(d["L"]):
        st = O.LayerState(k=d["k0"][l:l + 1].float(), v=d["v0"][l:l + 1].float())
        st.s, st.q, st.c = O.init_state_prefill((d["H"],), T - obs, obs, False)
        qf, kf, vf = d["q"][l:l + 1].float(), d["k"][l:l + 1].float(), d["v"][l:l + 1].float()
        o, ids, rank = R.observation_step(st, qf, kf, vf, policy, n_evict, SINK, pool, op)
        pv = O.attention_core(qf, st.k, st.v.abs(), O.causal_chunk_mask(obs, T, qf.dtype))[0][0] if d["dtype"] is BF else None
        out.append(dict(o=o[0], ids=ids, rank=rank, st=st, pv=pv))
    return out


def _bf16_close(out, ref, pv):
    err = (out - ref).abs()
    return bool(torch.isfinite(out).all()) and bool((err <= 2.0 ** -8 * (ref.abs() + pv) + 1e-6 * pv).all())


@pytest.mark.parametrize("shape,dt,policy,op", CASES, ids=["-".join(c) for c in CASES])
def test_reference_rows_meet_the_cap(shape, dt, policy, op):
    """Not a GPU test: the reference alone, on the seeds of (a) — every compared row has at least 90 % of its candidates and at least 10
    victims decided, and the reference's own victims are an answer of its class."""
    for i, (ks, obs, T, kind, _, _) in enumerate(INNER):
        ne = _n_evict(T, kind)
        for ref in _reference(_data(shape, dt, T, obs, _seed(shape, dt, policy, op, i)), T, obs, policy, ne, ks, op):
            for h in range(ref["rank"].shape[0]):
                assert R.meets_cap(ref["rank"][h], ne, SINK, obs), (i, h, [len(x) if isinstance(x, set) else x for x in R.row_class(ref["rank"][h], ne, SINK, obs)])
                assert R.valid(ref["ids"][h], ref["rank"][h], ne, SINK, obs), (i, h)


def _step(bank, plan, d, deferred):
    q, k, v = d["q"].cuda(), d["k"].cuda(), d["v"].cuda()
    if not deferred:
        return bank.attend(plan, q, k, v)
    outs = [bank.attend(plan, q[l:l + 1], k[l:l + 1], v[l:l + 1], layer_begin=l, defer=True)[0] for l in range(d["L"])]
    return torch.cat(outs), bank.flush()


def _check_step(bank, d, refs, out, ids, T, obs, ne, policy, tag, check_victims):
    """Outputs, victims (by `check_victims(layer, head, ids)`), and the state the unpooled scorer's code leaves for the device's victims."""
    from oracle import easykv_oracle as O
    from tests.test_hip_d256 import _permutation
    assert tuple(ids.shape) == (d["L"], d["H"], ne) and bank.n_slots == [T - ne] * d["L"], (tag, ids.shape, bank.n_slots)
    ids_c = ids.cpu().long()
    kk, vv = bank.ordered_kv()
    S, Q, C = bank.score_sum.cpu(), bank.score_sq.cpu(), bank.score_cnt.cpu()
    for l, ref in enumerate(refs):
        got = out[l].float().cpu()
        close = out_close(got, ref["o"]) if d["dtype"] is not BF else _bf16_close(got, ref["o"], ref["pv"])
        assert close, (tag, l, float((got - ref["o"]).abs().max()))
        for h in range(d["H"]):
            assert bool((ids_c[l, h, 1:] > ids_c[l, h, :-1]).all()), (tag, l, h, "evict_ids ascend")
            check_victims(l, h, ids_c[l, h])
        st = ref["st"]
        want = O.drop_columns(st.s, ids_c[l], torch.zeros(ne))
        assert torch.allclose(S[l, :, :T], want, rtol=2e-5, atol=1e-7), (tag, l, "score_sum", float((S[l, :, :T] - want).abs().max()))
        if policy == "roco":
            want_q, want_c = O.drop_columns(st.q, ids_c[l], torch.zeros(ne)), O.drop_columns(st.c, ids_c[l], -torch.arange(ne, dtype=torch.float32))
            assert torch.allclose(Q[l, :, :T], want_q, rtol=2e-5, atol=1e-7) and torch.equal(C[l, :, :T], want_c), (tag, l, "roco rows")
        k_all, v_all = torch.cat((d["k0"][l], d["k"][l]), 1)[None], torch.cat((d["v0"][l], d["v"][l]), 1)[None]
        assert torch.equal(kk[l].cpu(), O.drop_kv_slots(k_all, ids_c[l])[0]) and torch.equal(vv[l].cpu(), O.drop_kv_slots(v_all, ids_c[l])[0]), (tag, l, "rows")
    _permutation(bank)


@gpu
@pytest.mark.parametrize("shape,dt,policy,op", CASES, ids=["-".join(c) for c in CASES])
def test_pooled_step_against_the_reference(shape, dt, policy, op):
    from easykv_amd import KVBank, StepPlan
    n_decided = n_rows = 0
    for i, (ks, obs, T, kind, n_split, deferred) in enumerate(INNER):
        ne = _n_evict(T, kind)
        d = _data(shape, dt, T, obs, _seed(shape, dt, policy, op, i))
        refs = _reference(d, T, obs, policy, ne, ks, op)
        bank = KVBank(d["L"], d["Hq"], d["H"], d["D"], cap=T + 8, dtype=d["dtype"])
        bank.load_rows(d["k0"].cuda(), d["v0"].cuda())
        bank.state_init(T, 2, obs)
        plan = StepPlan(policy=policy, phase="prefill", accumulate=True, evict=True, budget=T, recent=obs, sink=SINK, stride=obs, n_evict=ne,
                        pool=ks, pool_op=op, n_split=n_split)
        info = bank.step_info(plan, obs)
        assert info["fused"] == 0 and info["n_split"] == n_split and info["n_launches"] >= 2, (shape, i, info)
        out, ids = _step(bank, plan, d, deferred)
        tag = (shape, dt, policy, op, i)

        def victims(l, h, v):
            assert R.valid(v, refs[l]["rank"][h], ne, SINK, obs), (tag, l, h, sorted(set(v.tolist()) ^ set(refs[l]["ids"][h].tolist()))[:20])
        _check_step(bank, d, refs, out, ids, T, obs, ne, policy, tag, victims)
        for ref in refs:
            for h in range(d["H"]):
                must, free, n_cand = R.row_class(ref["rank"][h], ne, SINK, obs)
                n_decided += n_cand - len(free)
                n_rows += n_cand
    print(f"[oneshot] {shape} {dt} {policy} {op}: {n_decided} of {n_rows} candidate columns decided")
    assert n_decided >= 0.9 * n_rows


@gpu
def test_pooled_step_past_the_lds_row_runs_on_the_scratch_path():
    """W = 9920: the four rows of the 512-thread build need 164 448 bytes > one CU's 160 KB, so the score rows live in global scratch and
    the stencil reads them there (the 1024-thread build); W = 9856 still fits."""
    from easykv_amd import KVBank, StepPlan
    obs, T, ks = 8, 9920, 7
    for name, n in (("lds", 16 * 9856 + 64 + 5664), ("scratch", 16 * T + 64 + 5664)):
        assert (n > 160 * 1024) == (name == "scratch"), (name, n)      # ekv_score_lds_bytes(512, W, rows = 8, big = false)
    g = torch.Generator().manual_seed(72001)
    d = dict(D=64, Hq=1, H=1, L=1, dtype=torch.float16, k0=_mk(1, 1, T - obs, g, 64, torch.float16), v0=_mk(1, 1, T - obs, g, 64, torch.float16),
             q=_mk(1, 1, obs, g, 64, torch.float16), k=_mk(1, 1, obs, g, 64, torch.float16), v=_mk(1, 1, obs, g, 64, torch.float16))
    for policy, op, ne in (("h2o_head", "max", T // 2), ("tova", "avg", T - 64)):
        refs = _reference(d, T, obs, policy, ne, ks, op)
        assert R.meets_cap(refs[0]["rank"][0], ne, SINK, obs)
        bank = KVBank(1, 1, 1, 64, cap=T + 8)
        bank.load_rows(d["k0"].cuda(), d["v0"].cuda())
        bank.state_init(T, 2, obs)
        plan = StepPlan(policy=policy, phase="prefill", accumulate=True, evict=True, budget=T, recent=obs, sink=SINK, stride=obs, n_evict=ne,
                        pool=ks, pool_op=op)
        out, ids = bank.attend(plan, d["q"].cuda(), d["k"].cuda(), d["v"].cuda())

        def victims(l, h, v):
            assert R.valid(v, refs[l]["rank"][h], ne, SINK, obs), (policy, sorted(set(v.tolist()) ^ set(refs[l]["ids"][h].tolist()))[:20])
        _check_step(bank, d, refs, out, ids, T, obs, ne, policy, ("scratch", policy), victims)


@gpu
def test_refusal_just_past_the_pooled_width_leaves_the_bank_untouched():
    """The widest pooled row is the generic scorer's: 4 W + 8 rows + 10 272 bytes of LDS for the keys of the scratch build, at most 160 KB:
    W <= 38 376 at 8 logits rows.  38 368 columns plan; 38 400 are refused before anything is launched, with zero workspace bytes."""
    from easykv_amd import KVBank, StepPlan
    from easykv_amd._lib import EkvError
    obs = 8
    bank = KVBank(1, 1, 1, 64, cap=38464)
    z = torch.zeros(1, 1, 38360, 64, dtype=torch.float16, device="cuda")
    bank.load_rows(z, z)
    bank.state_init(38368, 2, obs)
    plan = StepPlan(policy="h2o_head", phase="prefill", accumulate=True, evict=True, budget=38368, recent=obs, sink=SINK, stride=obs, n_evict=20000,
                    pool=7, pool_op="max")
    st = bank.make_step(plan, obs, 0, 1)
    fam = bank._family(plan)
    assert bank._step_check(st, fam) == 0 and bank._step_ws_bytes(st, fam) > 0 and bank.step_info(plan, obs)["n_launches"] >= 2
    bank.load_rows(z[:, :, :32], z[:, :, :32])
    st = bank.make_step(plan, obs, 0, 1)
    assert st.n_slots == 38400 and bank._step_check(st, fam) == -2 and bank._step_ws_bytes(st, fam) == 0
    info = bank.step_info(plan, obs)
    assert info["n_launches"] == 0 and info["fused"] == 0
    before = (list(bank.n_slots), list(bank.extent), bank.slot_of_pos.clone(), bank.score_sum.clone())
    q = torch.zeros(1, 1, obs, 64, dtype=torch.float16, device="cuda")
    with pytest.raises(EkvError, match="unsupported"):
        bank.attend(plan, q, q, q)
    assert (list(bank.n_slots), list(bank.extent)) == before[:2] and torch.equal(bank.slot_of_pos, before[2]) and torch.equal(bank.score_sum, before[3])


@gpu
def test_pool_one_is_the_plain_call_bit_for_bit():
    from easykv_amd import KVBank, StepPlan, _lib
    obs, T, ne = 8, 300, 150
    d = _data("d128_gqa2", "f16", T, obs, 72003)
    banks = [KVBank(d["L"], d["Hq"], d["H"], d["D"], cap=T + 8) for _ in range(2)]
    for b in banks:
        b.load_rows(d["k0"].cuda(), d["v0"].cuda())
        b.state_init(T, 2, obs)
    # kernel size 1 has no pooled call: radius 0 is an argument error of ekv_pool_*
    st = banks[0].make_step(StepPlan(policy="h2o_head", phase="prefill", evict=True, budget=T, recent=obs, sink=SINK, stride=obs, n_evict=ne), obs, 0, 2)
    for radius, op, want in ((0, 0, -1), (1, 0, 0), (1, 2, -1)):
        assert banks[0].lib.ekv_pool_step_check(ctypes.byref(banks[0]._bank), ctypes.byref(st), 0, ctypes.byref(_lib.Pool(radius, op))) == want
    old = dict(policy="h2o_head", phase="prefill", accumulate=True, evict=True, budget=T, recent=obs, sink=SINK, stride=ne)
    # (the twin is stepped without the new fields: `stride` victims, as before; its count arithmetic reads the stride, so compare h2o_head's rows)
    new = dict(old, stride=ne, n_evict=ne, pool=1, pool_op="avg")
    assert banks[0].step_info(StepPlan(**old), obs) == banks[1].step_info(StepPlan(**new), obs)
    (o0, i0), (o1, i1) = banks[0].attend(StepPlan(**old), d["q"].cuda(), d["k"].cuda(), d["v"].cuda()), \
        banks[1].attend(StepPlan(**new), d["q"].cuda(), d["k"].cuda(), d["v"].cuda())
    assert torch.equal(o0, o1) and torch.equal(i0, i1)
    for name in ("slot_of_pos", "score_sum", "score_sq", "score_cnt"):
        assert torch.equal(getattr(banks[0], name), getattr(banks[1], name)), name


# ---- (e) the unpooled one-shot step with roco ------------------------------------------------------------------------------------------
def _roco_rows(st, T, obs):
    from oracle import easykv_oracle as O
    return O.roco_std(st.s, st.q, st.c, SINK), st.s / st.c


def _roco_gaps(std_row, mean_row, k1, k):
    """Relative gaps at the two cuts of the reference's decision: the k1-th / (k1 + 1)-th smallest std, the k-th / (k + 1)-th smallest mean
    of the feasible set.  A decision whose gaps are far above the kernels' 1e-6 is the same on both sides."""
    std = torch.where(torch.isnan(std_row), torch.full_like(std_row, float("inf")), std_row).double()
    order = torch.argsort(std, stable=True)
    lo, hi = std[order[k1 - 1]], std[order[k1]]
    # (a cut among the 1e9 sentinels of the sink and the tail is an exact tie, which the class rule of tests/select_rule.py covers: the
    # means are then ranked over every column that may be feasible)
    gap_std = float("inf") if float(lo) >= 1e9 else float((hi - lo) / lo)
    feas = order[:k1] if float(lo) < 1e9 else torch.nonzero(std <= lo).flatten()
    m = torch.sort(mean_row.double()[feas])[0]
    return gap_std, float((m[k] - m[k - 1]) / m[k - 1].abs())


ROCO_CASES = [("d128_gqa2", 300, 8, 1, 73002), ("d64_gqa8", 300, 8, 1, 73001), ("d128_gqa2", 1500, 32, 2, 73000)]


@pytest.mark.parametrize("shape,T,obs,n_split,seed", ROCO_CASES, ids=[f"{c[0]}-T{c[1]}" for c in ROCO_CASES])
def test_roco_reference_decisions_are_well_separated(shape, T, obs, n_split, seed):
    """Not a GPU test: at the seeds of (e) both cuts of the reference's roco decision have a relative gap above 1e-4 in every row."""
    ne, k1 = T - 64, T - obs - SINK
    for ref in _reference(_data(shape, "f16", T, obs, seed), T, obs, "roco", ne, 1, "max"):
        std, mean = _roco_rows(ref["st"], T, obs)
        for h in range(std.shape[0]):
            gaps = _roco_gaps(std[h], mean[h], k1, ne)
            assert min(gaps) > 1e-4, (h, gaps)


@gpu
@pytest.mark.parametrize("shape,T,obs,n_split,seed", ROCO_CASES, ids=[f"{c[0]}-T{c[1]}" for c in ROCO_CASES])
def test_unpooled_one_shot_step_with_roco_takes_many_victims(shape, T, obs, n_split, seed):
    """n_evict = T - 64 at q_len = 8 / 32 through whatever scorer the plain call plans (the logits-resident kernel's tail, the wide
    column-sum pass's tail, the generic scorer): the reference's `_select_prefill` with k = n_evict under the class rule."""
    from easykv_amd import KVBank, StepPlan
    from tests.select_rule import feasible_classes, valid_victims
    ne, k1 = T - 64, T - obs - SINK
    d = _data(shape, "f16", T, obs, seed)
    refs = _reference(d, T, obs, "roco", ne, 1, "max")
    bank = KVBank(d["L"], d["Hq"], d["H"], d["D"], cap=T + 8)
    bank.load_rows(d["k0"].cuda(), d["v0"].cuda())
    bank.state_init(T, 2, obs)
    plan = StepPlan(policy="roco", phase="prefill", accumulate=True, evict=True, budget=T, recent=obs, sink=SINK, stride=obs, n_evict=ne, n_split=n_split)
    info = bank.step_info(plan, obs)
    print(f"[oneshot] roco {shape} T = {T}: {info}")
    st = bank.make_step(plan, obs, 0, d["L"])
    assert (st.n_evict, st.roco_k1) == (ne, k1)
    out, ids = bank.attend(plan, d["q"].cuda(), d["k"].cuda(), d["v"].cuda())

    def victims(l, h, v):
        std, mean = _roco_rows(refs[l]["st"], T, obs)
        forced, pool, need = feasible_classes(std[h], k1)
        assert valid_victims(v.tolist(), mean[h], forced, pool, need, ne), (shape, l, h, sorted(set(v.tolist()) ^ set(refs[l]["ids"][h].tolist()))[:20])
    _check_step(bank, d, refs, out, ids, T, obs, ne, "roco", ("roco", shape, T), victims)


# ---- (f) the hand-over --------------------------------------------------------------------------------------------------------------------
@gpu
def test_hand_over_leaves_a_decode_sized_bank_in_logical_order():
    from easykv_amd import KVBank, StepPlan
    from tests.test_hip_d256 import _permutation
    obs, T, B = 8, 300, 80
    d = _data("d128_gqa2", "f16", T, obs, 74001)
    bank = KVBank(d["L"], d["Hq"], d["H"], d["D"], cap=T + 8)
    bank.load_rows(d["k0"].cuda(), d["v0"].cuda())
    bank.state_init(T, 2, obs)
    plan = StepPlan(policy="h2o_head", phase="prefill", accumulate=True, evict=True, budget=T, recent=obs, sink=SINK, stride=obs, n_evict=T - B,
                    pool=7, pool_op="max")
    bank.attend(plan, d["q"].cuda(), d["k"].cuda(), d["v"].cuda())
    assert bank.n_slots == [B] * 2 and bank.extent == [T] * 2
    k_ord, v_ord = bank.ordered_kv()
    new = bank.hand_over(B + 40)
    assert new.cap == 128 and new.n_slots == [B] * 2 and new.extent == [B] * 2 and new.dtype == bank.dtype
    assert torch.equal(new.k[:, :, :B], k_ord) and torch.equal(new.v[:, :, :B], v_ord)      # logical order in the physical rows [0, B)
    assert torch.equal(new.slot_of_pos[:, :, :B].cpu(), torch.arange(B, dtype=torch.int32).expand(2, d["H"], B))
    _permutation(new)
    for name in ("score_sum", "score_sq", "score_cnt"):
        assert torch.equal(getattr(new, name)[:, :, :B], getattr(bank, name)[:, :, :B]), name
        assert not bool(getattr(new, name)[:, :, B:].any()), name
    # the next decode step: as on a bank that was loaded with the same rows directly
    twin = KVBank(d["L"], d["Hq"], d["H"], d["D"], cap=B + 40)
    twin.load_rows(k_ord, v_ord)
    for name in ("score_sum", "score_sq", "score_cnt"):
        getattr(twin, name)[:, :, :B].copy_(getattr(bank, name)[:, :, :B])
    g = torch.Generator().manual_seed(74002)
    for step in range(3):
        q, k, v = (_mk(2, h, 1, g, d["D"], torch.float16).cuda() for h in (d["Hq"], d["H"], d["H"]))
        dec = StepPlan(policy="h2o_head", phase="decode", accumulate=True, evict=True, score_off=0, budget=B)
        assert new.step_info(dec, 1) == twin.step_info(dec, 1)
        (o0, i0), (o1, i1) = new.attend(dec, q, k, v), twin.attend(dec, q, k, v)
        assert torch.equal(o0, o1) and torch.equal(i0, i1), step
    assert new.extent == twin.extent == [B + 1] * 2
    # a window bank carries the rows' token positions and the tokens seen
    win = KVBank(2, 8, 2, 64, cap=T + 8, sinks=torch.zeros(2, 8), windows=[16, 0])
    dw = _data("d64_gqa8", "f16", T, obs, 74003)
    win.load_rows(dw["k0"].cuda(), dw["v0"].cuda())
    win.state_init(T, 2, obs)
    wplan = StepPlan(policy="h2o_head", phase="prefill", accumulate=True, evict=True, budget=T, recent=obs, sink=SINK, stride=obs, n_evict=T - B)
    win.attend(wplan, dw["q"][:, :8].cuda(), dw["k"].cuda(), dw["v"].cuda())
    pos = win.ordered_tok_pos()
    new = win.hand_over(B + 40)
    assert new.windows == win.windows and new.tokens_seen == T and torch.equal(new.ordered_tok_pos(), pos)
    assert torch.equal(new.tok_pos[:, :, :B], pos) and torch.equal(new.sinks, win.sinks) and new.extent == [B] * 2


# ---- (g) generate ---------------------------------------------------------------------------------------------------------------------------
def _ids(length):
    return torch.arange(length).view(1, -1) % 16


GEN_CASES = [("encoding", "h2o_head", 7, "max"), ("auto", "tova", 3, "avg"), ("auto", "roco", 1, "max"), ("encoding", "roco", 1, "max")]


@gpu
@pytest.mark.parametrize("mode,policy,pool,op", GEN_CASES, ids=[f"{c[0]}-{c[1]}-{c[2]}" for c in GEN_CASES])
def test_generate_with_the_key_against_the_test_side_driver(mode, policy, pool, op):
    import easykv_amd
    from oracle import easykv_oracle as O
    from oracle.fake_model import make_streams
    from tests.native_fake_model import NativeFakeModel
    from tests.select_rule import feasible_classes, valid_victims
    from tests.test_hip_fullsize import Probe
    n, B, obs, m, L, Hq, H, D = 200, 80, 16, 6, 2, 8, 2, 64
    cfg = dict(budget=B, kv_policy=policy, max_new_tokens=m, prefill="one_shot", obs_window=obs, score_pool=pool, score_pool_op=op)
    streams = make_streams(L, Hq, H, D, n + m + 8, seed=75)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        res, cache = easykv_amd.generate(NativeFakeModel(*streams), _ids(n), dict(cfg, _record_evictions=True), kv_mode=mode, stride=4, return_cache=True)
    ev = [torch.stack(e).cpu().long() for e in cache.evictions]      # per evicting forward: [L, H, k]
    assert ev[0].shape == (L, H, n - B) and len(ev) == 1 + (m if mode == "auto" else 0)
    _, idx, _ = easykv_amd.geometry(mode, n, B, 4)
    assert cache.bank.cap == ((idx + 4 + (m if mode == "encoding" else 1) + 8) + 63) // 64 * 64
    assert max(cache.bank.extent) <= B + m      # the decode steps stream the budget's rows, not the prompt's

    def follow(l, ids_ref, rank):
        ours = ev[0][l]
        for h in range(H):
            if policy == "roco":
                st = follow.state[l]
                std, mean = O.roco_std(st.s, st.q, st.c, SINK), st.s / st.c
                forced, pl, need = feasible_classes(std[h], n - obs - SINK)
                assert valid_victims(ours[h].tolist(), mean[h], forced, pl, need, n - B), (l, h)
            else:
                assert R.meets_cap(rank[h], n - B, SINK, obs) and R.valid(ours[h], rank[h], n - B, SINK, obs), (l, h)
        return torch.sort(ours, dim=-1)[0]
    probe, alive, stats = Probe(), torch.ones(L, H, dtype=torch.bool), [0, 0]

    def on_decode(l, i, ids_ref):
        ok = ~probe.last_unstable
        same = ev[1 + i][l, :, 0] == ids_ref[:, 0]
        assert bool(same[ok & alive[l]].all()), (l, i, ev[1 + i][l, :, 0].tolist(), ids_ref[:, 0].tolist())
        stats[0] += int((ok & alive[l]).sum())
        stats[1] += H
        alive[l] &= ok & same
    if policy == "roco":      # (the class rule of roco needs the accumulated rows: observe them through the reference's own state)
        follow.state = {}
        real = R.observation_step

        def spy(st, *a, **kw):
            out = real(st, *a, **kw)
            follow.state[len(follow.state)] = st
            return out
        R.observation_step = spy
    O.SELECT_HOOK = probe
    try:
        ref = R.generate(*streams, n, cfg, mode, follow=follow, on_decode=on_decode)
    finally:
        O.SELECT_HOOK = None
        if policy == "roco":
            R.observation_step = real
    assert res == ref["tokens"] and buf.getvalue().strip() == ref["printed"], (res, ref["tokens"], buf.getvalue(), ref["printed"])
    assert cache.get_seq_length() == (B + m if mode == "encoding" else B)
    if mode == "auto":
        print(f"[oneshot] generate auto {policy}: compared {stats[0]} of {stats[1]} decode decisions")
        assert 2 * stats[0] >= stats[1]
    # the retained rows are the rows of the retained positions (heads that never left the probe's class)
    kk, _ = cache.bank.ordered_kv()
    for l in range(L):
        for h in range(H):
            if bool(alive[l, h]):
                assert torch.equal(kk[l, h].cpu(), streams[1][l][h][ref["positions"][l][h]]), (l, h)


class _Tok:
    eos_token_id = -1

    def decode(self, ids, skip_special_tokens=True):
        return " ".join(str(i) for i in ids)


@gpu
def test_stock_tiny_llama_with_the_key():
    """The first generated token comes from the prompt's last-token logits, which forwards A + B compute densely: the model's own greedy
    token (any other only where the model's top-2 margin is below the seam's bar of 3e-2)."""
    import easykv_amd
    from easykv_amd import hf
    from tests.test_hip_hf_adapter import _tiny
    model = _tiny(3)
    ids = torch.randint(0, 97, (1, 150), device="cuda", generator=torch.Generator("cuda").manual_seed(7))
    with torch.inference_mode():
        top2 = torch.topk(model(input_ids=ids).logits[0, -1].float(), 2)
    hf.patch_model(model)
    for mode, policy, pool, stride in (("encoding", "h2o_head", 7, 8), ("auto", "tova", 3, 8)):
        easykv_amd.enable_fixed_kv(model, _Tok(), mode=mode, stride=stride)
        gc = dict(budget=64, kv_policy=policy, max_new_tokens=5, eos_token_ids=[-1], temperature=1e-6, prefill="one_shot", obs_window=16,
                  score_pool=pool)
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            out, cache = model.easykv_generate(input_ids=ids, generation_config=gc, return_cache=True)
        assert len(out.split()) == 5 and cache.get_seq_length() == (64 + 5 if mode == "encoding" else 64) and max(cache.bank.extent) <= 64 + 5
        assert int(out.split()[0]) == int(top2.indices[0]) or float(top2.values[0] - top2.values[1]) < 3e-2, (out, top2)
        want = "KV cache budget ratio: 42.67%(64/150)" if mode == "encoding" else "KV Cache Budget ratio 41.29%[64/(150+5)]"
        assert want in buf.getvalue(), buf.getvalue()


@gpu
def test_tiny_sink_and_window_gpt_oss_with_an_unpooled_observation_step():
    """score_pool = 1 makes no new call: the observation step runs through the model's own family (sinks + windows)."""
    import easykv_amd
    from easykv_amd import hf
    from tests.test_hip_sink import _tiny_gpt_oss
    model = _tiny_gpt_oss(2).cuda()      # (sliding_window 256 on its first layer: the window family's kernels, no key masked at 125 tokens)
    ids = torch.randint(0, 97, (1, 120), device="cuda", generator=torch.Generator("cuda").manual_seed(8))
    with torch.inference_mode():
        top2 = torch.topk(model(input_ids=ids).logits[0, -1].float(), 2)
    hf.patch_model(model)
    easykv_amd.enable_fixed_kv(model, _Tok(), mode="auto", stride=8)
    gc = dict(budget=60, kv_policy="roco", max_new_tokens=5, eos_token_ids=[-1], temperature=1e-6, sliding_window="model", prefill="one_shot",
              obs_window=16, score_pool=1)
    with contextlib.redirect_stdout(io.StringIO()):
        out, cache = model.easykv_generate(input_ids=ids, generation_config=gc, return_cache=True)
    assert cache.windows == (256, 0) and cache.sinks is not None and cache.bank.tokens_seen == 125
    assert len(out.split()) == 5 and cache.get_seq_length() == 60 and max(cache.bank.extent) <= 61
    assert int(out.split()[0]) == int(top2.indices[0]) or float(top2.values[0] - top2.values[1]) < 3e-2, (out, top2)
    pos = cache.bank.ordered_tok_pos().cpu()
    assert bool((pos[:, :, 1:] > pos[:, :, :-1]).all()) and int(pos.max()) == 124
    with pytest.raises(ValueError, match="no pooled sink, window, capped or"):
        model.easykv_generate(input_ids=ids, generation_config=dict(gc, kv_policy="tova", score_pool=3))


# ---- (h) generate_batch ---------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("mode,policy,pool", [("encoding", "h2o_head", 7), ("auto", "tova", 3)], ids=["encoding", "auto"])
def test_generate_batch_with_the_key_equals_the_solo_runs(mode, policy, pool):
    from oracle.fake_model import make_streams
    from tests.test_hip_generate_batch import _evictions, _run_batch, _run_solo
    lengths, m = (150, 200, 96), 5
    cfg = dict(budget=64, kv_policy=policy, max_new_tokens=m, prefill="one_shot", obs_window=16, score_pool=pool, _record_evictions=True)
    streams = make_streams(2, 8, 2, 64, max(lengths) + m + 8, seed=76)
    model, res, cache, lines = _run_batch(streams, cfg, mode, 4, lengths)
    assert len(res) == len(lines) == len(lengths)
    for i, n in enumerate(lengths):
        smodel, sres, scache, sline = _run_solo(streams, cfg, mode, 4, n)
        assert res[i] == sres and lines[i] == sline, (i, n, res[i], sres, lines[i], sline)
        ours, solo = _evictions(cache.evictions[i]), _evictions(scache.evictions)
        assert len(ours) == len(solo) == 1 + (m if mode == "auto" else 0) and ours[0].shape[-1] == n - 64
        assert all(np.array_equal(a, b) for a, b in zip(ours, solo)), (i, n)
        assert cache.bat.n_slots(i) == scache.get_seq_length()
