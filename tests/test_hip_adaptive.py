"""Adaptive head budgets on the GPU (include/easykv_hip.h, "adaptive head budgets") against tests/adaptive_ref.py.

(a) One observation step against the reference: L = 2, n = 300, obs = 8, sink = 2, keep 64 per head on average; 4 KV heads of head_dim 128
    (rep 1) and 2 KV heads of head_dim 64 (rep 4); fp16 and bf16; h2o_head and tova; radius 0 and 3; max and avg.  The queries of a KV
    head are scaled (x8, x1, x0.25, x0.05): a peaked head's candidates are nearly all tiny and leave first, a flat head's stay.  With four
    heads every layer of the reference has a head at the floor of its keep (evict_max victims), one at the ceiling (evict_min) and one
    strictly between (the seeds are picked for that); with two heads and these bounds both ends cannot be reached at once (280 + 182 <
    2 * 236 < 280 + 280: one head at a bound puts the other strictly inside), so there the heads' counts must differ.
    test_reference_layers_meet_the_cap checks all of that, and the class's cap, without a GPU.
(b) Degenerate bounds (evict_min = evict_max = n_evict): the pooled call bit for bit; with radius 0 the plain call.
(c) Ties: hand-made score rows with equal values across heads at the layer's threshold, ranked as they are (accumulate off, radius 0):
    the counts and the victims are the (key, head, j) rule's, exactly.
(d) Rows past one CU's LDS (n = 12 000, the scratch build of the scorer) against the reference.
(e) The view: decode steps of a bank whose heads differ, served by the batched call on the bank seen as L * H one-head layers.  With
    uniform lengths out, victims, slot map and score rows equal the ordinary single-sequence step bit for bit (n_split 1 and 3); with
    ragged lengths (40 / 64 / 97 / 128) every head is compared with the single-sequence step on a one-head twin bank; then the
    hand-over of a ragged bank.
(f) The driver (generation_config['head_budgets'] = 'adaptive') over the fake model of tests/native_fake_model.py, `encoding` and `auto`
    mode, against adaptive_ref.generate following the device's victims once they are held to the class: tokens, printed line, retained
    positions per head, the mean retained count per layer.
(g) A tiny stock Llama through hf.patch_model: adaptive and uniform runs complete, both retain H * B rows per layer, the heads differ.
(e') evict_ids: a step that wants none back still hands the scorer [L][H][evict_max]; a caller's tensor of another shape is refused;
    layer-by-layer steps work and only the stepped layers refuse a further step."""
import math

import pytest
import torch

from tests import adaptive_ref as A
from tests import oneshot_ref as R
from tests.golden_util import out_close
from tests.test_hip_oneshot import _bf16_close, _mk

gpu = pytest.mark.gpu
BF = torch.bfloat16
SINK, OBS, N, KEEP, L = 2, 8, 300, 64, 2
SHAPES = {"h4_d128": (128, 4, 4), "h2_d64_gqa4": (64, 8, 2)}      # head_dim, query heads, KV heads
SCALES = {4: (8.0, 1.0, 0.25, 0.05), 2: (8.0, 0.05)}
CASES = [(s, dt, pol, r, op) for s in SHAPES for dt in ("f16", "bf16") for pol in ("h2o_head", "tova") for r in (0, 3) for op in ("max", "avg")]
IDS = ["-".join(str(x) for x in c) for c in CASES]


def bounds(n, obs, sink, keep, floor=0.2, ceil=2.0):
    """(n_evict, evict_min, evict_max) of a prompt of n tokens kept to `keep` rows per head on average: the driver's rule, fractions of the
    uniform candidate keep K = C - n_evict."""
    C, n_evict = n - obs - sink, n - keep
    K = C - n_evict
    return n_evict, max(0, C - math.ceil(ceil * K)), C - math.floor(floor * K)


def _data(shape, dt, seed, n=N, layers=L):
    D, Hq, H = SHAPES[shape]
    dtype = BF if dt == "bf16" else torch.float16
    g = torch.Generator().manual_seed(seed)
    d = dict(D=D, Hq=Hq, H=H, L=layers, dtype=dtype, k0=_mk(layers, H, n - OBS, g, D, dtype), v0=_mk(layers, H, n - OBS, g, D, dtype),
             q=_mk(layers, Hq, OBS, g, D, dtype), k=_mk(layers, H, OBS, g, D, dtype), v=_mk(layers, H, OBS, g, D, dtype))
    scale = torch.tensor(SCALES[H]).repeat_interleave(Hq // H).reshape(1, Hq, 1, 1)
    d["q"] = (d["q"].float() * scale).to(dtype)
    return d


def _reference(d, n, policy, ne, lo, hi, pool, op):
    from oracle import easykv_oracle as O
    out = []
    for l in range(d["L"]):
        st = O.LayerState(k=d["k0"][l:l + 1].float(), v=d["v0"][l:l + 1].float())
        st.s, st.q, st.c = O.init_state_prefill((d["H"],), n - OBS, OBS, False)
        qf, kf, vf = d["q"][l:l + 1].float(), d["k"][l:l + 1].float(), d["v"][l:l + 1].float()
        o, k, victims, rank = A.observation_step(st, qf, kf, vf, policy, ne, lo, hi, SINK, pool, op)
        pv = O.attention_core(qf, st.k, st.v.abs(), O.causal_chunk_mask(OBS, n, qf.dtype))[0][0] if d["dtype"] is BF else None
        out.append(dict(o=o[0], k=k, victims=victims, rank=rank, st=st, pv=pv))
    return out


# per (policy, radius, op): the first seed from 81000 at which every layer of the four-head reference has its three kinds of head
SEEDS = {("h2o_head", 0, "max"): 81020, ("h2o_head", 0, "avg"): 81020, ("h2o_head", 3, "max"): 81009, ("h2o_head", 3, "avg"): 81000,
         ("tova", 0, "max"): 81022, ("tova", 0, "avg"): 81022, ("tova", 3, "max"): 81000, ("tova", 3, "avg"): 81001}


def _seed(case):
    return SEEDS[case[2:]]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_reference_layers_meet_the_cap(case):
    """Not a GPU test: the reference alone on the inputs of (a)."""
    shape, dt, policy, radius, op = case
    ne, lo, hi = bounds(N, OBS, SINK, KEEP)
    assert (ne, lo, hi) == (236, 182, 280)
    for ref in _reference(_data(shape, dt, _seed(case)), N, policy, ne, lo, hi, 2 * radius + 1, op):
        k = ref["k"]
        assert sum(k) == len(k) * ne and all(lo <= x <= hi for x in k), k
        assert A.meets_cap(ref["rank"], ne, lo, hi, SINK, OBS), (case, k)
        assert A.valid(ref["victims"], ref["rank"], ne, lo, hi, SINK, OBS), case
        if len(k) == 4:
            assert hi in k and lo in k and any(lo < x < hi for x in k), (case, k)
        else:
            assert k[0] != k[1], (case, k)


def _bank(d, n, cap=None):
    from easykv_amd import KVBank
    bank = KVBank(d["L"], d["Hq"], d["H"], d["D"], cap=cap or n + 8, dtype=d["dtype"])
    bank.load_rows(d["k0"].cuda(), d["v0"].cuda())
    bank.state_init(n, 2, OBS)
    return bank


def _plan(policy, n, ne, pool, op, adaptive, **kw):
    from easykv_amd import StepPlan
    return StepPlan(policy=policy, phase="prefill", accumulate=True, evict=True, budget=n, recent=OBS, sink=SINK, stride=OBS, n_evict=ne,
                    pool=pool, pool_op=op, head_adaptive=adaptive, **kw)


def _check_against_reference(bank, d, refs, out, ids, n, ne, lo, hi, policy, tag):
    """Counts, bounds, victims under the class, outputs; then score rows, rows (through the slot map) and lengths for the DEVICE'S victims."""
    from tests.test_hip_d256 import _permutation
    assert tuple(ids.shape) == (d["L"], d["H"], hi), (tag, ids.shape)
    ids_c = ids.cpu().long()
    kk, vv = bank.ordered_kv()
    S = bank.score_sum.cpu()
    for l, ref in enumerate(refs):
        got = out[l].float().cpu()
        close = out_close(got, ref["o"]) if d["dtype"] is not BF else _bf16_close(got, ref["o"], ref["pv"])
        assert close, (tag, l, float((got - ref["o"]).abs().max()))
        t_h = bank.head_slots[l]
        k_dev = [n - t for t in t_h]
        print(f"[adaptive] {tag} layer {l}: device k = {k_dev}, reference k = {ref['k']}")
        assert sum(k_dev) == d["H"] * ne and all(lo <= x <= hi for x in k_dev) and bank.n_slots[l] == max(t_h), (tag, l, k_dev)
        victims = []
        for h in range(d["H"]):
            v = ids_c[l, h, :k_dev[h]]
            assert bool((v[1:] > v[:-1]).all()) and bool((ids_c[l, h, k_dev[h]:] == -1).all()), (tag, l, h, "evict_ids ascend, the rest unwritten")
            victims.append(v)
        assert A.valid(victims, ref["rank"], ne, lo, hi, SINK, OBS), (tag, l, k_dev, ref["k"])
        heads = A.compact_heads(ref["st"], victims, policy)
        k_all, v_all = torch.cat((d["k0"][l], d["k"][l]), 1), torch.cat((d["v0"][l], d["v"][l]), 1)
        for h, want in enumerate(heads):
            # (the surviving columns in the reference's order; not bit-equal because the device sums a column's obs x rep probabilities in
            # fp32 in its own order and its exp is the hardware's: the bar is the project's for score rows, tests/oneshot_ref.py's RTOL / ATOL)
            assert torch.allclose(S[l, h, :n], want["s"], rtol=2e-5, atol=1e-7), (tag, l, h, "score_sum", float((S[l, h, :n] - want["s"]).abs().max()))
            keep = torch.ones(n, dtype=torch.bool)
            keep[victims[h]] = False
            assert torch.equal(kk[l, h, :t_h[h]].cpu(), k_all[h][keep]) and torch.equal(vv[l, h, :t_h[h]].cpu(), v_all[h][keep]), (tag, l, h, "rows")
    _permutation(bank)


@gpu
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_adaptive_step_against_the_reference(case):
    shape, dt, policy, radius, op = case
    ne, lo, hi = bounds(N, OBS, SINK, KEEP)
    d = _data(shape, dt, _seed(case))
    refs = _reference(d, N, policy, ne, lo, hi, 2 * radius + 1, op)
    bank = _bank(d, N)
    plan = _plan(policy, N, ne, 2 * radius + 1, op, (lo, hi))
    info = bank.step_info(plan, OBS)
    assert info["fused"] == 0 and info["n_launches"] >= 4, info      # attention, then rank + allot + select
    out, ids = bank.attend(plan, d["q"].cuda(), d["k"].cuda(), d["v"].cuda())
    _check_against_reference(bank, d, refs, out, ids, N, ne, lo, hi, policy, case)
    with pytest.raises(RuntimeError, match="different numbers of rows"):
        bank.attend(plan, d["q"].cuda(), d["k"].cuda(), d["v"].cuda())
    bank.reset()
    assert bank.head_slots is None


@gpu
@pytest.mark.parametrize("deferred", (False, True), ids=("whole", "deferred"))
@pytest.mark.parametrize("policy", ("h2o_head", "tova"))
def test_degenerate_bounds_are_the_pooled_call_bit_for_bit(policy, deferred):
    """evict_min = evict_max = n_evict: out, evict_ids, slot map and score rows of the ekv_pool_* call with no tolerance; radius 0: the plain
    call's.  Whole steps and the deferred form (three launches in the flush)."""
    ne = N - KEEP
    d = _data("h2_d64_gqa4", "f16", 82001)
    q, k, v = d["q"].cuda(), d["k"].cuda(), d["v"].cuda()
    for pool, op in ((7, "max"), (3, "avg"), (1, "max")):
        got = []
        for adaptive in (None, (ne, ne)):
            bank = _bank(d, N)
            plan = _plan(policy, N, ne, pool, op, adaptive)
            if deferred:
                outs = [bank.attend(plan, q[l:l + 1], k[l:l + 1], v[l:l + 1], layer_begin=l, defer=True)[0] for l in range(L)]
                out, ids = torch.cat(outs), bank.flush()
            else:
                out, ids = bank.attend(plan, q, k, v)
            assert bank.n_slots == [KEEP] * L and (adaptive is None or bank.head_slots == [[KEEP] * d["H"]] * L)
            got.append((out, ids, bank.slot_of_pos.clone(), bank.score_sum.clone(), bank.score_sq.clone(), bank.score_cnt.clone()))
        for a, b, name in zip(got[0], got[1], ("out", "evict_ids", "slot_of_pos", "score_sum", "score_sq", "score_cnt")):
            assert torch.equal(a, b), (policy, pool, op, name)


@gpu
def test_ties_across_heads_go_by_key_head_index():
    """Score rows of small integers, ranked as they stand: every value is shared by many columns of every head, so the layer's threshold
    falls inside a tie that spans heads and the boundaries inside ties of their own.  Exact: counts and victims equal the rule's."""
    n, H, ne, lo, hi = 200, 4, 120, 60, 170
    g = torch.Generator().manual_seed(83001)
    d = dict(D=64, Hq=4, H=H, L=2, dtype=torch.float16, k0=_mk(2, H, n - OBS, g, 64, torch.float16), v0=_mk(2, H, n - OBS, g, 64, torch.float16),
             q=_mk(2, 4, OBS, g, 64, torch.float16), k=_mk(2, H, OBS, g, 64, torch.float16), v=_mk(2, H, OBS, g, 64, torch.float16))
    rows = torch.randint(0, 6, (2, H, n), generator=g).float()
    rows[1, 1] = rows[1, 0]      # two heads with the same row: every key of one ties with the other's
    rows[0, 2, 5] = float("nan")
    for adaptive in ((lo, hi), (0, n - OBS - SINK), (ne - 1, ne + 1)):
        bank = _bank(d, n)
        bank.score_sum[:, :, :n] = rows.cuda()
        plan = _plan("h2o_head", n, ne, 1, "max", adaptive, )
        plan.accumulate = False
        out, ids = bank.attend(plan, d["q"].cuda(), d["k"].cuda(), d["v"].cuda())
        ids_c = ids.cpu().long()
        for l in range(2):
            k_ref, victims = A.allot(rows[l], ne, adaptive[0], adaptive[1], SINK, OBS)
            assert [n - t for t in bank.head_slots[l]] == k_ref, (adaptive, l, bank.head_slots[l], k_ref)
            for h in range(H):
                assert torch.equal(ids_c[l, h, :k_ref[h]], victims[h]), (adaptive, l, h)


@gpu
def test_rows_past_the_lds_row_run_on_the_scratch_path():
    n, keep = 12000, 1024
    ne, lo, hi = bounds(n, OBS, SINK, keep)
    d = _data("h2_d64_gqa4", "f16", 84001, n=n, layers=1)
    for policy, radius, op in (("h2o_head", 3, "max"), ("tova", 0, "avg")):
        refs = _reference(d, n, policy, ne, lo, hi, 2 * radius + 1, op)
        assert A.meets_cap(refs[0]["rank"], ne, lo, hi, SINK, OBS) and refs[0]["k"][0] != refs[0]["k"][1]
        bank = _bank(d, n)
        out, ids = bank.attend(_plan(policy, n, ne, 2 * radius + 1, op, (lo, hi)), d["q"].cuda(), d["k"].cuda(), d["v"].cuda())
        _check_against_reference(bank, d, refs, out, ids, n, ne, lo, hi, policy, ("scratch", policy))


@gpu
def test_evict_ids_are_sized_by_evict_max_on_every_path():
    """evict_ids=False (nothing wanted back), a caller's tensor, one layer per call: the same bank state as the whole-stack step with
    returned ids.  The scorer writes at pitch evict_max, so a buffer of n_evict entries per head would be overrun."""
    case = CASES[0]
    shape, dt, policy, radius, op = case
    ne, lo, hi = bounds(N, OBS, SINK, KEEP)
    d = _data(shape, dt, _seed(case))
    q, k, v = d["q"].cuda(), d["k"].cuda(), d["v"].cuda()
    plan = _plan(policy, N, ne, 2 * radius + 1, op, (lo, hi))
    want = _bank(d, N)
    out0, ids0 = want.attend(plan, q, k, v)
    state = lambda b: (b.head_slots, b.n_slots, b.slot_of_pos.clone(), b.score_sum.clone())
    same = lambda a, b: a[0] == b[0] and a[1] == b[1] and torch.equal(a[2], b[2]) and torch.equal(a[3], b[3])
    # nothing wanted back
    bank = _bank(d, N)
    out, ids = bank.attend(plan, q, k, v, evict_ids=False)
    assert ids is None and torch.equal(out, out0) and same(state(bank), state(want))
    # a caller's tensor: the right shape is used, any other is refused before anything runs
    bank = _bank(d, N)
    mine = torch.full((L, d["H"], hi), -1, dtype=torch.int32, device="cuda")
    for bad in (torch.empty(L, d["H"], ne, dtype=torch.int32, device="cuda"), torch.empty(L, d["H"], hi, dtype=torch.int64, device="cuda"),
                torch.empty(L, d["H"], hi, dtype=torch.int32)):
        with pytest.raises(ValueError, match="evict_max"):
            bank.attend(plan, q, k, v, evict_ids=bad)
    assert bank.head_slots is None and bank.n_slots == [N - OBS] * L
    out, ids = bank.attend(plan, q, k, v, evict_ids=mine)
    assert ids is mine and torch.equal(ids, ids0) and same(state(bank), state(want))
    # one layer per call: layer 0's raggedness does not stop layer 1's step; a stepped layer refuses a second one
    bank = _bank(d, N)
    got = [bank.attend(plan, q[l:l + 1], k[l:l + 1], v[l:l + 1], layer_begin=l) for l in range(L)]
    # (a one-layer launch may split the keys differently from the two-layer one, so the probabilities may differ in the last bit: the
    # outputs are compared closely, the counts by their sum and bounds, the ids by their form)
    assert torch.allclose(torch.cat([g[0] for g in got]).float(), out0.float(), rtol=0, atol=2e-3)
    for l in range(L):
        k_dev = [N - t for t in bank.head_slots[l]]
        assert sum(k_dev) == d["H"] * ne and all(lo <= x <= hi for x in k_dev) and bank.n_slots[l] == max(bank.head_slots[l]), (l, k_dev)
        ids_l = got[l][1].cpu()
        assert tuple(ids_l.shape) == (1, d["H"], hi)
        for h in range(d["H"]):
            assert bool((ids_l[0, h, :k_dev[h]] >= SINK).all()) and bool((ids_l[0, h, k_dev[h]:] == -1).all()), (l, h)
    with pytest.raises(RuntimeError, match="different numbers of rows"):
        bank.attend(plan, q[:1], k[:1], v[:1], layer_begin=0)


def _decode_bank(Lh, Hq, H, D, rows, k0, v0, S0, lens=None):
    """A bank holding `rows` rows per head with hand-made score rows; `lens`: the heads hold only that many (the slot map is the
    identity, so the rest of a head's rows are its free tail, as after an adaptive step and a hand-over)."""
    from easykv_amd import KVBank
    bank = KVBank(Lh, Hq, H, D, cap=rows + 8)
    bank.use_slot_rows = False
    bank.load_rows(k0.cuda(), v0.cuda())
    bank.score_sum.zero_()
    bank.score_sum[:, :, :rows] = S0.cuda()
    if lens is not None:
        bank.head_slots = [list(lens) for _ in range(Lh)]
        bank.n_slots = [max(lens)] * Lh
    return bank


@gpu
@pytest.mark.parametrize("n_split", (1, 3))
@pytest.mark.parametrize("evict", (False, True), ids=("grow", "evict"))
def test_decode_steps_over_heads_of_different_lengths(evict, n_split):
    """Three decode steps.  Exact wherever the arithmetic is the same: uniform lengths against the ordinary step at both split counts;
    ragged lengths against the one-head twin at n_split = 1, and at n_split = 3 for the longest head, whose geometry is the call's
    envelope.  A shorter head at n_split = 3 is cut into key ranges by the envelope's pitch, not by its own length, so its fp32 partial
    sums fold in another order than its twin's: there the outputs are held to the project's output bar (golden_util.out_close) and the
    score rows to the score-row bar, while the victims, the slot map and the lengths stay exact."""
    from easykv_amd import StepPlan
    Lh, Hq, H, D, rows, steps = 2, 8, 4, 128, 128, 3
    rep = Hq // H
    g = torch.Generator().manual_seed(85001)
    k0, v0 = _mk(Lh, H, rows, g, D, torch.float16), _mk(Lh, H, rows, g, D, torch.float16)
    qs, ks, vs = _mk(Lh, Hq, steps, g, D, torch.float16), _mk(Lh, H, steps, g, D, torch.float16), _mk(Lh, H, steps, g, D, torch.float16)
    S0 = torch.rand(Lh, H, rows, generator=g) + 0.5
    plan = StepPlan(policy="h2o_head", phase="decode", evict=evict, score_off=0, budget=32, n_split=n_split)
    step = lambda b, t, sl=slice(None), hs=slice(None), hq=slice(None): b.attend(
        plan, qs[sl, hq, t:t + 1].cuda().contiguous(), ks[sl, hs, t:t + 1].cuda().contiguous(), vs[sl, hs, t:t + 1].cuda().contiguous())
    # uniform lengths: the view against the ordinary step
    plain, view = _decode_bank(Lh, Hq, H, D, rows, k0, v0, S0), _decode_bank(Lh, Hq, H, D, rows, k0, v0, S0, [rows] * H)
    for t in range(steps):
        (o1, i1), (o2, i2) = step(plain, t), step(view, t)
        assert torch.equal(o1, o2) and (not evict or torch.equal(i1, i2)), ("uniform", t)
        assert view.head_slots == [[plain.n_slots[0]] * H] * Lh and view.n_slots == plain.n_slots
        for arr in ("slot_of_pos", "score_sum"):
            assert torch.equal(getattr(plain, arr), getattr(view, arr)), ("uniform", t, arr)
    # ragged lengths: every head against its one-head twin
    lens = [40, 64, 97, 128]
    Sr = S0.clone()
    for h, T in enumerate(lens):
        Sr[:, h, T:] = 0
    bank = _decode_bank(Lh, Hq, H, D, rows, k0, v0, Sr, lens)
    twins = {}
    for l in range(Lh):
        for h, T in enumerate(lens):
            tw = _decode_bank(1, rep, 1, D, rows, k0[l:l + 1, h:h + 1], v0[l:l + 1, h:h + 1], Sr[l:l + 1, h:h + 1])
            tw.n_slots = [T]
            twins[l, h] = tw
    for t in range(steps):
        out, ids = step(bank, t)
        assert (ids is None) == (not evict)
        for (l, h), tw in twins.items():
            o2, i2 = step(tw, t, slice(l, l + 1), slice(h, h + 1), slice(h * rep, (h + 1) * rep))
            exact = n_split == 1 or lens[h] == max(lens)
            got = out[l, h * rep:(h + 1) * rep]
            assert torch.equal(got, o2[0]) if exact else out_close(got, o2[0]), (t, l, h, float((got.float() - o2[0].float()).abs().max()))
            assert not evict or torch.equal(ids[l, h], i2[0, 0]), (t, l, h, "victim")
            assert bank.head_slots[l][h] == tw.n_slots[0] == lens[h] + (0 if evict else t + 1), (t, l, h)
            assert torch.equal(bank.slot_of_pos[l, h], tw.slot_of_pos[0, 0]), (t, l, h, "slot map")
            a, b = bank.score_sum[l, h], tw.score_sum[0, 0]
            assert torch.equal(a, b) if exact else torch.allclose(a, b, rtol=2e-5, atol=1e-7), (t, l, h, "score row")
        assert bank.n_slots == [max(r) for r in bank.head_slots]
    # the hand-over of a ragged bank: the longest head's count of rows per head, identity slot map, lengths and score rows carried
    new = bank.hand_over(rows + 16)
    assert new.head_slots == bank.head_slots and new.n_slots == bank.n_slots and new.head_slots is not bank.head_slots
    kk, vv = bank.ordered_kv()
    k2, v2 = new.ordered_kv()
    for l in range(Lh):
        for h in range(H):
            T = bank.head_slots[l][h]
            assert torch.equal(kk[l, h, :T], k2[l, h, :T]) and torch.equal(vv[l, h, :T], v2[l, h, :T]), (l, h)
            assert torch.equal(new.slot_of_pos[l, h].cpu(), torch.arange(new.cap, dtype=torch.int32))
            assert torch.equal(new.score_sum[l, h, :T], bank.score_sum[l, h, :T])
    o1, _ = step(bank, 0)
    o2, _ = step(new, 0)
    assert out_close(o1, o2)


def _prompt(length):
    return torch.arange(length).view(1, -1) % 16


GEN = dict(n=200, B=80, obs=16, m=6, L=2, Hq=8, H=2, D=64, sink=4, seed=77)      # (the first seed from 75 at which the heads of every reference layer differ)
GEN_CASES = [("encoding", "h2o_head", 7, "max"), ("auto", "tova", 3, "avg")]


def _gen_cfg(policy, pool, op):
    return dict(budget=GEN["B"], kv_policy=policy, max_new_tokens=GEN["m"], prefill="one_shot", obs_window=GEN["obs"], score_pool=pool,
                score_pool_op=op, head_budgets="adaptive")


@pytest.mark.parametrize("mode,policy,pool,op", GEN_CASES, ids=[f"{c[0]}-{c[1]}" for c in GEN_CASES])
def test_reference_driver_layers_meet_the_cap(mode, policy, pool, op):
    """Not a GPU test: the reference driver alone on the streams of (f): every layer is a comparison and its heads' counts differ."""
    from oracle.fake_model import make_streams
    g = GEN
    ref = A.generate(*make_streams(g["L"], g["Hq"], g["H"], g["D"], g["n"] + g["m"] + 8, seed=g["seed"]), g["n"], _gen_cfg(policy, pool, op), mode)
    ne, lo, hi = ref["bounds"]
    assert (ne, lo, hi) == (120, 60, 168)
    for l in range(g["L"]):
        assert A.meets_cap(ref["rank"][l], ne, lo, hi, g["sink"], g["obs"]), (l, ref["k"][l])
        assert sum(ref["k"][l]) == g["H"] * ne and len(set(ref["k"][l])) > 1, ref["k"][l]


@gpu
@pytest.mark.parametrize("mode,policy,pool,op", GEN_CASES, ids=[f"{c[0]}-{c[1]}" for c in GEN_CASES])
def test_generate_with_adaptive_head_budgets_against_the_test_side_driver(mode, policy, pool, op):
    import contextlib
    import io
    import easykv_amd
    from oracle import easykv_oracle as O
    from oracle.fake_model import make_streams
    from tests.native_fake_model import NativeFakeModel
    from tests.test_hip_fullsize import Probe
    g = GEN
    n, B, obs, m, Lg, H = g["n"], g["B"], g["obs"], g["m"], g["L"], g["H"]
    cfg = _gen_cfg(policy, pool, op)
    streams = make_streams(Lg, g["Hq"], H, g["D"], n + m + 8, seed=g["seed"])
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        res, cache = easykv_amd.generate(NativeFakeModel(*streams), _prompt(n), dict(cfg, _record_evictions=True), kv_mode=mode, stride=4, return_cache=True)
    ev = [torch.stack(e).cpu().long() for e in cache.evictions]      # per evicting forward: [L, H, k]
    ne, lo, hi = A.budget_bounds(n, B, obs, g["sink"])
    assert ev[0].shape == (Lg, H, hi) and len(ev) == 1 + (m if mode == "auto" else 0)
    assert max(cache.bank.extent) <= n - lo + m      # the decode steps stream at most the ceiling's rows, not the prompt's

    def follow(l, victims_ref, rank, bounds):
        ours = [ev[0][l, h][ev[0][l, h] >= 0] for h in range(H)]
        assert bounds == (ne, lo, hi) and A.meets_cap(rank, ne, lo, hi, g["sink"], obs) and A.valid(ours, rank, ne, lo, hi, g["sink"], obs), (l, [len(o) for o in ours])
        print(f"[adaptive] generate {mode} layer {l}: device k = {[len(o) for o in ours]}, reference k = {[len(v) for v in victims_ref]}")
        return ours
    probe, alive, stats = Probe(), torch.ones(Lg, H, dtype=torch.bool), [0, 0]

    def on_decode(l, i, h, ids_ref):
        ok = not bool(probe.last_unstable[0])
        same = int(ev[1 + i][l, h, 0]) == int(ids_ref[0, 0])
        assert same or not (ok and alive[l, h]), (l, i, h, int(ev[1 + i][l, h, 0]), int(ids_ref[0, 0]))
        stats[0] += int(ok and bool(alive[l, h]))
        stats[1] += 1
        alive[l, h] &= ok and same
    O.SELECT_HOOK = probe
    try:
        ref = A.generate(*streams, n, cfg, mode, follow=follow, on_decode=on_decode)
    finally:
        O.SELECT_HOOK = None
    assert res == ref["tokens"] and buf.getvalue().strip() == ref["printed"], (res, ref["tokens"], buf.getvalue(), ref["printed"])
    grown = m if mode == "encoding" else 0
    assert cache.get_seq_length() == B + grown
    for l in range(Lg):      # the mean retained count of a layer is the budget's; the heads differ
        assert sum(cache.bank.head_slots[l]) == H * (B + grown) and len(set(cache.bank.head_slots[l])) > 1, cache.bank.head_slots[l]
        assert cache.bank.head_slots[l] == [len(p) for p in ref["positions"][l]]
    if mode == "auto":
        assert all(bool((e >= 0).all()) and e.shape == (Lg, H, 1) for e in ev[1:])      # every head gives one row per step: every T_h stays put
        print(f"[adaptive] generate auto {policy}: compared {stats[0]} of {stats[1]} decode decisions")
        assert 2 * stats[0] >= stats[1]
    kk, _ = cache.bank.ordered_kv()
    for l in range(Lg):
        for h in range(H):
            if bool(alive[l, h]):
                pos = ref["positions"][l][h]
                assert torch.equal(kk[l, h, :len(pos)].cpu(), streams[1][l][h][pos]), (l, h)


@gpu
def test_stock_tiny_llama_with_adaptive_head_budgets():
    import contextlib
    import io
    import easykv_amd
    from easykv_amd import hf
    from tests.test_hip_hf_adapter import _tiny
    from tests.test_hip_oneshot import _Tok
    model = _tiny(3)
    ids = torch.randint(0, 97, (1, 150), device="cuda", generator=torch.Generator("cuda").manual_seed(7))
    hf.patch_model(model)
    for mode, policy, pool in (("encoding", "h2o_head", 7), ("auto", "tova", 3)):
        easykv_amd.enable_fixed_kv(model, _Tok(), mode=mode, stride=8)
        lens = {}
        for key in (None, "adaptive"):
            gc = dict(budget=64, kv_policy=policy, max_new_tokens=5, eos_token_ids=[-1], temperature=1e-6, prefill="one_shot", obs_window=16,
                      score_pool=pool, **({} if key is None else dict(head_budgets=key)))
            buf = io.StringIO()
            with contextlib.redirect_stdout(buf):
                out, cache = model.easykv_generate(input_ids=ids, generation_config=gc, return_cache=True)
            grown = 5 if mode == "encoding" else 0
            assert len(out.split()) == 5 and cache.get_seq_length() == 64 + grown, (mode, key, out)
            want = "KV cache budget ratio: 42.67%(64/150)" if mode == "encoding" else "KV Cache Budget ratio 41.29%[64/(150+5)]"
            assert want in buf.getvalue(), buf.getvalue()
            H = cache.bank.n_kv_heads
            lens[key] = [cache.bank.head_slots[l] if cache.bank.head_slots is not None else [cache.bank.n_slots[l]] * H for l in range(cache.bank.n_layers)]
        for l, (uni, ada) in enumerate(zip(lens[None], lens["adaptive"])):      # both retain H * B rows per layer
            assert sum(uni) == sum(ada) == len(uni) * (64 + grown), (mode, l, uni, ada)
        assert any(len(set(ada)) > 1 for ada in lens["adaptive"]), (mode, lens["adaptive"])
