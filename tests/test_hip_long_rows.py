"""The long-row scorer on the GPU (KVBank(long_rows=True); include/easykv_hip.h, "long score rows").

(a) Bit identity with the generic scorer: twin banks, long_rows=False and True, same rows and inputs; after every step out, evict_ids,
    slot_of_pos, score_sum, score_sq and score_cnt are torch.equal — no tolerance: the arithmetic contract and the exact selection of
    ekv_score_long.inc make them equal.  Shapes: the smallest at which the plain plan ends in the generic scorer.
(b) Beyond the old limit (W = 40 000, just past the 38 392 columns one CU's LDS holds as keys, and 65 600, past 16-bit indices) against
    the oracle, by the protocol of tests/test_hip_fullsize.py::test_wide_score_rows_beyond_one_cus_lds — with every decision checked:
    the seeds are chosen so that the oracle's own stability probe calls all 5 * H decisions of a case well defined (see CASES_B).
    The same first step on a long_rows=False bank is refused.
(c) The driver: generate(long_rows=True) against long_rows=False on the fake model, decode caches beyond 6144 slots."""
import contextlib
import io

import pytest
import torch

from tests.golden_util import out_close
from tests.test_hip_fullsize import Probe, _check_permutation

pytestmark = pytest.mark.gpu

STATE = ("slot_of_pos", "score_sum", "score_sq", "score_cnt")


def _twins(L, hq, h, d, cap, dtype=torch.float16):
    from easykv_amd import KVBank
    return KVBank(L, hq, h, d, cap=cap, dtype=dtype), KVBank(L, hq, h, d, cap=cap, dtype=dtype, long_rows=True)


def _same_state(plain, long, what):
    for name in STATE:
        assert torch.equal(getattr(plain, name), getattr(long, name)), (what, name)
    assert plain.n_slots == long.n_slots and plain.extent == long.extent, what


def _ends_in_the_two_scorers(plain, long, plan, n, **kw):
    """The plain plan ends in the generic scorer's launch, the long plan in the long-row scorer (info field 10) with one or two launches more."""
    ip, il = plain.step_info(plan, n, **kw), long.step_info(plan, n, **kw)
    assert "long_scorer" not in ip and il["long_scorer"] == 1 and il["long_tiles"] >= 1, (ip, il)
    assert not ip["fused"] and not il["fused"] and il["n_launches"] - ip["n_launches"] in (1, 2), (ip, il)
    assert all(ip[k] == il[k] for k in ("n_split", "two_pass", "wide", "n_qblocks", "qb_rows", "n_col_parts", "fold_in_kernel")), (ip, il)
    return ip, il


def _step_both(plain, long, plan, q, k, v, what, **kw):
    (o_p, i_p), (o_l, i_l) = plain.attend(plan, q, k, v, **kw), long.attend(plan, q, k, v, **kw)
    assert torch.equal(o_p.view(torch.int16), o_l.view(torch.int16)), what
    assert (i_p is None) == (i_l is None) and (i_p is None or torch.equal(i_p, i_l)), what
    _same_state(plain, long, what)
    return o_p, i_p


def _warm(banks, T, g):
    """The same warm score state on both banks (a cold one has thousands of exact ties at zero: legal, but a dull selection)."""
    L, H = banks[0].n_layers, banks[0].n_kv_heads
    warm = torch.rand(L, H, T, generator=g) * 1e-3
    for b in banks:
        b.score_sum[:, :, :T] += warm.cuda()
        b.score_sq[:, :, :T] += (warm ** 2).cuda()


# ---- (a) bit identity ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("policy", ["roco", "h2o_head", "tova"])
@pytest.mark.parametrize("hq,dtype", [(2, torch.float16), (4, torch.float16), (2, torch.bfloat16)], ids=["gqa1", "gqa2", "gqa1-bf16"])
def test_split_decode_steps_equal_the_generic_scorer_bit_for_bit(policy, hq, dtype):
    """Split decode at T = 6400 (beyond the fast decode scorer's 6144 slots): the generic scorer folds ~50 key-range partials itself, so
    the long plan has its fold launch in front, then sweep (7 column tiles) and select.  Four steps, one victim per head each."""
    from easykv_amd import StepPlan
    H, D, T = 2, 64, 6400
    g = torch.Generator().manual_seed(640 + hq)
    k0, v0 = torch.randn(1, H, T, D, generator=g).to(dtype), torch.randn(1, H, T, D, generator=g).to(dtype)
    plain, long = banks = _twins(1, hq, H, D, T + 64, dtype)
    for b in banks:
        b.load_rows(k0.cuda(), v0.cuda())
        b.state_init(T + 1, 0)
    _warm(banks, T, g)
    plan = StepPlan(policy=policy, phase="decode", accumulate=True, evict=True, budget=T)
    ip, il = _ends_in_the_two_scorers(plain, long, plan, 1)
    assert ip["n_split"] > 8 and il["n_launches"] == ip["n_launches"] + 2 and il["long_tiles"] == 7, (ip, il)
    for step in range(4):
        q, k, v = (torch.randn(1, n_h, 1, D, generator=g).to(dtype).cuda() for n_h in (hq, H, H))
        _, ids = _step_both(plain, long, plan, q, k, v, (policy, step))
        assert ids.shape == (1, H, 1)
    assert plain.n_slots == [T]
    _check_permutation(long)


@pytest.mark.parametrize("policy,two_pass,head_mean", [("roco", -1, False), ("roco", 1, False), ("h2o_head", 1, False), ("tova", 0, False), ("tova", 0, True)],
                         ids=["roco-onepass", "roco-twopass", "h2o-twopass", "tova", "tova-headmean"])
def test_split_chunk_steps_equal_the_generic_scorer_bit_for_bit(policy, two_pass, head_mean):
    """A chunk step of stride 16 onto ~1500 rows with the heads forced into two key-range splits (no scorer tail, no in-kernel fold): the
    exported logits of the one-pass kernel, the column-sum partials of the two passes, tova's last row and its head mean."""
    from easykv_amd import StepPlan
    H, hq, D, idx, s = 2, 4, 64, 1488, 16
    g = torch.Generator().manual_seed(1500)
    k0, v0 = torch.randn(1, H, idx, D, generator=g).half(), torch.randn(1, H, idx, D, generator=g).half()
    plain, long = banks = _twins(1, hq, H, D, idx + s)
    for b in banks:
        b.load_rows(k0.cuda(), v0.cuda())
        b.state_init(idx + s, 2, s)
    kw = dict(policy=policy, phase="prefill", accumulate=True, evict=True, budget=idx, recent=int(idx * 0.1), sink=4, stride=s, n_split=2,
              two_pass=two_pass, tova_head_mean=head_mean)
    ip, il = _ends_in_the_two_scorers(plain, long, StepPlan(**kw), s)
    assert ip["n_split"] == 2 and ip["two_pass"] == (1 if two_pass == 1 else 0) and il["long_tiles"] == 2, (ip, il)
    for step in range(2):
        q, k, v = (torch.randn(1, n_h, s, D, generator=g).half().cuda() for n_h in (hq, H, H))
        _, ids = _step_both(plain, long, StepPlan(**kw), q, k, v, (policy, two_pass, step))
        assert ids.shape == (1, H, s)
    assert long.n_slots == [idx]
    _check_permutation(long)


def test_many_partials_under_the_512_thread_build_equal_the_generic_scorer_bit_for_bit():
    """288 (head, layer) pairs with narrow rows: the plain call runs the generic scorer's 512-thread build, which folds the key-range
    partials in batches of 16 (the other builds: 8).  With 24 partials per query row (12 forced splits of the 16x16 kernel, two key halves
    each) the two batch widths round differently, so the long fold and the sweep's row statistics must take the 16-wide batches too."""
    from easykv_amd import StepPlan
    L, H, D, idx, s = 9, 32, 32, 1520, 16
    g = torch.Generator().manual_seed(288)
    k0, v0 = torch.randn(L, H, idx, D, generator=g).half(), torch.randn(L, H, idx, D, generator=g).half()
    plain, long = banks = _twins(L, H, H, D, idx + s)
    for b in banks:
        b.load_rows(k0.cuda(), v0.cuda())
        b.state_init(idx + s, 2, s)
    kw = dict(policy="roco", phase="prefill", accumulate=True, evict=True, budget=idx, recent=int(idx * 0.1), sink=4, stride=s, n_split=12, two_pass=-1)
    ip, il = _ends_in_the_two_scorers(plain, long, StepPlan(**kw), s)
    assert ip["n_split"] == 12 and ip["two_pass"] == 0 and ip["fold_in_kernel"] == 0 and il["n_launches"] == ip["n_launches"] + 2, (ip, il)
    for step in range(2):
        q, k, v = (torch.randn(L, H, s, D, generator=g).half().cuda() for _ in range(3))
        _step_both(plain, long, StepPlan(**kw), q, k, v, step)
    _check_permutation(long)


def test_wide_rows_of_the_scratch_build_equal_the_generic_scorer_bit_for_bit():
    """The shape of test_wide_score_rows_beyond_one_cus_lds (12 400 columns: the plain call runs the generic scorer's build that keeps
    S / Q / C in scratch): two chunk steps of stride 16 and three decode steps."""
    from easykv_amd import StepPlan
    H, D, idx, s = 2, 64, 12400, 16
    g = torch.Generator().manual_seed(31)
    k0, v0 = torch.randn(1, H, idx, D, generator=g).half(), torch.randn(1, H, idx, D, generator=g).half()
    plain, long = banks = _twins(1, H, H, D, idx + s)
    for b in banks:
        b.load_rows(k0.cuda(), v0.cuda())
        b.state_init(idx + s, 2, s)
    kw = dict(policy="roco", phase="prefill", accumulate=True, evict=True, budget=idx, recent=int(idx * 0.1), sink=4, stride=s)
    _ends_in_the_two_scorers(plain, long, StepPlan(**kw), s)
    for step in range(2):
        q, k, v = (torch.randn(1, H, s, D, generator=g).half().cuda() for _ in range(3))
        _step_both(plain, long, StepPlan(**kw), q, k, v, ("chunk", step))
    kw = dict(policy="roco", phase="decode", accumulate=True, evict=True, budget=idx)
    _ends_in_the_two_scorers(plain, long, StepPlan(**kw), 1)
    for step in range(3):
        q, k, v = (torch.randn(1, H, 1, D, generator=g).half().cuda() for _ in range(3))
        _step_both(plain, long, StepPlan(**kw), q, k, v, ("decode", step))
    _check_permutation(long)


def test_deferred_layers_and_flush_equal_the_generic_scorer_bit_for_bit():
    """One layer per call on a 2-layer bank at T = 6400 (what a decoder stack through the HF seam does): attention + fold per layer, the
    scorers of both layers at flush() — the generic scorer over all layers against sweep + select over all layers."""
    from easykv_amd import StepPlan
    L, H, D, T = 2, 2, 64, 6400
    g = torch.Generator().manual_seed(6402)
    k0, v0 = torch.randn(L, H, T, D, generator=g).half(), torch.randn(L, H, T, D, generator=g).half()
    plain, long = banks = _twins(L, H, H, D, T + 64)
    for b in banks:
        b.load_rows(k0.cuda(), v0.cuda())
        b.state_init(T + 1, 0)
    _warm(banks, T, g)
    plan = StepPlan(policy="roco", phase="decode", accumulate=True, evict=True, budget=T)
    for step in range(3):
        q, k, v = (torch.randn(L, H, 1, D, generator=g).half().cuda() for _ in range(3))
        for l in range(L):
            o_p, _ = plain.attend(plan, q[l:l + 1], k[l:l + 1], v[l:l + 1], layer_begin=l, defer=True)
            o_l, _ = long.attend(plan, q[l:l + 1], k[l:l + 1], v[l:l + 1], layer_begin=l, defer=True)
            assert torch.equal(o_p, o_l), (step, l)
        i_p, i_l = plain.flush(), long.flush()
        assert i_p.shape == (L, H, 1) and torch.equal(i_p, i_l), step
        _same_state(plain, long, step)
    _check_permutation(long)


# ---- (b) beyond the old limit, against the oracle ------------------------------------------------------------------------------------
# (policy, idx, stride, seed).  Stride 16: the one-pass chunk kernel (exported logits); 48: the two-pass kernels (column sums; tova has no
# two-pass form).  Seeds: each case was run on the CPU with the oracle alone, seeds 31, 32, 33, ... in order, and the first seed at which
# the probe calls all 5 * H decisions well defined was taken (tried, in order: see the list next to each case).
CASES_B = [
    ("roco", 40000, 16, 31),          # tried 31
    ("h2o_head", 40000, 48, 31),      # tried 31
    ("roco", 65600, 48, 31),          # tried 31
    ("h2o_head", 65600, 16, 31),      # tried 31
    ("tova", 40000, 16, 31),          # tried 31
]


def oracle_protocol(policy, idx, s, seed, H=2, D=64):
    """The oracle's side of a case, step by step: yields (kind, step, plan kwargs, (q, k, v), o_ref, ids_ref, unstable, state) for two
    scored chunk steps and three budgeted decode steps; the first item is ("rows", k0, v0).  Runs on the CPU alone."""
    from oracle import easykv_oracle as O
    bp, recent, sink = idx, int(idx * 0.1), 4
    g = torch.Generator().manual_seed(seed)
    k0, v0 = torch.randn(1, H, idx, D, generator=g).half(), torch.randn(1, H, idx, D, generator=g).half()
    yield "rows", k0, v0
    st = O.LayerState(k=k0.float(), v=v0.float())
    st.s, st.q, st.c = O.init_state_prefill((H,), idx, s, False)
    probe = Probe()
    O.SELECT_HOOK = probe
    try:
        for step in range(2):
            q, k, v = (torch.randn(1, H, s, D, generator=g).half() for _ in range(3))
            kw = dict(policy=policy, phase="prefill", accumulate=True, evict=True, budget=bp, recent=recent, sink=sink, stride=s)
            o_ref, ids_ref = O.layer_step(st, q.float(), k.float(), v.float(), O.StepPlan(**kw))
            yield "chunk", step, kw, (q, k, v), o_ref, ids_ref, probe.last_unstable.clone(), st
        st.s, st.q, st.c = (x[..., :-(s - 1)].clone() for x in (st.s, st.q, st.c))   # easykv/easykv.py:666-669
        for step in range(3):
            q, k, v = (torch.randn(1, H, 1, D, generator=g).half() for _ in range(3))
            kw = dict(policy=policy, phase="decode", accumulate=True, evict=True, budget=bp)
            o_ref, ids_ref = O.layer_step(st, q.float(), k.float(), v.float(), O.StepPlan(**kw))
            yield "decode", step, kw, (q, k, v), o_ref, ids_ref, probe.last_unstable.clone(), st
    finally:
        O.SELECT_HOOK = None


@pytest.mark.parametrize("policy,idx,s,seed", CASES_B, ids=[f"{p}-{i}-s{s}" for p, i, s, _ in CASES_B])
def test_rows_beyond_the_generic_scorers_width_against_the_oracle(policy, idx, s, seed):
    """Outputs within the output bar, eviction sets equal to the oracle's for EVERY decision (5 steps x H heads, none left out: the
    seeds make every one well defined), score rows at the project's rtol = 2e-4 / atol = 1e-6, the slot map a permutation.  The plain
    family refuses the first step (this is what fails without the feature)."""
    from easykv_amd import KVBank, StepPlan
    from easykv_amd._lib import EkvError
    H, D = 2, 64
    steps = oracle_protocol(policy, idx, s, seed, H, D)
    _, k0, v0 = next(steps)
    bank = KVBank(1, H, H, D, cap=idx + s, long_rows=True)
    bank.load_rows(k0.cuda(), v0.cuda())
    bank.state_init(idx + s, 2, s)
    checked, refused = 0, False
    for kind, step, kw, (q, k, v), o_ref, ids_ref, unstable, st in steps:
        if not refused:      # the same step on a plain bank: refused before anything is launched
            plain = KVBank(1, H, H, D, cap=idx + s)
            plain.load_rows(k0.cuda(), v0.cuda())
            plain.state_init(idx + s, 2, s)
            with pytest.raises(EkvError, match="unsupported shape"):
                plain.attend(StepPlan(**kw), q.cuda(), k.cuda(), v.cuda())
            assert plain.n_slots == [idx]
            del plain
            refused = True
        n = q.shape[2]
        info = bank.step_info(StepPlan(**kw), n)
        assert info["long_scorer"] == 1 and info["long_tiles"] == (idx + n + 1023) // 1024, info
        assert info["two_pass"] == (1 if (kind == "chunk" and s >= 40 and policy != "tova") else 0), info
        out, ids = bank.attend(StepPlan(**kw), q.cuda(), k.cuda(), v.cuda())
        assert out_close(out[0].float().cpu(), o_ref[0]), (kind, step)
        assert not bool(unstable.any()), (kind, step, "the oracle's probe calls a decision of this seed ill defined: choose another")
        got, ref = torch.sort(ids[0].cpu().long(), dim=-1)[0], torch.sort(ids_ref.view(H, -1), dim=-1)[0]
        assert torch.equal(got, ref), (kind, step)
        checked += H
        if kind == "chunk" and step == 1:
            for name, row in (("score_sum", st.s), ("score_sq", st.q)):
                if policy == "roco" or name == "score_sum":
                    assert torch.allclose(getattr(bank, name)[0, :, :idx].cpu(), row[..., :idx], rtol=2e-4, atol=1e-6), name
    for name, row in (("score_sum", st.s), ("score_sq", st.q)):
        if policy == "roco" or name == "score_sum":
            assert torch.allclose(getattr(bank, name)[0, :, :idx].cpu(), row[..., :idx], rtol=2e-4, atol=1e-6), name
    assert checked == 5 * H
    assert bank.n_slots[0] == idx
    _check_permutation(bank)


# ---- (c) the driver ----------------------------------------------------------------------------------------------------------------------
def test_generate_with_long_rows_equals_generate_without():
    """generate(long_rows=True) against long_rows=False on the fake model: a 6200-token prompt in decoding mode, so that every decode
    cache has more than 6144 slots (the fast decode scorer's bound: the plain run's steps end in the generic scorer, the long run's in
    sweep + select at every flush).  Identical tokens, printed line and evictions of every forward."""
    import easykv_amd
    from easykv_amd import StepPlan
    from easykv_amd._lib import EkvError
    from oracle.fake_model import make_streams
    from tests.native_fake_model import NativeFakeModel
    L, hq, h, D, n, budget, new = 2, 4, 2, 64, 6200, 8, 14
    streams = make_streams(L, hq, h, D, n + new + 2, seed=62)
    ids = torch.arange(n).view(1, -1) % 16
    runs = {}
    for long_rows in (False, True):
        model = NativeFakeModel(*streams)
        cfg = dict(budget=budget, kv_policy="roco", max_new_tokens=new, long_rows=long_rows, _record_evictions=True)
        printed = io.StringIO()
        with contextlib.redirect_stdout(printed):
            text, cache = easykv_amd.generate(model, ids, cfg, kv_mode="decoding", stride=1, return_cache=True)
        runs[long_rows] = (text, printed.getvalue(), cache, model.outputs_log)
        assert cache.bank.long_rows is long_rows and len(cache.evictions) == new - budget > 0, len(cache.evictions)
        plan = StepPlan(policy="roco", phase="decode", accumulate=True, evict=True, score_off=n, budget=budget)
        info = cache.bank.step_info(plan, 1, 0, 1)
        assert not info["fused"] and info.get("long_scorer", 0) == (1 if long_rows else 0), info      # the long scorer ran / did not
    (t0, p0, c0, o0), (t1, p1, c1, o1) = runs[False], runs[True]
    assert t0 == t1 and len(t0.split()) == new and p0 == p1 and "budget ratio" in p0
    assert all(torch.equal(a, b) for a, b in zip(o0, o1)) and len(o0) == len(o1)
    for f, (mine, theirs) in enumerate(zip(c1.evictions, c0.evictions)):
        assert torch.equal(torch.stack(list(mine)), torch.stack(list(theirs))), f
    for name in STATE:
        assert torch.equal(getattr(c0.bank, name), getattr(c1.bank, name)), name
    with pytest.raises(ValueError, match="long_rows.*kv_quant"):
        easykv_amd.generate(NativeFakeModel(*streams), ids, dict(cfg, kv_quant="fp8"), kv_mode="decoding", stride=1)
    with pytest.raises(ValueError, match="generate_batch.*long_rows"):
        easykv_amd.generate_batch(NativeFakeModel(*streams), [ids, ids], cfg, kv_mode="decoding", stride=1)
    with pytest.raises(EkvError, match="long_rows=True"):
        c1.bank.quantize("fp8")
