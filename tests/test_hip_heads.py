"""Deferred decode steps over KV heads of different lengths on the GPU (include/easykv_hip.h, "heads"): KVBank.attend(...,
defer=True) + flush() on a bank whose heads differ, served by the heads family (ekv_heads_*), whose kernels read every head's row count from
a device-resident table.

(1) Uniform counts: a bank with head_slots = [[128] * 4] * 2 against a plain bank, both stepped one layer per call with one flush — outputs,
    victims, slot map, score rows and the appended K/V rows are bit-identical (n_split 1 and 3, evict and grow, h2o_head / tova / roco, fp16
    and bf16).
(2) Ragged counts, the rule and the bars of test_hip_adaptive.test_decode_steps_over_heads_of_different_lengths: every head against a
    one-head twin bank stepped with the plain deferred call at the same explicit n_split.  Victims, slot maps and lengths are exact
    everywhere; outputs and score rows are exact wherever the arithmetic is the same — one key range per head, or the envelope's longest
    head — and otherwise inside golden_util.out_close / rtol 2e-5, atol 1e-7.  lens = [40, 64, 97, 128] and [128, 20, 20, 50]: the envelope
    (129 rows, two key ranges of 128 at n_split = 3) spans layers, and the second key range lies wholly past the end of every head but the
    longest.  Once more at head_dim 64, GQA 4, bf16, lens = [2, 33, 64, 65]: the envelope of 66 rows is ONE key range of the kernel's 128-row
    pitch whatever n_split asks for, so there every head is exact; a third case gives that build a head of 140 rows (160-row banks), so that
    its second key range is empty for every other head.
(3) A layer without head_slots inside a ragged bank; 66 KV heads, which the batched view call cannot express; flush() with a layer missing
    and a second step before the flush; a chunk plan on ragged layers.
(4) The driver with generation_config['head_decode'] = 'deferred': the fake model of test_hip_adaptive's driver test held against
    tests/adaptive_ref.generate exactly as that test holds it, one flush per forward and no call of the view; the tiny stock Llama."""
import pytest
import torch

from tests.golden_util import out_close
from tests.test_hip_adaptive import GEN, GEN_CASES, _decode_bank, _gen_cfg, _prompt
from tests.test_hip_oneshot import _mk

gpu = pytest.mark.gpu
BF = torch.bfloat16
ROWS, STEPS = 128, 3


def _bank(Lh, Hq, H, D, rows, k0, v0, S0, lens=None, dtype=torch.float16, roco=False):
    """tests/test_hip_adaptive._decode_bank, for either element type (`lens`: one list for all layers, or one per layer); roco: count and
    square rows to go with the hand-made sums."""
    from easykv_amd import KVBank
    if dtype is torch.float16:
        bank = _decode_bank(Lh, Hq, H, D, rows, k0, v0, S0, None)
    else:
        bank = KVBank(Lh, Hq, H, D, cap=rows + 8, dtype=dtype)
        bank.use_slot_rows = False
        bank.load_rows(k0.cuda(), v0.cuda())
        bank.score_sum.zero_()
        bank.score_sum[:, :, :rows] = S0.cuda()
    if roco:
        bank.score_cnt[:, :, :rows] = (S0 > 0).float().cuda() * 4.0
        bank.score_sq[:, :, :rows] = (S0 * S0 / 4.0 + 0.01 * S0).cuda()
    if lens is not None:
        per_layer = [lens] * Lh if not isinstance(lens[0], (list, type(None))) else lens
        bank.head_slots = [list(r) if r is not None else None for r in per_layer]
        bank.n_slots = [max(r) if r is not None else rows for r in per_layer]
    return bank


def _token(bank, plan, q, k, v, t, layers=None):
    """One token step, one layer per call, one flush: (out [L, Hq, 1, D], ids or None)."""
    outs = [bank.attend(plan, q[l:l + 1, :, t:t + 1].cuda().contiguous(), k[l:l + 1, :, t:t + 1].cuda().contiguous(), v[l:l + 1, :, t:t + 1].cuda().contiguous(),
                        layer_begin=l, defer=True)[0] for l in (range(bank.n_layers) if layers is None else layers)]
    return torch.cat(outs), bank.flush()


def _plan(policy, evict, n_split, budget=32):
    from easykv_amd import StepPlan
    return StepPlan(policy=policy, phase="decode", evict=evict, score_off=0, budget=budget, n_split=n_split)


def _data(Lh, Hq, H, D, rows, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    k0, v0 = _mk(Lh, H, rows, g, D, dtype), _mk(Lh, H, rows, g, D, dtype)
    qs, ks, vs = _mk(Lh, Hq, STEPS, g, D, dtype), _mk(Lh, H, STEPS, g, D, dtype), _mk(Lh, H, STEPS, g, D, dtype)
    return k0, v0, qs, ks, vs, torch.rand(Lh, H, rows, generator=g) + 0.5


@gpu
@pytest.mark.parametrize("policy", ("h2o_head", "tova", "roco"))
@pytest.mark.parametrize("dt", ("f16", "bf16"))
def test_uniform_counts_equal_the_plain_deferred_step_bit_for_bit(dt, policy):
    Lh, Hq, H, D = 2, 8, 4, 128
    dtype = BF if dt == "bf16" else torch.float16
    k0, v0, qs, ks, vs, S0 = _data(Lh, Hq, H, D, ROWS, dtype, 86001)
    for n_split in (1, 3):
        for evict in (False, True):
            plan = _plan(policy, evict, n_split)
            plain = _bank(Lh, Hq, H, D, ROWS, k0, v0, S0, None, dtype, policy == "roco")
            heads = _bank(Lh, Hq, H, D, ROWS, k0, v0, S0, [ROWS] * H, dtype, policy == "roco")
            for t in range(STEPS):
                (o1, i1), (o2, i2) = _token(plain, plan, qs, ks, vs, t), _token(heads, plan, qs, ks, vs, t)
                tag = (dt, policy, n_split, evict, t)
                assert torch.equal(o1, o2) and bool(torch.isfinite(o2.float()).all()), tag
                assert (i1 is None and i2 is None and not evict) or torch.equal(i1, i2), tag
                assert heads.head_slots == [[plain.n_slots[0]] * H] * Lh and heads.n_slots == plain.n_slots, tag
                for arr in ("slot_of_pos", "score_sum") + (("score_sq", "score_cnt") if policy == "roco" else ()):
                    assert torch.equal(getattr(plain, arr), getattr(heads, arr)), tag + (arr,)
            (k1, v1), (k2, v2) = plain.ordered_kv(), heads.ordered_kv()      # the appended rows among them
            assert torch.equal(k1, k2) and torch.equal(v1, v2), (dt, policy, n_split, evict, "rows")
            assert heads.head_table_uploads == 1 and plain.head_table_uploads == 0
            assert heads._view is None      # (the view call never ran)


def _ragged_case(Lh, Hq, H, D, dtype, lens, budget, seed, n_splits, ROWS=ROWS):
    """Every head of a ragged bank against its one-head twin (Lh layers, each a copy of that head), both stepped one layer per call."""
    rep = Hq // H
    k0, v0, qs, ks, vs, S0 = _data(Lh, Hq, H, D, ROWS, dtype, seed)
    Sr = S0.clone()
    for l in range(Lh):
        for h, T in enumerate(lens[l]):
            Sr[l, h, T:] = 0
    longest = max(max(r) for r in lens)
    for n_split in n_splits:
        one_range = n_split == 1 or longest + STEPS + 1 <= 128      # (the split kernel's key ranges are multiples of 128 rows)
        for evict in (False, True):
            plan = _plan("h2o_head", evict, n_split, budget)
            bank = _bank(Lh, Hq, H, D, ROWS, k0, v0, Sr, lens, dtype)
            twins = {}
            for l in range(Lh):
                for h, T in enumerate(lens[l]):
                    x = lambda a: a[l:l + 1, h:h + 1].expand(Lh, -1, -1, -1).contiguous()
                    tw = _bank(Lh, rep, 1, D, ROWS, x(k0), x(v0), x(Sr[:, :, :, None])[..., 0], None, dtype)
                    tw.n_slots = [T] * Lh
                    twins[l, h] = tw
            for t in range(STEPS):
                out, ids = _token(bank, plan, qs, ks, vs, t)
                assert (ids is None) == (not evict) and (ids is None or tuple(ids.shape) == (Lh, H, 1))
                for (l, h), tw in twins.items():
                    xq = qs[l:l + 1, h * rep:(h + 1) * rep].expand(Lh, -1, -1, -1)
                    xk, xv = ks[l:l + 1, h:h + 1].expand(Lh, -1, -1, -1), vs[l:l + 1, h:h + 1].expand(Lh, -1, -1, -1)
                    o2, i2 = _token(tw, plan, xq, xk, xv, t)
                    tag = (str(dtype), n_split, evict, t, l, h)
                    exact = one_range or lens[l][h] == longest
                    got = out[l, h * rep:(h + 1) * rep]
                    diff = float((got.float() - o2[0].float()).abs().max())
                    print(f"[heads] ragged {tag}: max |out - twin| = {diff:.3g}")
                    assert torch.equal(got, o2[0]) if exact else out_close(got, o2[0]), tag + (diff,)
                    assert not evict or torch.equal(ids[l, h], i2[0, 0]), tag + ("victim",)
                    assert bank.head_slots[l][h] == tw.n_slots[0] == lens[l][h] + (0 if evict else t + 1), tag
                    assert torch.equal(bank.slot_of_pos[l, h], tw.slot_of_pos[0, 0]), tag + ("slot map",)
                    a, b = bank.score_sum[l, h], tw.score_sum[0, 0]
                    assert torch.equal(a, b) if exact else torch.allclose(a, b, rtol=2e-5, atol=1e-7), tag + ("score row",)
                assert bank.n_slots == [max(r) for r in bank.head_slots]
            assert bank.head_table_uploads == 1 and bank._heads["desc"].grow == (0 if evict else STEPS), (n_split, evict)
            assert bank._view is None


@gpu
def test_ragged_counts_against_one_head_twins():
    _ragged_case(2, 8, 4, 128, torch.float16, [[40, 64, 97, 128], [128, 20, 20, 50]], 32, 86002, (1, 3))


@gpu
def test_ragged_counts_head_dim_64_gqa4_bf16():
    _ragged_case(2, 16, 4, 64, BF, [[2, 33, 64, 65], [2, 33, 64, 65]], 4, 86003, (3,))


@gpu
def test_ragged_counts_head_dim_64_gqa4_bf16_with_an_empty_key_range():
    """The same build (head_dim 64, REP = 4, bf16) with one head of 140 rows: the envelope of 141 rows is two key ranges of 128, and the second
    lies wholly past the end of every other head."""
    _ragged_case(2, 16, 4, 64, BF, [[2, 33, 64, 140], [140, 64, 2, 33]], 4, 86006, (3,), ROWS=160)


@gpu
def test_other_engine_paths():
    from easykv_amd import StepPlan
    from easykv_amd._lib import EkvError
    Lh, Hq, H, D = 2, 8, 4, 128
    k0, v0, qs, ks, vs, S0 = _data(Lh, Hq, H, D, ROWS, torch.float16, 86004)
    # a layer without head_slots inside a ragged bank counts as uniform lengths: its heads step as the plain bank's
    lens0 = [40, 64, 97, 128]
    Sr = S0.clone()
    for h, T in enumerate(lens0):
        Sr[0, h, T:] = 0
    plan = _plan("h2o_head", True, 3)
    plain, bank = _bank(Lh, Hq, H, D, ROWS, k0, v0, Sr), _bank(Lh, Hq, H, D, ROWS, k0, v0, Sr, [lens0, None])
    for t in range(STEPS):
        (o1, i1), (o2, i2) = _token(plain, plan, qs, ks, vs, t), _token(bank, plan, qs, ks, vs, t)
        assert torch.equal(o1[1], o2[1]) and torch.equal(i1[1], i2[1]), t
        assert torch.equal(plain.slot_of_pos[1], bank.slot_of_pos[1]) and torch.equal(plain.score_sum[1], bank.score_sum[1]), t
        assert torch.equal(o1[0, 6:8], o2[0, 6:8])      # (layer 0's longest head holds what the plain bank's holds)
    assert bank.head_slots == [lens0, [ROWS] * H] and bank.head_table_uploads == 1
    # flush() with a layer missing; a second step before the flush; a chunk plan on ragged layers
    step = lambda b, p, l: b.attend(p, qs[l:l + 1, :, :1].cuda().contiguous(), ks[l:l + 1, :, :1].cuda().contiguous(), vs[l:l + 1, :, :1].cuda().contiguous(),
                                    layer_begin=l, defer=True)
    step(bank, plan, 0)
    with pytest.raises(EkvError, match="1 of 2 layers attended"):
        bank.flush()
    with pytest.raises(EkvError, match="previous step was not flushed"):
        step(bank, _plan("h2o_head", True, 3), 1)
    step(bank, plan, 1)
    with pytest.raises(EkvError, match="previous step was not flushed"):
        step(bank, plan, 0)
    assert tuple(bank.flush().shape) == (Lh, H, 1)
    chunk = StepPlan(policy="h2o_head", phase="prefill", accumulate=True, evict=True, budget=64, stride=8)
    with pytest.raises(EkvError, match="different numbers of rows"):
        bank.attend(chunk, qs[:1, :, :2].cuda().contiguous(), ks[:1, :, :2].cuda().contiguous(), vs[:1, :, :2].cuda().contiguous(), layer_begin=0, defer=True)
    # 66 KV heads (head_dim 64, 32 rows, one layer): past the 64 entries of the batched view call, served by the table
    H2, D2, rows2 = 66, 64, 32
    g = torch.Generator().manual_seed(86005)
    k2, v2 = _mk(1, H2, rows2, g, D2, torch.float16), _mk(1, H2, rows2, g, D2, torch.float16)
    q2, kn2, vn2 = _mk(1, H2, STEPS, g, D2, torch.float16), _mk(1, H2, STEPS, g, D2, torch.float16), _mk(1, H2, STEPS, g, D2, torch.float16)
    S2 = torch.rand(1, H2, rows2, generator=g) + 0.5
    plan2 = _plan("h2o_head", True, 1, budget=8)
    plain, wide = _bank(1, H2, H2, D2, rows2, k2, v2, S2), _bank(1, H2, H2, D2, rows2, k2, v2, S2, [rows2] * H2)
    for t in range(STEPS):
        (o1, i1), (o2, i2) = _token(plain, plan2, q2, kn2, vn2, t), _token(wide, plan2, q2, kn2, vn2, t)
        assert torch.equal(o1, o2) and torch.equal(i1, i2) and torch.equal(plain.slot_of_pos, wide.slot_of_pos) and torch.equal(plain.score_sum, wide.score_sum), t
    with pytest.raises(ValueError, match="ekv_batch_step_attend"):      # (the immediate form stays the view call, which has no table of 66 entries)
        wide.attend(plan2, q2[:, :, :1].cuda().contiguous(), kn2[:, :, :1].cuda().contiguous(), vn2[:, :, :1].cuda().contiguous())


@gpu
@pytest.mark.parametrize("mode,policy,pool,op", GEN_CASES, ids=[f"{c[0]}-{c[1]}" for c in GEN_CASES])
def test_generate_with_deferred_head_decode_against_the_test_side_driver(mode, policy, pool, op, monkeypatch):
    """tests/test_hip_adaptive.test_generate_with_adaptive_head_budgets_against_the_test_side_driver with head_decode = 'deferred': the same
    streams, seed and assertions.  The reference alone, run on a CPU, marks 24 of 24 decode decisions of the `auto` case stable."""
    import contextlib
    import io
    import easykv_amd
    from easykv_amd.engine import KVBank
    from oracle import easykv_oracle as O
    from oracle.fake_model import make_streams
    from tests import adaptive_ref as A
    from tests.native_fake_model import NativeFakeModel
    from tests.test_hip_fullsize import Probe
    g = GEN
    n, B, obs, m, Lg, H = g["n"], g["B"], g["obs"], g["m"], g["L"], g["H"]
    cfg = _gen_cfg(policy, pool, op)
    streams = make_streams(Lg, g["Hq"], H, g["D"], n + m + 8, seed=g["seed"])
    calls = dict(flush=0, layer=0)

    def no_view(self, *a, **k):
        raise AssertionError("_attend_ragged was called")
    flush_heads, attend_heads = KVBank._flush_heads, KVBank._attend_heads

    def count_flush(self, d):
        calls["flush"] += 1
        return flush_heads(self, d)

    def count_layer(self, *a, **k):
        calls["layer"] += 1
        return attend_heads(self, *a, **k)
    monkeypatch.setattr(KVBank, "_attend_ragged", no_view)
    monkeypatch.setattr(KVBank, "_flush_heads", count_flush)
    monkeypatch.setattr(KVBank, "_attend_heads", count_layer)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        res, cache = easykv_amd.generate(NativeFakeModel(*streams), _prompt(n), dict(cfg, _record_evictions=True, head_decode="deferred"), kv_mode=mode, stride=4,
                                         return_cache=True)
    assert calls == dict(flush=m, layer=m * Lg), calls      # one flush per decode forward, one deferred attend per layer
    assert cache.bank.head_table_uploads == 1      # written once per prompt: evicting steps leave every length, growing steps advance `grow`
    ev = [torch.stack(e).cpu().long() for e in cache.evictions]      # per evicting forward: [L, H, k]
    ne, lo, hi = A.budget_bounds(n, B, obs, g["sink"])
    assert ev[0].shape == (Lg, H, hi) and len(ev) == 1 + (m if mode == "auto" else 0)
    assert max(cache.bank.extent) <= n - lo + m

    def follow(l, victims_ref, rank, bounds):
        ours = [ev[0][l, h][ev[0][l, h] >= 0] for h in range(H)]
        assert bounds == (ne, lo, hi) and A.meets_cap(rank, ne, lo, hi, g["sink"], obs) and A.valid(ours, rank, ne, lo, hi, g["sink"], obs), (l, [len(o) for o in ours])
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
    for l in range(Lg):
        assert sum(cache.bank.head_slots[l]) == H * (B + grown) and len(set(cache.bank.head_slots[l])) > 1, cache.bank.head_slots[l]
        assert cache.bank.head_slots[l] == [len(p) for p in ref["positions"][l]]
    if mode == "auto":
        assert all(bool((e >= 0).all()) and e.shape == (Lg, H, 1) for e in ev[1:])
        print(f"[heads] generate auto {policy}: compared {stats[0]} of {stats[1]} decode decisions")
        assert stats[1] == m * Lg * H and 2 * stats[0] >= stats[1]
    kk, _ = cache.bank.ordered_kv()
    for l in range(Lg):
        for h in range(H):
            if bool(alive[l, h]):
                pos = ref["positions"][l][h]
                assert torch.equal(kk[l, h, :len(pos)].cpu(), streams[1][l][h][pos]), (l, h)


@gpu
def test_stock_tiny_llama_with_deferred_head_decode():
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
        gc = dict(budget=64, kv_policy=policy, max_new_tokens=5, eos_token_ids=[-1], temperature=1e-6, prefill="one_shot", obs_window=16,
                  score_pool=pool, head_budgets="adaptive", head_decode="deferred")
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            out, cache = model.easykv_generate(input_ids=ids, generation_config=gc, return_cache=True)
        grown = 5 if mode == "encoding" else 0
        assert len(out.split()) == 5 and cache.get_seq_length() == 64 + grown, (mode, out)
        want = "KV cache budget ratio: 42.67%(64/150)" if mode == "encoding" else "KV Cache Budget ratio 41.29%[64/(150+5)]"
        assert want in buf.getvalue(), buf.getvalue()
        bank = cache.bank
        assert bank._view is None and bank.head_table_uploads == 1 and cache.head_decode == "deferred"
        assert all(sum(r) == len(r) * (64 + grown) for r in bank.head_slots) and any(len(set(r)) > 1 for r in bank.head_slots), (mode, bank.head_slots)
