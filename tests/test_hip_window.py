"""Per-layer sliding-window masking (gpt-oss: sliding_window = 128 on every other layer) on the GPU: a KVBank(windows=...)
against a twin bank without windows and against the oracle with the windowed attention as its `attention_core` (tests/window_ref.py).
Every bank has L = 2 layers with windows [W, 0] or [0, W], so one launch serves a local and a full layer.

(1) Twin banks, no tolerance.  With every window 0, and with a window wider than the sequence, outputs, victims, slot maps and score rows
equal those of the plain bank (head_dim 128, no resident rows) or the sink bank (head_dim 64) bit for bit, at cache lengths T = 2 / 65 /
300 with the key range of the last unsplit, split in 2 and split in 3.
(2) Decode steps against O.layer_step with the window core: the shapes of tests/test_hip_sink.py's DECODE_CASES (64 / 16 / 2 with sinks,
128 / 4 / 4 and 128 / 8 / 2 without), roco / h2o_head / tova, fp16 and bf16, T = 2, 65, 300 with six evicting steps where T > 2, and
W = 1 (only the query's own key: without sinks the output is v_new exactly), 5 (a mask edge inside a byte of mask bits), 64 (on a word
edge) and 40 (at T = 300 split in 3, the first two key ranges are wholly masked); one case starts from load_rows(tok_pos=...) with
gaps that differ per head, so heads mask different counts.  Outputs under out_close (bf16: the bar of tests/test_hip_sink.py), victims
identical wherever the Probe of tests/test_hip_fullsize.py calls the decision stable, ordered_tok_pos() equal to the positions the test
tracked for every head that never left the probe's class, and the oracle's own distance between windowed and full attention over the run
at least 1e-2: a path that ignores the window cannot pass.

(3) Chunk steps and the dense prefix: one twin case per mode of the 16x16x32 kernel, one oracle case per planned path (one pass with the
scorer tail, statistics + exact pass + generic scorer, split) with W < stride, W = stride and W so small that whole 32-key half tiles
and a whole key split are masked, and a 300-token dense prefix at W = 40, with and without keep_attention.

(4) easykv_amd.generate on a fake window + sink model (generation_config['sliding_window'] as a list) against O.generate with the window
core: eviction ids under the probe, the printed line, the text.
(5) The seam: a tiny stock GptOssForCausalLM with sliding_window = 8 on a 40-token prompt against the eager forward of an fp32 copy of
its 16-bit weights — inside the bar with generation_config['sliding_window'] = 'model', outside it without the key."""
import contextlib
import io

import numpy as np
import pytest
import torch

from tests.golden_util import out_close
from tests.test_hip_d256 import _enough, _permutation
from tests.test_hip_fullsize import Probe
from tests.window_ref import drop_positions, make_core, model_core, patched

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
WIDE = 1 << 20      # a window wider than any sequence here


def _mk(L, H, n, g, d, dtype=torch.float16):
    return torch.randn(L, H, n, d, generator=g).to(dtype)


def _sinks(L, Hq, seed=11):
    return torch.randn(L, Hq, generator=torch.Generator().manual_seed(seed)) + 1


def _bf16_close(out, ref, pv):
    """The bf16 bar of tests/test_hip_sink.py: |o - ref| <= 2^-8 (|ref| + pv) + 1e-6 pv, pv = p.|V| of the reference's probabilities."""
    err = (out - ref).abs()
    return bool(torch.isfinite(out).all()) and bool((err <= 2.0 ** -8 * (ref.abs() + pv) + 1e-6 * pv).all())


# ---- (1) twin banks -------------------------------------------------------------------------------------------------------------------------
def _same_state(a, b, what):
    for name in ("slot_of_pos", "score_sum", "score_sq", "score_cnt"):
        assert torch.equal(getattr(a, name), getattr(b, name)), (what, name)


TWIN_DECODE = [
    # id, D, Hq, H, with sinks, n_split at T = 300, windows
    ("d128_mha_unsplit_zero", 128, 4, 4, False, 1, (0, 0)),
    ("d128_mha_split2_wide_bf16", 128, 4, 4, False, 2, (WIDE, 0)),
    ("d128_gqa4_split3_wide", 128, 8, 2, False, 3, (0, WIDE)),
    ("d128_gqa4_split3_zero", 128, 8, 2, False, 3, (0, 0)),
    ("d64_gqa8_sinks_unsplit_wide", 64, 16, 2, True, 1, (WIDE, 0)),
    ("d64_gqa8_sinks_split2_zero_bf16", 64, 16, 2, True, 2, (0, 0)),
    ("d64_gqa8_sinks_split3_wide", 64, 16, 2, True, 3, (0, WIDE)),
]


@pytest.mark.parametrize("name,D,Hq,H,with_sinks,n_split,windows", TWIN_DECODE, ids=[c[0] for c in TWIN_DECODE])
def test_zero_and_wide_windows_equal_the_twin_without_windows_bit_for_bit(name, D, Hq, H, with_sinks, n_split, windows):
    from easykv_amd import KVBank, StepPlan
    dtype = BF if name.endswith("bf16") else torch.float16
    L = 2
    g = torch.Generator().manual_seed(61000 + D + Hq + n_split)
    base = dict(sinks=_sinks(L, Hq)) if with_sinks else {}
    paths = set()
    for T in (2, 65, 300):
        budget, evict, steps = T - 1, T > 2, (6 if T > 2 else 1)
        k0, v0 = _mk(L, H, budget, g, D, dtype), _mk(L, H, budget, g, D, dtype)
        banks = [KVBank(L, Hq, H, D, cap=T + 8, dtype=dtype, **kw) for kw in (base, dict(base, windows=list(windows)))]
        banks[0].resident_bytes = 0      # (the twin: no resident rows, as the window instances are built)
        for b in banks:
            b.load_rows(k0.cuda(), v0.cuda())
            b.state_init(T, 0)
        assert banks[1].tokens_seen == budget
        for i in range(steps):
            q, k, v = _mk(L, Hq, 1, g, D, dtype).cuda(), _mk(L, H, 1, g, D, dtype).cuda(), _mk(L, H, 1, g, D, dtype).cuda()
            plan = StepPlan(policy="roco", phase="decode", evict=evict, score_off=0, budget=budget, n_split=n_split)
            infos = [b.step_info(plan, 1) for b in banks]
            same = ("n_split", "fused", "n_launches", "two_pass", "wide", "fold_in_kernel")
            assert {k_: infos[0][k_] for k_ in same} == {k_: infos[1][k_] for k_ in same}, (name, T, i, infos)
            assert infos[1]["fused_order"] == 0, infos[1]      # the window instances run phase order F
            paths.add((bool(infos[1]["fused"]), infos[1]["n_split"]))
            (o0, i0), (o1, i1) = (b.attend(plan, q, k, v) for b in banks)
            assert torch.equal(o0, o1), (name, T, i, float((o0.float() - o1.float()).abs().max()))
            assert (i0 is None and i1 is None) or torch.equal(i0, i1), (name, T, i)
        assert banks[1].tokens_seen == budget + steps
        _same_state(banks[0], banks[1], (name, T))
        _permutation(banks[1])
    assert (True, 1) in paths and (n_split == 1 or (False, n_split) in paths), (name, paths)


@pytest.mark.parametrize("W", [WIDE, 5], ids=["wide", "w5"])
def test_window_steps_on_the_slot_indexed_layout(W):
    """528 heads in one launch run the one-launch kernel on the slot-indexed layout of the score rows (its own tail).  A wide window
    there equals the plain twin; a real one (W = 5: most of the cache masked, the victims chosen among masked rows) equals the same
    window bank kept on the ordered layout, whose kernels section (2) holds to the oracle — outputs, victims and positions, step by step."""
    from easykv_amd import KVBank, StepPlan
    L, Hq, H, D, budget, steps = 33, 16, 16, 128, 70, 14
    g = torch.Generator().manual_seed(61500)
    windows = [W if l % 2 == 0 else 0 for l in range(L)]
    k0, v0 = _mk(L, H, budget, g, D), _mk(L, H, budget, g, D)
    banks = [KVBank(L, Hq, H, D, cap=budget + 1 + 63, **kw) for kw in ((dict() if W == WIDE else dict(windows=windows)), dict(windows=windows))]
    banks[0].resident_bytes = 0
    banks[0].use_slot_rows = W == WIDE      # (the real window's reference: the same bank on the ordered layout)
    for b in banks:
        b.load_rows(k0.cuda(), v0.cuda())
        b.state_init(budget + 1, 0)
    n_slot = 0
    for i in range(steps):
        q, k, v = _mk(L, Hq, 1, g, D).cuda(), _mk(L, H, 1, g, D).cuda(), _mk(L, H, 1, g, D).cuda()
        plan = StepPlan(policy="roco", phase="decode", evict=True, score_off=0, budget=budget, n_split=0)
        assert banks[1].step_info(plan, 1)["fused"] == 1
        (o0, i0), (o1, i1) = (b.attend(plan, q, k, v) for b in banks)
        n_slot += int(all(banks[1]._slot_rows))
        assert torch.equal(o0, o1), (W, i, float((o0.float() - o1.float()).abs().max()))
        assert torch.equal(i0, i1), (W, i)
    assert n_slot == steps, n_slot
    if W != WIDE:
        assert not any(banks[0]._slot_rows)
        assert torch.equal(banks[0].ordered_tok_pos(), banks[1].ordered_tok_pos())
        assert int(banks[1].ordered_tok_pos().max()) == budget + steps - 1
    else:      # (the same layout on both sides: the score rows too, bit for bit; across the two layouts the victims above are the statement)
        _same_state(banks[0], banks[1], W)
    _permutation(banks[1])


# ---- (2) decode steps against the oracle ------------------------------------------------------------------------------------------------
DECODE_CASES = [
    # id, D, Hq, H, policy, n_split, dtype, with sinks, W, the layer that has it, gaps, seed
    ("d64_gqa8_sinks_roco_fused_w5", 64, 16, 2, "roco", 1, torch.float16, True, 5, 0, False, 0),
    ("d64_gqa8_sinks_h2o_split3_w40", 64, 16, 2, "h2o_head", 3, torch.float16, True, 40, 1, False, 0),
    ("d64_gqa8_sinks_tova_split2_w64_bf16", 64, 16, 2, "tova", 2, BF, True, 64, 0, False, 0),
    ("d64_gqa8_sinks_roco_split2_w1", 64, 16, 2, "roco", 2, torch.float16, True, 1, 1, False, 0),
    ("d128_mha_roco_split3_w40", 128, 4, 4, "roco", 3, torch.float16, False, 40, 0, False, 0),
    ("d128_mha_tova_fused_w1", 128, 4, 4, "tova", 1, torch.float16, False, 1, 1, False, 0),
    ("d128_mha_h2o_split2_w64_gaps", 128, 4, 4, "h2o_head", 2, torch.float16, False, 64, 0, True, 0),
    ("d128_gqa4_h2o_split2_w5_bf16", 128, 8, 2, "h2o_head", 2, BF, False, 5, 0, False, 0),
    ("d128_gqa4_roco_fused_w64", 128, 8, 2, "roco", 1, torch.float16, False, 64, 1, False, 0),
    ("d128_gqa4_tova_split3_w40", 128, 8, 2, "tova", 3, torch.float16, False, 40, 1, False, 0),
]


def _gapped_positions(L, H, n, g):
    """Increasing token positions with gaps, different for every head: head (l, h) keeps a random n of the first n + 20 + 30 * h."""
    rows = []
    for l in range(L):
        for h in range(H):
            span = n + 20 + 30 * h
            rows.append(torch.sort(torch.randperm(span, generator=g)[:n])[0])
    return torch.stack(rows).view(L, H, n).int()


def run_decode_case(name, D, Hq, H, policy, n_split, dtype, with_sinks, W, wl, gaps, seed, oracle_only=False):
    """Whole-cache decode steps (score_off = 0) at cache lengths T = 2 (one accumulating step onto a 1-row cache), 65 and 300 (six
    evicting steps each; the forced split count applies at 300, where a key range holds at least 100 rows)."""
    from oracle import easykv_oracle as O
    L, rep = 2, Hq // H
    windows = [W if l == wl else 0 for l in range(L)]
    sinks = _sinks(L, Hq) if with_sinks else None
    g = torch.Generator().manual_seed(62000 + D + Hq + n_split + W + 1000 * seed)
    probe = Probe()
    n_checked = n_total = 0
    dist, paths = [0.0], set()
    for T in (2, 65, 300):
        budget, evict, steps = T - 1, T > 2, (6 if T > 2 else 1)
        k0, v0 = _mk(L, H, budget, g, D, dtype), _mk(L, H, budget, g, D, dtype)
        warm = torch.rand(L, H, T, generator=g) * 1e-3
        warm[:, :, budget:] = 0      # (the column of the row about to be appended starts empty)
        tp0 = _gapped_positions(L, H, budget, g) if gaps else torch.arange(budget, dtype=torch.int32).expand(L, H, budget)
        pos = [[tp0[l, h].tolist() for h in range(H)] for l in range(L)]      # token positions of the retained keys, in cache order
        seen = int(tp0.max()) + 1
        bank = None
        if not oracle_only:
            from easykv_amd import KVBank, StepPlan
            bank = KVBank(L, Hq, H, D, cap=T + 8, dtype=dtype, windows=windows, **(dict(sinks=sinks) if with_sinks else {}))
            bank.load_rows(k0.cuda(), v0.cuda(), **(dict(tok_pos=tp0) if gaps else {}))
            assert bank.tokens_seen == seen
            bank.state_init(T, 0)
            bank.score_sum[:, :, :T] += warm.cuda()
            bank.score_sq[:, :, :T] += (warm ** 2).cuda()
        sts = []
        for l in range(L):
            st = O.LayerState(k=k0[l:l + 1].float(), v=v0[l:l + 1].float())
            st.s, st.q, st.c = O.init_state_decoding((H,), budget)
            st.s += warm[l]
            st.q += warm[l] ** 2
            sts.append(st)
        kw = dict(policy=policy, phase="decode", evict=evict, score_off=0, budget=budget, range_start=-1)
        alive = torch.ones(L, H, dtype=torch.bool)
        O.SELECT_HOOK = probe
        try:
            for i in range(steps):
                q, k, v = _mk(L, Hq, 1, g, D, dtype), _mk(L, H, 1, g, D, dtype), _mk(L, H, 1, g, D, dtype)
                q_pos = seen + i
                if bank is not None:
                    plan = StepPlan(n_split=n_split, **kw)
                    info = bank.step_info(plan, 1)
                    want_fused = n_split == 1 or T < 300
                    assert bool(info["fused"]) == want_fused and (want_fused or info["n_split"] == n_split), (name, T, info)
                    assert info["fused_order"] == 0, info
                    paths.add(bool(info["fused"]))
                    assert bank.tokens_seen == q_pos
                    out, ids = bank.attend(plan, q.cuda(), k.cuda(), v.cuda())
                for l in range(L):
                    qf, kf, vf = q[l:l + 1].float(), k[l:l + 1].float(), v[l:l + 1].float()
                    key_pos = torch.tensor([pos[l][h] + [q_pos] for h in range(H)])
                    sk = sinks[l] if with_sinks else None
                    pv = None
                    if bank is not None and dtype is BF:
                        pv = make_core(windows[l], key_pos, [q_pos], sk)(qf, torch.cat([sts[l].k, kf], 2), torch.cat([sts[l].v, vf], 2).abs())[0][0]
                    with patched(windows[l], key_pos, [q_pos], sk, dist):
                        o_ref, ids_ref = O.layer_step(sts[l], qf, kf, vf, O.StepPlan(**kw))
                    if bank is not None:
                        rows = alive[l].repeat_interleave(rep)
                        got_o, ref_o = out[l].float().cpu(), o_ref[0]
                        close = out_close(got_o[rows], ref_o[rows]) if dtype is not BF else _bf16_close(got_o[rows], ref_o[rows], pv[rows])
                        assert close, (name, T, i, l, float((got_o[rows] - ref_o[rows]).abs().max()))
                        if windows[l] == 1 and not with_sinks:      # only the query's own key is attended: p = 1, the output IS v_new
                            assert torch.equal(out[l].cpu(), v[l].repeat_interleave(rep, dim=0)), (name, T, i, l)
                    for h in range(H):
                        pos[l][h].append(q_pos)
                    if evict:
                        drop_positions(pos[l], ids_ref)
                        ok = ~probe.last_unstable
                        same = torch.ones(H, dtype=torch.bool)
                        if bank is not None:
                            same = ids[l, :, 0].cpu().long() == ids_ref[:, 0]
                            assert bool(same[ok & alive[l]].all()), (name, T, i, l, ids[l, :, 0].tolist(), ids_ref[:, 0].tolist())
                        n_total += H
                        n_checked += int((ok & alive[l]).sum())
                        alive[l] &= ok & same
        finally:
            O.SELECT_HOOK = None
        if bank is not None:
            assert bank.tokens_seen == seen + steps
            tp = bank.ordered_tok_pos().cpu()
            for l in range(L):
                for h in range(H):
                    if bool(alive[l, h]):      # (a head that left the probe's class may have evicted another row than the oracle)
                        assert tp[l, h].tolist() == pos[l][h], (name, T, l, h)
            if not evict:      # T = 2: the accumulated rows are the window oracle's probabilities
                S = bank.score_sum.cpu()
                for l in range(L):
                    assert torch.allclose(S[l, :, :T], sts[l].s[:, :T], rtol=2e-5, atol=1e-7), (name, l, S[l, :, :T], sts[l].s[:, :T])
            _permutation(bank)
    if not oracle_only and n_split > 1:
        assert paths == {True, False}, (name, paths)      # the one-launch kernel at 2 and 65 rows, the split path at 300
    print(f"[window] {name}: max |o_window - o_full| of the oracle over the run = {dist[0]:.3e}")
    assert dist[0] >= 1e-2, (name, dist[0])      # a path that ignores the window cannot pass
    _enough(name, n_checked, n_total)
    return n_checked, n_total, dist[0]


@pytest.mark.parametrize("name,D,Hq,H,policy,n_split,dtype,with_sinks,W,wl,gaps,seed", DECODE_CASES, ids=[c[0] for c in DECODE_CASES])
def test_window_decode_steps_against_the_oracle(name, D, Hq, H, policy, n_split, dtype, with_sinks, W, wl, gaps, seed):
    run_decode_case(name, D, Hq, H, policy, n_split, dtype, with_sinks, W, wl, gaps, seed)


# ---- (3) chunk steps and the dense prefix -------------------------------------------------------------------------------------------------
TWIN_CHUNK = [
    # id, D, Hq, H, with sinks, stride, cached rows, windows, plan keywords, what the plan must say
    ("one_pass_split_d128_mha_zero", 128, 4, 4, False, 8, 1500, (0, 0), dict(), dict(fused=0, two_pass=0)),
    ("two_pass_d128_mha_wide_bf16", 128, 4, 4, False, 8, 1500, (WIDE, 0), dict(two_pass=1), dict(fused=0, two_pass=1)),
    ("one_pass_tail_d64_gqa8_sinks_wide", 64, 16, 2, True, 4, 1500, (0, WIDE), dict(n_split=1), dict(fused=1, two_pass=0, n_launches=1)),
    ("two_pass_split2_d64_gqa8_sinks_zero", 64, 16, 2, True, 4, 1500, (0, 0), dict(n_split=2, two_pass=1), dict(fused=0, two_pass=1, n_split=2)),
    # the head-mean TOVA row (encoding / ppl mode): the plain build of its kernel without sinks, the sink build with them
    ("tova_head_mean_d64_gqa8_sinks_wide", 64, 16, 2, True, 4, 1500, (WIDE, 0), dict(policy="tova", tova_head_mean=True), dict(two_pass=0)),
    ("tova_head_mean_d128_mha_zero", 128, 4, 4, False, 8, 1500, (0, 0), dict(policy="tova", tova_head_mean=True, n_split=2), dict(two_pass=0, n_split=2)),
]


@pytest.mark.parametrize("name,D,Hq,H,with_sinks,s,idx,windows,kw,expect", TWIN_CHUNK, ids=[c[0] for c in TWIN_CHUNK])
def test_zero_and_wide_windows_chunk_steps_equal_the_twin_bit_for_bit(name, D, Hq, H, with_sinks, s, idx, windows, kw, expect):
    """One chunk case per mode of the 16x16x32 kernel (one pass, one pass with the scorer tail, statistics + exact pass): shapes whose
    plain call runs the same one-tile build (tests/test_hip_sink.py: more than 1024 rows, few heads)."""
    from easykv_amd import KVBank, StepPlan
    dtype = BF if name.endswith("bf16") else torch.float16
    L = 2
    g = torch.Generator().manual_seed(61700 + D + s)
    k0, v0 = _mk(L, H, idx, g, D, dtype), _mk(L, H, idx, g, D, dtype)
    base = dict(sinks=_sinks(L, Hq)) if with_sinks else {}
    banks = [KVBank(L, Hq, H, D, cap=idx + s, dtype=dtype, **x) for x in (base, dict(base, windows=list(windows)))]
    for b in banks:
        b.load_rows(k0.cuda(), v0.cuda())
        b.state_init(idx + s, 2, s)
    plan = StepPlan(**dict(dict(policy="roco", phase="prefill", accumulate=True, evict=True, budget=idx + s // 2, recent=int(idx * 0.2), sink=4,
                                stride=s, tova_head_mean=False), **kw))
    for step in range(3):
        q, k, v = _mk(L, Hq, s, g, D, dtype).cuda(), _mk(L, H, s, g, D, dtype).cuda(), _mk(L, H, s, g, D, dtype).cuda()
        infos = [b.step_info(plan, s) for b in banks]
        assert infos[0] == infos[1] and infos[1]["wide"] == 0, (name, infos)
        assert all(infos[1][k_] == v_ for k_, v_ in expect.items()), (name, infos[1])
        (o0, i0), (o1, i1) = (b.attend(plan, q, k, v) for b in banks)
        assert torch.equal(o0, o1), (name, step, float((o0.float() - o1.float()).abs().max()))
        assert torch.equal(i0, i1), (name, step)
        _same_state(banks[0], banks[1], (name, step))
    assert banks[1].tokens_seen == idx + 3 * s
    _permutation(banks[1])


CHUNK_CASES = [
    # id, D, Hq, H, stride, cached rows, policy, two_pass, n_split, with sinks, W, the layer that has it, what the plan must say
    # (one per planned path of tests/test_hip_sink.py's CHUNK_CASES; W = stride, W < stride so the window cuts inside the chunk, and W = 40
    #  on 205 rows in two key ranges: the first range and whole 32-key half tiles of the second are masked)
    ("d64_gqa8_sinks_s4_one_pass_tail_w4", 64, 16, 2, 4, 200, "roco", -1, 1, True, 4, 0, dict(fused=1, two_pass=0, n_qblocks=1)),
    ("d64_gqa8_sinks_s8_two_pass_two_blocks_w5", 64, 16, 2, 8, 200, "roco", 0, 0, True, 5, 1, dict(fused=0, two_pass=1, n_qblocks=2)),
    ("d128_gqa4_s16_two_pass_split2_w40", 128, 8, 2, 16, 205, "roco", 1, 2, False, 40, 0, dict(fused=0, two_pass=1, n_split=2)),
    ("d128_gqa4_s8_one_pass_split2_w8", 128, 8, 2, 8, 200, "h2o_head", -1, 2, False, 8, 1, dict(fused=0, two_pass=0, n_split=2)),
    ("d128_mha_s8_one_pass_tail_w3", 128, 4, 4, 8, 200, "h2o_head", -1, 1, False, 3, 0, dict(fused=1, two_pass=0)),
]


def run_chunk_case(name, D, Hq, H, s, idx, policy, two_pass, n_split, with_sinks, W, wl, expect, oracle_only=False):
    """Four evicting chunk steps of `s` queries onto `idx` cached rows.  The score rows start from small distinct values in the bank and in
    the oracle alike: under a window most cached columns receive p = 0 from every query, and all-zero rows would leave every decision to
    the tie rule.  (tova is left to the decode cases: its row IS the last query's probabilities, exactly 0 on every masked key.)"""
    from oracle import easykv_oracle as O
    from tests.select_rule import feasible_classes, valid_victims
    from tests.test_hip_d256 import _ProbeAndCapture
    rep, L, n_steps = Hq // H, 2, 4
    windows = [W if l == wl else 0 for l in range(L)]
    budget_p, recent, sink = idx + s // 2, int(idx * 0.2), 4
    g = torch.Generator().manual_seed(63700 + D + s + idx)
    k0, v0 = _mk(L, H, idx, g, D), _mk(L, H, idx, g, D)
    warm = torch.rand(L, H, idx, generator=g) * 1e-3
    sinks = _sinks(L, Hq) if with_sinks else None
    pos = [[list(range(idx)) for _ in range(H)] for _ in range(L)]
    bank = None
    if not oracle_only:
        from easykv_amd import KVBank, StepPlan
        bank = KVBank(L, Hq, H, D, cap=idx + s, windows=windows, **(dict(sinks=sinks) if with_sinks else {}))
        bank.load_rows(k0.cuda(), v0.cuda())
        bank.state_init(idx + s, 2, s)
        bank.score_sum[:, :, :idx] += warm.cuda()
        bank.score_sq[:, :, :idx] += (warm ** 2).cuda()
    sts = []
    for l in range(L):
        st = O.LayerState(k=k0[l:l + 1].float(), v=v0[l:l + 1].float())
        st.s, st.q, st.c = O.init_state_prefill((H,), idx, s, False)
        st.s[:, :idx] += warm[l]
        st.q[:, :idx] += warm[l] ** 2
        sts.append(st)
    hook = _ProbeAndCapture()
    O.SELECT_HOOK = hook
    alive = torch.ones(L, H, dtype=torch.bool)
    n_checked = 0
    dist = [0.0]
    k1 = max(budget_p - recent - sink, s)
    try:
        for step in range(n_steps):
            q, k, v = _mk(L, Hq, s, g, D), _mk(L, H, s, g, D), _mk(L, H, s, g, D)
            q_pos = [idx + step * s + i for i in range(s)]
            kw = dict(policy=policy, phase="prefill", accumulate=True, evict=True, budget=budget_p, recent=recent, sink=sink, stride=s,
                      tova_head_mean=False)
            if bank is not None:
                plan = StepPlan(two_pass=two_pass, n_split=n_split, **kw)
                info = bank.step_info(plan, s)
                assert info["wide"] == 0 and info["qb_rows"] * rep <= 32 and info["n_qblocks"] == -(-s // info["qb_rows"]), (name, info)
                assert all(info[k_] == v_ for k_, v_ in expect.items()), (name, info)
                assert bank.tokens_seen == q_pos[0]
                out, ids = bank.attend(plan, q.cuda(), k.cuda(), v.cuda())
            for l in range(L):
                key_pos = torch.tensor([pos[l][h] + q_pos for h in range(H)])
                with patched(windows[l], key_pos, q_pos, sinks[l] if with_sinks else None, dist):
                    o_ref, ids_ref = O.layer_step(sts[l], q[l:l + 1].float(), k[l:l + 1].float(), v[l:l + 1].float(), O.StepPlan(**kw))
                for h in range(H):
                    pos[l][h].extend(q_pos)
                drop_positions(pos[l], ids_ref)
                if not bool(alive[l].any()):
                    continue
                ref = torch.sort(ids_ref, dim=-1)[0]
                if bank is not None:
                    rows = alive[l].repeat_interleave(rep)
                    got_o = out[l].float().cpu()
                    assert out_close(got_o[rows], o_ref[0][rows]), (name, step, l, float((got_o[rows] - o_ref[0][rows]).abs().max()))
                    got = torch.sort(ids[l].cpu().long(), dim=-1)[0]
                for h in range(H):
                    if not bool(alive[l, h]):
                        continue
                    if bool(hook.probe.last_unstable[h]):
                        alive[l, h] = False
                        continue
                    tied = False
                    if policy == "roco":
                        c = hook.cap
                        forced, pool, need = feasible_classes(O.roco_std(c.s, c.q, c.c, sink)[h], k1)
                        tied = len(pool) != need
                        if bank is not None:
                            assert valid_victims(got[h].tolist(), (c.s / c.c)[h], forced, pool, need, s), (name, step, l, h)
                    if tied:
                        alive[l, h] = False
                        continue
                    if bank is not None:
                        assert bool((got[h] == ref[h]).all()), (name, step, l, h, got[h].tolist(), ref[h].tolist())
                    n_checked += 1
    finally:
        O.SELECT_HOOK = None
    if bank is not None:
        assert bank.n_slots == [idx] * L and bank.tokens_seen == idx + n_steps * s
        tp = bank.ordered_tok_pos().cpu()
        for l in range(L):
            for h in range(H):
                if bool(alive[l, h]):
                    assert tp[l, h].tolist() == pos[l][h], (name, l, h)
        _permutation(bank)
    print(f"[window] {name}: max |o_window - o_full| of the oracle over the run = {dist[0]:.3e}")
    assert dist[0] >= 1e-2, (name, dist[0])
    _enough(name, n_checked, n_steps * L * H)
    return n_checked, n_steps * L * H, dist[0]


@pytest.mark.parametrize("name,D,Hq,H,s,idx,policy,two_pass,n_split,with_sinks,W,wl,expect", CHUNK_CASES, ids=[c[0] for c in CHUNK_CASES])
def test_window_chunk_steps_against_the_oracle(name, D, Hq, H, s, idx, policy, two_pass, n_split, with_sinks, W, wl, expect):
    run_chunk_case(name, D, Hq, H, s, idx, policy, two_pass, n_split, with_sinks, W, wl, expect)


@pytest.mark.parametrize("with_sinks,keep", [(False, False), (False, True), (True, True)], ids=["d128", "d128_keep_attention", "d64_sinks_keep_attention"])
def test_window_dense_prefix_against_the_windowed_attention(with_sinks, keep):
    """A 300-token dense prefix at W = 40 on one of the two layers: token position = logical position, so the mask is the band
    i - j < 40 under the diagonal.  Outputs against the window core; with keep_attention (accumulate) the column sums of the score rows
    against the core's GQA-folded probabilities."""
    from easykv_amd import KVBank, StepPlan
    (D, Hq, H), L, n, W = ((64, 16, 2) if with_sinks else (128, 8, 2)), 2, 300, 40
    rep = Hq // H
    g = torch.Generator().manual_seed(64000 + D)
    sinks = _sinks(L, Hq) if with_sinks else None
    windows = [W, 0]
    bank = KVBank(L, Hq, H, D, cap=n + 8, windows=windows, **(dict(sinks=sinks) if with_sinks else {}))
    bank.state_init(n, 1 if keep else 2, 8)
    q, k, v = _mk(L, Hq, n, g, D), _mk(L, H, n, g, D), _mk(L, H, n, g, D)
    plan = StepPlan(policy="roco", phase="prefill", accumulate=keep, evict=False, stride=8)
    info = bank.step_info(plan, n)
    assert info["wide"] == 0 and info["qb_rows"] * rep <= 32, info
    out, _ = bank.attend(plan, q.cuda(), k.cuda(), v.cuda())
    assert bank.tokens_seen == n and bank.ordered_tok_pos().cpu()[0, 0].tolist() == list(range(n))
    dist = [0.0]
    for l in range(L):
        key_pos = torch.arange(n).expand(H, n)
        core = make_core(windows[l], key_pos, list(range(n)), sinks[l] if with_sinks else None, dist)
        o_ref, p = core(q[l:l + 1].float(), k[l:l + 1].float(), v[l:l + 1].float(), torch.full((n, n), float("-inf")).triu(1)[None, None])
        assert out_close(out[l].float().cpu(), o_ref[0]), (l, float((out[l].float().cpu() - o_ref[0]).abs().max()))
        if keep:      # (the bars of tests/test_hip_sink.py's dense prefix)
            pbar = p[0].view(H, rep, n, n).mean(1)
            S, Q = bank.score_sum.cpu(), bank.score_sq.cpu()
            assert torch.allclose(S[l, :, :n], pbar.sum(1), rtol=2e-5, atol=1e-6), (l, float((S[l, :, :n] - pbar.sum(1)).abs().max()))
            assert torch.allclose(Q[l, :, :n], (pbar ** 2).sum(1), rtol=2e-5, atol=1e-6), l
    assert dist[0] >= 1e-2, dist


# ---- (4) the driver ---------------------------------------------------------------------------------------------------------------------------
DRIVER_CASES = [
    # mode, stride, policy (the modes of tests/test_hip_sink.py's DRIVER_CASES; gpt-oss's shape class: head_dim 64, GQA x 8, sinks)
    ("decoding", 1, "roco"), ("decoding", 1, "h2o_head"), ("auto", 8, "roco"),
    ("encoding", 8, "tova"),      # the head-mean TOVA row of the encoding mode (easykv/easykv.py:456): rebuilt from logits with -inf columns
]
DRIVER_WINDOWS = [16, 0]


def _tie_probe():
    """The event probe of tests/test_hip_sink.py, which also calls a decision unstable when it moves under ABSOLUTE noise of 1e-9.  Under a
    window a strided prefill without keep_attention leaves every key that lies outside the window of all of a chunk's queries with a score
    of exactly 0: the victims among them are chosen by the tie rule alone (the reference's torch.topk promises no order among equal
    keys), and the relative noise of the probe leaves zeros tied, so it cannot see that those decisions are not well defined."""
    from tests.test_hip_sink import _EventProbe

    class TieProbe(_EventProbe):
        def __call__(self, fn, policy, s, q, c, args, ids):
            Probe.__call__(self, fn, policy, s, q, c, args, ids)
            base = torch.sort(ids, dim=-1)[0]
            for _ in range(2):
                alt = fn(policy, s + torch.rand(s.shape, generator=self.gen) * 1e-9, q + torch.rand(s.shape, generator=self.gen) * 1e-18, c.clone(), *args)
                alt = alt.unsqueeze(-1) if alt.dim() < ids.dim() else alt
                self.last_unstable |= (torch.sort(alt, dim=-1)[0] != base).any(dim=-1)
            self.events.append(self.last_unstable.clone())
    return TieProbe()


def run_driver_case(mode, stride, policy, oracle_only=False):
    """A 120-token prompt (longer than the window of 16 on layer 0) under a budget of 60, so the run evicts."""
    from oracle import easykv_oracle as O
    from oracle.fake_model import FakeAttnModel, make_streams
    from tests.golden_util import trace_events
    from tests.test_hip_generate_batch import _evictions, _ids
    D, Hq, length = 64, 16, 120
    sinks = torch.randn(2, Hq, generator=torch.Generator().manual_seed(11)) + 1
    cfg = dict(budget=60, kv_policy=policy, max_new_tokens=24, recent_ratio=0.3)
    if mode == "decoding":
        cfg = dict(budget=60, kv_policy=policy, max_new_tokens=84)
    streams = make_streams(2, Hq, 2, D, length + cfg["max_new_tokens"] + 8, seed=47)
    res = line = cache = None
    if not oracle_only:
        import easykv_amd
        from tests.native_fake_model import NativeFakeModel
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            res, cache = easykv_amd.generate(NativeFakeModel(*streams), _ids(length),
                                             dict(cfg, _record_evictions=True, attention_sinks=sinks, sliding_window=DRIVER_WINDOWS),
                                             kv_mode=mode, stride=stride, return_cache=True)
        line = buf.getvalue().strip()
        assert cache.windows == tuple(DRIVER_WINDOWS) and cache.bank.windows == cache.windows and torch.equal(cache.sinks.cpu(), sinks)
    probe, dist = _tie_probe(), [0.0]
    O.SELECT_HOOK = probe
    try:
        tr = O.generate(FakeAttnModel(*streams, core=model_core(DRIVER_WINDOWS, sinks, dist)), _ids(length), cfg, kv_mode=mode, stride=stride)
    finally:
        O.SELECT_HOOK = None
    kinds, ref, _ = trace_events(tr)
    assert len(ref) == len(probe.events) > 0 and not kinds.any(), (len(ref), len(probe.events))
    ours = _evictions(cache.evictions) if cache is not None else ref
    assert len(ours) == len(ref)
    alive = np.ones(ref[0].shape[:2], dtype=bool)
    n_checked = n_total = 0
    for e, (a, b) in enumerate(zip(ours, ref)):
        stable = ~probe.events[e].numpy()
        same = (a == b).all(-1)
        assert same[alive & stable].all(), (mode, policy, f"eviction ids differ at eviction {e}", a.tolist(), b.tolist())
        n_total += alive.size
        n_checked += int((alive & stable).sum())
        alive &= stable & same
    print(f"[window] generate {mode} {policy}: compared {n_checked} of {n_total} decisions; max |o_window - o_full| = {dist[0]:.3e}")
    assert n_checked >= 10 and 2 * n_checked >= n_total and dist[0] >= 1e-2, (n_checked, n_total, dist[0])
    if cache is not None:
        ref_text = tr.result if isinstance(tr.result, str) else " ".join(str(t) for t in tr.result)
        assert res == ref_text and line == tr.report.strip(), (res, ref_text, line, tr.report)
    return n_checked, n_total, dist[0]


@pytest.mark.parametrize("mode,stride,policy", DRIVER_CASES, ids=[f"{c[0]}-{c[2]}" for c in DRIVER_CASES])
def test_generate_on_a_window_sink_model_equals_the_window_oracles_run(mode, stride, policy):
    run_driver_case(mode, stride, policy)


# ---- (5) the seam ---------------------------------------------------------------------------------------------------------------------------
def test_stock_gpt_oss_with_a_sliding_window_through_the_seam():
    """gpt-oss with sliding_window = 8 on its first layer, a 40-token prompt.  The yardstick is the eager forward of a float32 copy of the
    same 16-bit-rounded weights; the bar is the one tests/test_hip_sink.py's test_stock_gpt_oss_through_the_seam derives: the seam's 3e-2
    on the logits, or twice the measured fp16-eager-to-fp32-eager distance where that is larger (printed).  With the windows of
    generation_config['sliding_window'] = 'model' the logits are inside the bar; without them — what the seam served before — they are
    outside it: this is the test that shows the feature matters."""
    import copy
    import transformers
    import easykv_amd
    from easykv_amd import api, hf
    from tests.test_hip_sink import BAR, _Tok
    torch.manual_seed(0)
    cfg = transformers.GptOssConfig(vocab_size=97, hidden_size=64, intermediate_size=64, num_hidden_layers=2, num_attention_heads=8,
                                    num_key_value_heads=2, head_dim=64, num_local_experts=2, num_experts_per_tok=1, max_position_embeddings=512,
                                    layer_types=["sliding_attention", "full_attention"], sliding_window=8, initializer_range=0.25,
                                    attn_implementation="eager")
    model16 = transformers.GptOssForCausalLM(cfg)
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for layer in model16.model.layers:
            layer.self_attn.sinks.copy_(torch.randn(8, generator=g))
    model16 = model16.half().eval()
    model32 = copy.deepcopy(model16).float().cuda()
    model = model16.cuda()
    ids = torch.randint(0, 97, (1, 40), device="cuda", generator=torch.Generator("cuda").manual_seed(5))
    with torch.inference_mode():
        ref_logits = model32(input_ids=ids).logits.float()
        own16 = model(input_ids=ids).logits.float()
        seq, ref_tokens, gaps = ids, [], []
        for _ in range(8):
            top2 = torch.topk(model32(input_ids=seq).logits[0, -1].float(), 2)
            ref_tokens.append(int(top2.indices[0]))
            gaps.append(float(top2.values[0] - top2.values[1]))
            seq = torch.cat([seq, top2.indices[:1].view(1, 1)], dim=1)
    d16 = float((own16 - ref_logits).abs().max())
    bar = BAR if d16 <= BAR else 2 * d16
    print(f"[window] gpt-oss, sliding_window 8: the model's own fp16 eager forward is {d16:.3e} from its fp32 forward (bar {bar:.3e})")
    hf.patch_model(model)
    easykv_amd.enable_fixed_kv(model, _Tok(), mode="decoding", stride=1)
    sinks = torch.stack([l.self_attn.sinks.detach().float() for l in model.model.layers])
    windows = api._collect_windows(model, dict(sliding_window="model"), 2)
    assert windows == [8, 0]
    pos = torch.arange(40, device="cuda").view(1, -1)
    dense = easykv_amd.StepPlan(policy="full", phase="prefill", accumulate=False)
    cache = easykv_amd.BudgetedKVCache(2, 8, 2, 64, 64, torch.device("cuda"), sinks=sinks, windows=windows)
    with torch.inference_mode(), cache.active(dense):
        got = model(input_ids=ids, past_key_values=cache, position_ids=pos, use_cache=True).logits.float()
    err = float((got - ref_logits).abs().max())
    plain = easykv_amd.BudgetedKVCache(2, 8, 2, 64, 64, torch.device("cuda"), sinks=sinks)
    with torch.inference_mode(), plain.active(dense):
        old = model(input_ids=ids, past_key_values=plain, position_ids=pos, use_cache=True).logits.float()
    moved = float((old - ref_logits).abs().max())
    print(f"[window] gpt-oss through the seam: max |logits - fp32 eager| = {err:.3e} with the windows, {moved:.3e} without them")
    assert torch.allclose(got, ref_logits, atol=bar, rtol=bar), err
    assert moved > bar, (moved, bar)      # without the key the seam serves another model
    # windows that are not the module's raise instead of computing another model
    for wrong in ([0, 8], [4, 0], [8, 8]):
        c2 = easykv_amd.BudgetedKVCache(2, 8, 2, 64, 64, torch.device("cuda"), sinks=sinks, windows=wrong)
        with torch.inference_mode(), c2.active(dense):
            with pytest.raises(ValueError, match="sliding window"):
                model(input_ids=ids, past_key_values=c2, position_ids=pos, use_cache=True)
    # the driver with the key: the model's own greedy tokens (a differing token only where the reference's top-2 margin is below the bar)
    gc = dict(temperature=1e-6, kv_policy="full", budget=200, max_new_tokens=8, eos_token_ids=[-1], sliding_window="model")
    with contextlib.redirect_stdout(io.StringIO()):
        out, cache = model.easykv_generate(input_ids=ids, generation_config=gc, return_cache=True)
    assert cache.windows == (8, 0) and cache.bank.tokens_seen >= 47
    toks = [int(t) for t in out.split()]
    for i, (t, r, gap) in enumerate(zip(toks, ref_tokens, gaps)):
        if t != r:
            assert gap < bar, (i, toks, ref_tokens, gaps)
            break
    # eviction under the key: auto mode at half the prompt, stride 8
    ids2 = torch.randint(0, 97, (1, 120), device="cuda", generator=torch.Generator("cuda").manual_seed(6))
    gc2 = dict(budget=60, kv_policy="roco", max_new_tokens=6, recent_ratio=0.3, eos_token_ids=[-1], temperature=1e-6, sliding_window="model")
    easykv_amd.enable_fixed_kv(model, _Tok(), mode="auto", stride=8)
    with contextlib.redirect_stdout(io.StringIO()):
        out, cache = model.easykv_generate(input_ids=ids2, generation_config=gc2, return_cache=True)
    _, idx, _ = easykv_amd.geometry("auto", 120, 60, 8)
    assert len(out.split()) == 6 and cache.get_seq_length() == idx
    for extra, match in ((dict(streaming=True), "streaming"), (dict(kv_quant="fp8"), "kv_quant"), (dict(long_rows=True), "long_rows"), (dict(hipgraph=True), "q_pos0")):
        with pytest.raises(ValueError, match=match):
            model.easykv_generate(input_ids=ids2, generation_config=dict(gc2, **extra))
    with pytest.raises(ValueError, match="generate_batch"):      # (the sinks of this model are refused first; the key alone: tests/test_window_cpu.py)
        model.easykv_generate_batch(input_ids_list=[ids2, ids2], generation_config=gc2)
