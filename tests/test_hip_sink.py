"""Attention sinks (gpt-oss: one learned logit per query head in every softmax) on the GPU: a KVBank(sinks=...) against a twin bank without
them, against the oracle with gpt-oss's eager attention as its `attention_core` (tests/sink_ref.py), the drivers over fake models and a
tiny stock GptOssForCausalLM through the seam.

(1) Twin banks, no tolerance.  With sinks = -1e4 everywhere the virtual key contributes exp -> 0 and M is the real maximum, so outputs,
victims, slot maps and score rows equal the plain call's on a twin bank bit for bit: decode steps on both score-row layouts and on the
split path, a one-pass and a two-pass chunk step (shapes whose plain call runs the same 16x16x32 build: more than 1024 rows, few heads).
(2) Decode steps against O.layer_step with the sink core at cache lengths T = 2 (where the sink dominates), 65 and 300, the last with the
key range split in 2 and in 3 (the sink must be counted exactly once), one-launch and split path.  Outputs under out_close (bf16: the bar of tests/test_hip_bf16.py), victims exact
wherever the Probe of tests/test_hip_fullsize.py calls the decision stable.
(3) Chunk steps, stride 8 and 16 onto about 200 cached rows: one pass with the kernel's tail, two passes with the generic scorer, and a
40-token dense prefix with keep_attention.
(4) easykv_amd.generate against O.generate: eviction ids under the probe, the printed line, the text.
(5) The seam: a stock GptOssForCausalLM against the eager forward of an fp32 copy of its 16-bit weights."""
import contextlib
import io

import numpy as np
import pytest
import torch

from tests.golden_util import out_close
from tests.sink_ref import make_core, model_core, patched
from tests.test_hip_d256 import _enough, _permutation, _ProbeAndCapture
from tests.test_hip_fullsize import Probe

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
FAR = -1.0e4      # a sink far below every logit: exp(FAR - M) is 0 in fp32


def _mk(L, H, n, g, d, dtype=torch.float16):
    return torch.randn(L, H, n, d, generator=g).to(dtype)


def _sinks(kind, L, Hq, seed=11):
    if kind == "randn+1":
        return torch.randn(L, Hq, generator=torch.Generator().manual_seed(seed)) + 1
    return torch.full((L, Hq), float(kind))


# ---- (1) twin banks -------------------------------------------------------------------------------------------------------------------------
def _same_state(a, b, what):
    for name in ("slot_of_pos", "score_sum", "score_sq", "score_cnt"):
        assert torch.equal(getattr(a, name), getattr(b, name)), (what, name)


TWIN_DECODE = [
    # id, D, Hq, H, L, budget, score_off = prompt rows (0: the whole cache, which 528 heads run on the slot-indexed layout), n_split, slot rows
    ("ordered_d64_gqa8_fused", 64, 16, 2, 2, 140, 5, 1, False),
    ("slot_rows_d128_528_heads", 128, 16, 16, 33, 70, 0, 0, True),
    ("split3_d64_gqa8", 64, 16, 2, 2, 420, 5, 3, False),
    ("split2_d128_mha_bf16", 128, 4, 4, 2, 300, 5, 2, False),
]


@pytest.mark.parametrize("name,D,Hq,H,L,budget,P,n_split,slot", TWIN_DECODE, ids=[c[0] for c in TWIN_DECODE])
def test_far_sinks_decode_steps_equal_the_plain_twin_bit_for_bit(name, D, Hq, H, L, budget, P, n_split, slot):
    from easykv_amd import KVBank, StepPlan
    dtype = BF if name.endswith("bf16") else torch.float16
    g = torch.Generator().manual_seed(52000 + D + budget)
    rows = budget if P == 0 else P
    k0, v0 = _mk(L, H, rows, g, D, dtype), _mk(L, H, rows, g, D, dtype)
    banks = [KVBank(L, Hq, H, D, cap=P + budget + 1 + (63 if slot else 0), dtype=dtype, **kw) for kw in ({}, dict(sinks=torch.full((L, Hq), FAR)))]
    for b in banks:
        b.load_rows(k0.cuda(), v0.cuda())
        b.state_init(budget + 1, 0)
    steps = 14 if P == 0 else budget + 12
    n_slot, n_fused, splits = 0, 0, set()
    for i in range(steps):
        q, k, v = _mk(L, Hq, 1, g, D, dtype).cuda(), _mk(L, H, 1, g, D, dtype).cuda(), _mk(L, H, 1, g, D, dtype).cuda()
        evict = banks[0].n_slots[0] + 1 - P > budget
        plan = StepPlan(policy="roco", phase="decode", evict=evict, score_off=P, budget=budget, n_split=n_split)
        infos = [b.step_info(plan, 1) for b in banks]
        assert {k_: infos[0][k_] for k_ in ("n_split", "fused", "n_launches")} == {k_: infos[1][k_] for k_ in ("n_split", "fused", "n_launches")}, (name, i, infos)
        assert infos[1]["fused_order"] == 0, infos[1]      # the sink instances run phase order F
        n_fused += infos[1]["fused"]
        splits.add(infos[1]["n_split"])
        (o0, i0), (o1, i1) = (b.attend(plan, q, k, v) for b in banks)
        n_slot += int(all(banks[1]._slot_rows))
        assert torch.equal(o0, o1), (name, i, float((o0.float() - o1.float()).abs().max()))
        assert (i0 is None and i1 is None) or torch.equal(i0, i1), (name, i)
        if not slot and i % 16 == 0:      # (reading the state of a slot-indexed bank converts it back: only at the end there)
            _same_state(banks[0], banks[1], (name, i))
    if slot:
        assert n_slot == steps, n_slot
    elif n_split > 1:
        assert 0 < n_fused < steps and n_split in splits, (name, n_fused, splits)      # one launch while the cache is short, then the split path
    _same_state(banks[0], banks[1], name)
    _permutation(banks[1])


TWIN_CHUNK = [
    # id, D, Hq, H, stride, cached rows, plan keywords, what the plan must say
    ("one_pass_tail_d64_gqa8", 64, 16, 2, 4, 1500, dict(n_split=1), dict(fused=1, two_pass=0, n_launches=1)),
    ("two_pass_split2_d64_gqa8", 64, 16, 2, 4, 1500, dict(n_split=2, two_pass=1), dict(fused=0, two_pass=1, n_split=2)),
    ("one_pass_split_d128_mha", 128, 4, 4, 8, 1500, dict(), dict(fused=0, two_pass=0)),
    ("two_pass_d128_mha_bf16", 128, 4, 4, 8, 1500, dict(two_pass=1), dict(fused=0, two_pass=1)),
    # the head-mean TOVA row (encoding / ppl mode): rebuilt from the exported logits by the sink build of its kernel
    ("tova_head_mean_d64_gqa8", 64, 16, 2, 4, 1500, dict(policy="tova", tova_head_mean=True), dict(two_pass=0)),
    ("tova_head_mean_d128_mha", 128, 4, 4, 8, 1500, dict(policy="tova", tova_head_mean=True, n_split=2), dict(two_pass=0, n_split=2)),
]


@pytest.mark.parametrize("name,D,Hq,H,s,idx,kw,expect", TWIN_CHUNK, ids=[c[0] for c in TWIN_CHUNK])
def test_far_sinks_chunk_steps_equal_the_plain_twin_bit_for_bit(name, D, Hq, H, s, idx, kw, expect):
    from easykv_amd import KVBank, StepPlan
    dtype = BF if name.endswith("bf16") else torch.float16
    L = 2
    g = torch.Generator().manual_seed(52500 + D + s)
    k0, v0 = _mk(L, H, idx, g, D, dtype), _mk(L, H, idx, g, D, dtype)
    banks = [KVBank(L, Hq, H, D, cap=idx + s, dtype=dtype, **x) for x in ({}, dict(sinks=torch.full((L, Hq), FAR)))]
    for b in banks:
        b.load_rows(k0.cuda(), v0.cuda())
        b.state_init(idx + s, 2, s)
    plan = StepPlan(**dict(dict(policy="roco", phase="prefill", accumulate=True, evict=True, budget=idx + s // 2, recent=int(idx * 0.2), sink=4,
                                stride=s, tova_head_mean=False), **kw))
    for step in range(3):
        q, k, v = _mk(L, Hq, s, g, D, dtype).cuda(), _mk(L, H, s, g, D, dtype).cuda(), _mk(L, H, s, g, D, dtype).cuda()
        infos = [b.step_info(plan, s) for b in banks]
        assert infos[0] == infos[1] and infos[1]["wide"] == 0, (name, infos)      # the plain call runs the same build of the same kernel
        assert all(infos[1][k_] == v_ for k_, v_ in expect.items()), (name, infos[1])
        (o0, i0), (o1, i1) = (b.attend(plan, q, k, v) for b in banks)
        assert torch.equal(o0, o1), (name, step, float((o0.float() - o1.float()).abs().max()))
        assert torch.equal(i0, i1), (name, step)
        _same_state(banks[0], banks[1], (name, step))
    _permutation(banks[1])


# ---- (2) decode steps against the oracle ------------------------------------------------------------------------------------------------
def _bf16_close(out, ref, pv):
    """The bf16 bar of tests/test_hip_bf16.py: |o - ref| <= 2^-8 (|ref| + pv) + 1e-6 pv, pv = p.|V| of the reference's probabilities."""
    err = (out - ref).abs()
    return bool(torch.isfinite(out).all()) and bool((err <= 2.0 ** -8 * (ref.abs() + pv) + 1e-6 * pv).all())


DECODE_CASES = [
    # id, D, Hq, H, policy, n_split, dtype, sinks, expected path (True: one launch throughout, None: one launch, then the split path)
    ("d64_gqa8_roco_fused_randn", 64, 16, 2, "roco", 1, torch.float16, "randn+1", True),
    ("d64_gqa8_h2o_split2_plus8", 64, 16, 2, "h2o_head", 2, torch.float16, 8.0, None),
    ("d64_gqa8_tova_split3_minus8_bf16", 64, 16, 2, "tova", 3, BF, -8.0, None),
    ("d128_mha_roco_split3_plus8", 128, 4, 4, "roco", 3, torch.float16, 8.0, None),
    ("d128_mha_tova_fused_minus8", 128, 4, 4, "tova", 1, torch.float16, -8.0, True),
    ("d128_gqa4_h2o_split2_randn_bf16", 128, 8, 2, "h2o_head", 2, BF, "randn+1", None),
    ("d128_gqa4_roco_split2_randn", 128, 8, 2, "roco", 2, torch.float16, "randn+1", None),
    ("d128_gqa4_h2o_fused_plus8_bf16", 128, 8, 2, "h2o_head", 1, BF, 8.0, True),
]


def run_decode_case(name, D, Hq, H, policy, n_split, dtype, kind, one_launch, oracle_only=False):
    """Whole-cache decode steps (score_off = 0) at cache lengths T = 2 (one accumulating step onto a 1-row cache: the sink dominates), 65
    and 300 (six evicting steps each; the forced split count applies at 300, where a key range holds at least 100 rows)."""
    from oracle import easykv_oracle as O
    L, rep = 2, Hq // H
    sinks = _sinks(kind, L, Hq)
    g = torch.Generator().manual_seed(53000 + D + Hq + n_split)
    probe = Probe()
    n_checked = n_total = 0
    dist, paths = [0.0], set()
    for T in (2, 65, 300):
        budget, evict, steps = T - 1, T > 2, (6 if T > 2 else 1)
        k0, v0 = _mk(L, H, budget, g, D, dtype), _mk(L, H, budget, g, D, dtype)
        warm = torch.rand(L, H, T, generator=g) * 1e-3
        warm[:, :, budget:] = 0      # (the column of the row about to be appended starts empty)
        bank = None
        if not oracle_only:
            from easykv_amd import KVBank, StepPlan
            bank = KVBank(L, Hq, H, D, cap=T + 8, dtype=dtype, sinks=sinks)
            bank.load_rows(k0.cuda(), v0.cuda())
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
                if bank is not None:
                    plan = StepPlan(n_split=n_split, **kw)
                    info = bank.step_info(plan, 1)
                    want_fused = True if (one_launch or T < 300) else False
                    assert bool(info["fused"]) == want_fused and (want_fused or info["n_split"] == n_split), (name, T, info)
                    paths.add(bool(info["fused"]))
                    out, ids = bank.attend(plan, q.cuda(), k.cuda(), v.cuda())
                for l in range(L):
                    qf, kf, vf = q[l:l + 1].float(), k[l:l + 1].float(), v[l:l + 1].float()
                    pv = None
                    if bank is not None and dtype is BF:
                        pv = make_core(sinks[l])(qf, torch.cat([sts[l].k, kf], 2), torch.cat([sts[l].v, vf], 2).abs())[0][0]
                    with patched(sinks[l], dist):
                        o_ref, ids_ref = O.layer_step(sts[l], qf, kf, vf, O.StepPlan(**kw))
                    if bank is not None:
                        rows = alive[l].repeat_interleave(rep)
                        got_o, ref_o = out[l].float().cpu(), o_ref[0]
                        close = out_close(got_o[rows], ref_o[rows]) if dtype is not BF else _bf16_close(got_o[rows], ref_o[rows], pv[rows])
                        assert close, (name, T, i, l, float((got_o[rows] - ref_o[rows]).abs().max()))
                    if evict:
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
            if not evict:      # T = 2: the accumulated rows are the sink oracle's probabilities (the real keys' mass is below 1)
                S = bank.score_sum.cpu()
                for l in range(L):
                    assert torch.allclose(S[l, :, :T], sts[l].s[:, :T], rtol=2e-5, atol=1e-7), (name, l, S[l, :, :T], sts[l].s[:, :T])
            _permutation(bank)
    if not oracle_only and one_launch is None:
        assert paths == {True, False}, (name, paths)      # the one-launch kernel at 2 and 65 rows, the split path at 300
    print(f"[sink] {name}: max |o_sink - o_plain| of the oracle over the run = {dist[0]:.3e}")
    if kind != -8.0:
        assert dist[0] >= 1e-2, (name, dist[0])      # a path that ignores the sinks cannot pass (a sink at -8 is nearly invisible by design)
    _enough(name, n_checked, n_total)
    return n_checked, n_total, dist[0]


@pytest.mark.parametrize("name,D,Hq,H,policy,n_split,dtype,kind,one_launch", DECODE_CASES, ids=[c[0] for c in DECODE_CASES])
def test_sink_decode_steps_against_the_oracle(name, D, Hq, H, policy, n_split, dtype, kind, one_launch):
    run_decode_case(name, D, Hq, H, policy, n_split, dtype, kind, one_launch)


# ---- (3) chunk steps ------------------------------------------------------------------------------------------------------------------------
CHUNK_CASES = [
    # id, D, Hq, H, stride, cached rows, policy, two_pass, n_split, sinks, what the plan must say
    ("d64_gqa8_s4_one_pass_tail", 64, 16, 2, 4, 200, "roco", -1, 1, "randn+1", dict(fused=1, two_pass=0, n_qblocks=1)),
    ("d64_gqa8_s8_two_pass_two_blocks", 64, 16, 2, 8, 200, "roco", 0, 0, "randn+1", dict(fused=0, two_pass=1, n_qblocks=2)),
    ("d64_gqa8_s16_two_pass_h2o", 64, 16, 2, 16, 210, "h2o_head", 0, 0, 8.0, dict(fused=0, two_pass=1, n_qblocks=4)),
    ("d128_mha_s8_one_pass_tail_tova", 128, 4, 4, 8, 200, "tova", -1, 1, -8.0, dict(fused=1, two_pass=0)),
    ("d128_gqa4_s16_two_pass_split2", 128, 8, 2, 16, 205, "roco", 1, 2, "randn+1", dict(fused=0, two_pass=1, n_split=2)),
    ("d128_gqa4_s8_one_pass_split2", 128, 8, 2, 8, 200, "h2o_head", -1, 2, 8.0, dict(fused=0, two_pass=0, n_split=2)),
]


def run_chunk_case(name, D, Hq, H, s, idx, policy, two_pass, n_split, kind, expect, oracle_only=False):
    from oracle import easykv_oracle as O
    from tests.select_rule import feasible_classes, valid_victims
    rep, L, n_steps = Hq // H, 2, 4
    budget_p, recent, sink = idx + s // 2, int(idx * 0.2), 4
    g = torch.Generator().manual_seed(53700 + D + s + idx)
    k0, v0 = _mk(L, H, idx, g, D), _mk(L, H, idx, g, D)
    sinks = _sinks(kind, L, Hq)
    bank = None
    if not oracle_only:
        from easykv_amd import KVBank, StepPlan
        bank = KVBank(L, Hq, H, D, cap=idx + s, sinks=sinks)
        bank.load_rows(k0.cuda(), v0.cuda())
        bank.state_init(idx + s, 2, s)
    sts = []
    for l in range(L):
        st = O.LayerState(k=k0[l:l + 1].float(), v=v0[l:l + 1].float())
        st.s, st.q, st.c = O.init_state_prefill((H,), idx, s, False)
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
            kw = dict(policy=policy, phase="prefill", accumulate=True, evict=True, budget=budget_p, recent=recent, sink=sink, stride=s,
                      tova_head_mean=False)
            if bank is not None:
                plan = StepPlan(two_pass=two_pass, n_split=n_split, **kw)
                info = bank.step_info(plan, s)
                assert info["wide"] == 0 and info["qb_rows"] * rep <= 32 and info["n_qblocks"] == -(-s // info["qb_rows"]), (name, info)
                assert all(info[k_] == v_ for k_, v_ in expect.items()), (name, info)
                out, ids = bank.attend(plan, q.cuda(), k.cuda(), v.cuda())
            for l in range(L):
                if not bool(alive[l].any()):
                    continue
                with patched(sinks[l], dist):
                    o_ref, ids_ref = O.layer_step(sts[l], q[l:l + 1].float(), k[l:l + 1].float(), v[l:l + 1].float(), O.StepPlan(**kw))
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
        assert bank.n_slots == [idx] * L
        _permutation(bank)
    print(f"[sink] {name}: max |o_sink - o_plain| of the oracle over the run = {dist[0]:.3e}")
    if kind != -8.0:
        assert dist[0] >= 1e-2, (name, dist[0])
    _enough(name, n_checked, n_steps * L * H)
    return n_checked, n_steps * L * H


@pytest.mark.parametrize("name,D,Hq,H,s,idx,policy,two_pass,n_split,kind,expect", CHUNK_CASES, ids=[c[0] for c in CHUNK_CASES])
def test_sink_chunk_steps_against_the_oracle(name, D, Hq, H, s, idx, policy, two_pass, n_split, kind, expect):
    run_chunk_case(name, D, Hq, H, s, idx, policy, two_pass, n_split, kind, expect)


@pytest.mark.parametrize("D,Hq,H", [(64, 16, 2), (128, 4, 4)], ids=["d64_gqa8", "d128_mha"])
def test_sink_dense_prefix_with_keep_attention(D, Hq, H):
    """A 40-token dense prefix whose probabilities seed the score rows (keep_attention): outputs under out_close, and the accumulated
    S / Q rows against the column sums of the sink oracle's probabilities (GQA mean over the group, as easykv/easykv.py:173-196)."""
    from easykv_amd import KVBank, StepPlan
    L, n, rep = 2, 40, Hq // H
    g = torch.Generator().manual_seed(53900 + D)
    q, k, v = _mk(L, Hq, n, g, D), _mk(L, H, n, g, D), _mk(L, H, n, g, D)
    sinks = _sinks("randn+1", L, Hq)
    bank = KVBank(L, Hq, H, D, cap=n + 24, sinks=sinks)
    bank.state_init(n, 1, 8)
    plan = StepPlan(policy="roco", phase="prefill", accumulate=True, evict=False, stride=8)
    info = bank.step_info(plan, n)
    assert info["wide"] == 0 and info["qb_rows"] * rep <= 32, info
    out, _ = bank.attend(plan, q.cuda(), k.cuda(), v.cuda())
    mask = torch.full((n, n), float("-inf")).triu(1)[None, None]
    S, Q = bank.score_sum.cpu(), bank.score_sq.cpu()
    moved = 0.0
    for l in range(L):
        o_ref, p = make_core(sinks[l])(q[l:l + 1].float(), k[l:l + 1].float(), v[l:l + 1].float(), mask)
        o_plain, _ = make_core(None)(q[l:l + 1].float(), k[l:l + 1].float(), v[l:l + 1].float(), mask)
        moved = max(moved, float((o_ref - o_plain).abs().max()))
        assert out_close(out[l].float().cpu(), o_ref[0]), (l, float((out[l].float().cpu() - o_ref[0]).abs().max()))
        pbar = p[0].view(H, rep, n, n).mean(1)
        assert torch.allclose(S[l, :, :n], pbar.sum(1), rtol=2e-5, atol=1e-6), (l, float((S[l, :, :n] - pbar.sum(1)).abs().max()))
        assert torch.allclose(Q[l, :, :n], (pbar ** 2).sum(1), rtol=2e-5, atol=1e-6), l
    assert moved >= 1e-2, moved


# ---- (4) the drivers --------------------------------------------------------------------------------------------------------------------------
class _EventProbe(Probe):
    """The stability probe, one mask [L, H] per eviction event of oracle.generate."""

    def __init__(self):
        super().__init__()
        self.events = []

    def __call__(self, *args):
        super().__call__(*args)
        self.events.append(self.last_unstable.clone())


DRIVER_CASES = [
    # mode, stride, head_dim, query heads, policy
    ("decoding", 1, 64, 16, "roco"), ("decoding", 1, 64, 16, "h2o_head"), ("decoding", 1, 128, 8, "tova"), ("auto", 8, 64, 16, "roco"),
    ("encoding", 8, 64, 16, "tova"),      # the head-mean TOVA row of the encoding mode (easykv/easykv.py:456)
]


@pytest.mark.parametrize("mode,stride,D,Hq,policy", DRIVER_CASES, ids=[f"{c[0]}-d{c[2]}-{c[4]}" for c in DRIVER_CASES])
def test_generate_on_a_sink_model_equals_the_sink_oracles_run(mode, stride, D, Hq, policy):
    import easykv_amd
    from oracle import easykv_oracle as O
    from oracle.fake_model import FakeAttnModel, make_streams
    from tests.golden_util import trace_events
    from tests.native_fake_model import NativeFakeModel
    from tests.test_hip_generate_batch import _evictions, _ids
    length = 120
    sinks = torch.randn(2, Hq, generator=torch.Generator().manual_seed(11)) + 1
    cfg = dict(budget=60, kv_policy=policy, max_new_tokens=24, recent_ratio=0.3)
    if mode == "decoding":
        cfg = dict(budget=60, kv_policy=policy, max_new_tokens=84)
    streams = make_streams(2, Hq, 2, D, length + cfg["max_new_tokens"] + 8, seed=43)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        res, cache = easykv_amd.generate(NativeFakeModel(*streams), _ids(length), dict(cfg, _record_evictions=True, attention_sinks=sinks),
                                         kv_mode=mode, stride=stride, return_cache=True)
    line = buf.getvalue().strip()
    assert torch.equal(cache.sinks.cpu(), sinks) and cache.bank.sinks is cache.sinks and cache.sinks.dtype == torch.float32
    probe, dist = _EventProbe(), [0.0]
    O.SELECT_HOOK = probe
    try:
        tr = O.generate(FakeAttnModel(*streams, core=model_core(sinks, dist)), _ids(length), cfg, kv_mode=mode, stride=stride)
    finally:
        O.SELECT_HOOK = None
    ours = _evictions(cache.evictions)
    kinds, ref, _ = trace_events(tr)
    assert len(ours) == len(ref) == len(probe.events) > 0 and not kinds.any(), (len(ours), len(ref), len(probe.events))
    alive = np.ones(ours[0].shape[:2], dtype=bool)
    n_checked = n_total = 0
    for e, (a, b) in enumerate(zip(ours, ref)):
        stable = ~probe.events[e].numpy()
        same = (a == b).all(-1)
        assert same[alive & stable].all(), (mode, D, policy, f"eviction ids differ at eviction {e}")
        n_total += alive.size
        n_checked += int((alive & stable).sum())
        alive &= stable & same
    print(f"[sink] generate {mode} d{D} {policy}: compared {n_checked} of {n_total} decisions; max |o_sink - o_plain| = {dist[0]:.3e}")
    assert n_checked >= 10 and 2 * n_checked >= n_total and dist[0] >= 1e-2
    ref_text = tr.result if isinstance(tr.result, str) else " ".join(str(t) for t in tr.result)
    assert res == ref_text and line == tr.report.strip(), (res, ref_text, line, tr.report)


# ---- (5) the seam ---------------------------------------------------------------------------------------------------------------------------
BAR = 3e-2      # the seam's logit bar (tests/test_hip_hf_adapter.py)


class _Tok:
    eos_token_id = -1

    def decode(self, ids, skip_special_tokens=True):
        return " ".join(str(i) for i in ids)


def _tiny_gpt_oss(seed=0):
    import transformers
    torch.manual_seed(seed)
    cfg = transformers.GptOssConfig(vocab_size=97, hidden_size=64, intermediate_size=64, num_hidden_layers=2, num_attention_heads=8,
                                    num_key_value_heads=2, head_dim=64, num_local_experts=2, num_experts_per_tok=1, max_position_embeddings=512,
                                    layer_types=["sliding_attention", "full_attention"], sliding_window=256, initializer_range=0.25,
                                    attn_implementation="eager")
    model = transformers.GptOssForCausalLM(cfg)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for layer in model.model.layers:      # (the sinks are re-drawn N(0, 1))
            layer.self_attn.sinks.copy_(torch.randn(8, generator=g))
    return model.half().eval()


def test_stock_gpt_oss_through_the_seam():
    """The yardstick is the eager forward of a float32 copy of the same 16-bit-rounded weights (gpt-oss's eager softmax runs in the
    model's dtype).  The bar is the seam's 3e-2 on the logits; only if the model's own fp16 eager forward is farther than that from its
    fp32 forward, twice that measured distance (printed; DESIGN.md §8 records it)."""
    import copy
    import easykv_amd
    from easykv_amd import hf
    model16 = _tiny_gpt_oss()
    model32 = copy.deepcopy(model16).float().cuda()
    model = model16.cuda()
    assert type(model).__name__ == "GptOssForCausalLM" and model.model.layers[0].self_attn.sinks.numel() == 8
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
        saved = [l.self_attn.sinks.data.clone() for l in model32.model.layers]
        for l in model32.model.layers:
            l.self_attn.sinks.data.fill_(-1e4)
        no_sinks = model32(input_ids=ids).logits.float()
        for l, s in zip(model32.model.layers, saved):
            l.self_attn.sinks.data.copy_(s)
    d16 = float((own16 - ref_logits).abs().max())
    bar = BAR if d16 <= BAR else 2 * d16
    moved = float((no_sinks - ref_logits).abs().max())
    print(f"[sink] gpt-oss: the model's own fp16 eager forward is {d16:.3e} from its fp32 forward (bar {bar:.3e}); removing the sinks moves the "
          f"fp32 eager logits by {moved:.3f}")
    assert moved >= 10 * bar, (moved, bar)      # the model is one the old seam computed wrongly
    hf.patch_model(model)
    easykv_amd.enable_fixed_kv(model, _Tok(), mode="decoding", stride=1)
    sinks = torch.stack([l.self_attn.sinks.detach().float() for l in model.model.layers])
    pos = torch.arange(40, device="cuda").view(1, -1)
    dense = easykv_amd.StepPlan(policy="full", phase="prefill", accumulate=False)
    cache = easykv_amd.BudgetedKVCache(2, 8, 2, 64, 64, torch.device("cuda"), sinks=sinks)
    with torch.inference_mode(), cache.active(dense):
        got = model(input_ids=ids, past_key_values=cache, position_ids=pos, use_cache=True).logits.float()
    err = float((got - ref_logits).abs().max())
    print(f"[sink] gpt-oss through the seam: max |logits - fp32 eager| = {err:.3e}")
    assert torch.allclose(got, ref_logits, atol=bar, rtol=bar), err
    # a cache without sinks, and one with another layer's rows, raise instead of computing another model
    for kw in (dict(), dict(sinks=sinks.flip(0))):
        wrong = easykv_amd.BudgetedKVCache(2, 8, 2, 64, 64, torch.device("cuda"), **kw)
        with torch.inference_mode(), wrong.active(dense):
            with pytest.raises(ValueError, match="easykv_amd attention"):
                model(input_ids=ids, past_key_values=wrong, position_ids=pos, use_cache=True)
    with contextlib.redirect_stdout(io.StringIO()):
        out, cache = model.easykv_generate(input_ids=ids, generation_config=dict(temperature=1e-6, kv_policy="full", budget=200, max_new_tokens=8, eos_token_ids=[-1]),
                                           return_cache=True)
    assert torch.allclose(cache.sinks.cpu(), sinks.cpu())      # collected from the model's modules by the driver
    toks = [int(t) for t in out.split()]
    for i, (t, r, gap) in enumerate(zip(toks, ref_tokens, gaps)):
        if t != r:
            assert gap < bar, (i, toks, ref_tokens, gaps)      # a differing token only where the reference's top-2 margin is below the bar
            break
    # eviction: auto mode at half the prompt, stride 8
    ids2 = torch.randint(0, 97, (1, 120), device="cuda", generator=torch.Generator("cuda").manual_seed(6))
    gc = dict(budget=60, kv_policy="roco", max_new_tokens=6, recent_ratio=0.3, eos_token_ids=[-1], temperature=1e-6)
    easykv_amd.enable_fixed_kv(model, _Tok(), mode="auto", stride=8)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        out, cache = model.easykv_generate(input_ids=ids2, generation_config=gc, return_cache=True)
    bp, idx, _ = easykv_amd.geometry("auto", 120, 60, 8)
    assert len(out.split()) == 6 and cache.get_seq_length() == idx
    line = buf.getvalue().strip()
    assert line.startswith("KV Cache Budget ratio") and line.endswith(f"[{idx}/(120+6)]") and "\n" not in line, line
    for extra, match in ((dict(streaming=True), "streaming"), (dict(kv_quant="fp8"), "kv_quant"), (dict(long_rows=True), "long_rows")):
        with pytest.raises(ValueError, match=match):
            model.easykv_generate(input_ids=ids2, generation_config=dict(gc, **extra))
    with pytest.raises(ValueError, match="attention sinks"):
        model.easykv_generate_batch(input_ids_list=[ids2, ids2], generation_config=gc)
