"""Batched decode steps on 16-bit-key / MXFP4-value rows ("kv164 batches", include/easykv_hip.h) on the GPU, by the scheme of
tests/test_hip_batch_kv164.py:

(a) a uniform table is the kv164 multi-layer step, bit for bit;
(b) ragged tables with 2, 17, 96, 300 and 2049 slots (tests/batch_kv6_cases.py) and mixed n_evict against the oracle per entry on the
    bank's own contents, one launch and split;
(c) the 16-bit twin of one ragged table: equal victims, slot maps, score rows and K rows, with no tolerance;
(d) adopt() does not mix formats, and a batch created in the format never holds a 16-bit V; (e) generate_batch equals the solo runs,
    and evicts what the unquantised 16-bit run evicts."""
import contextlib
import io

import numpy as np
import pytest
import torch

from tests import batch_kv6_cases as cases
from tests import kv4_ref
from tests.golden_util import out_close
from tests.test_hip_batch_kv6 import _evictions, _ids, _oracle_states, _solo_bank
from tests.test_hip_fullsize import Probe

pytestmark = pytest.mark.gpu
BF, F16 = torch.bfloat16, torch.float16
PLANES = ("k", "v4", "v_exp")      # (k: the 16-bit rows, kept)
Q = "k16_mxfp4"
DECISION = ("slot_of_pos", "score_sum", "score_sq", "score_cnt", "k")


# ---- (a) uniform --------------------------------------------------------------------------------------------------------------------
UNIFORM = [
    # id, Hq, H, B, rows, policy, dtype, n_split, one launch?   (head_dim 128 throughout)
    ("fused8_roco", 32, 32, 8, 300, "roco", F16, 0, True),                  # B * H = 256: the 8-wave one-launch build
    ("fused4_gqa8_tova_bf16", 16, 2, 4, 700, "tova", BF, 1, True),          # explicit n_split = 1: the 4-wave build, GQA x 8
    ("fused4_gqa3_h2o", 6, 2, 3, 200, "h2o_head", F16, 1, True),            # the padded GQA x 3 build
    ("split_h2o_fold", 4, 4, 3, 700, "h2o_head", F16, 4, False),            # split path, in-kernel fold
    ("recency", 4, 4, 2, 500, "recency", F16, 0, False),                    # range compaction
]


@pytest.mark.parametrize("name,Hq,H,B,rows,policy,dtype,n_split,one_launch", UNIFORM, ids=[c[0] for c in UNIFORM])
def test_uniform_kv164_batch_is_the_kv164_multi_layer_step_bit_for_bit(name, Hq, H, B, rows, policy, dtype, n_split, one_launch):
    from easykv_amd import KVBank, KVBankBatch, StepPlan
    from tests.test_hip_batch import _copy_layer, _fill
    D = 128
    g = torch.Generator().manual_seed(16400 + rows + B)
    T = rows + 1
    ref = KVBank(B, Hq, H, D, cap=T + 6, dtype=dtype)
    ref.use_slot_rows = False      # like against like: a batch runs the ordered score-row layout
    ref.k.zero_(), ref.v.zero_()
    for l in range(B):
        _fill(ref, l, rows, g, T)
    LPS, layer = 3, 1
    bat = KVBankBatch(B, LPS, Hq, H, D, cap=T + 6, dtype=dtype)
    bat.bank.k.zero_(), bat.bank.v.zero_()
    order = [(5 * i + 2) % B for i in range(B)] if B % 5 else list(reversed(range(B)))
    for i, s in enumerate(order):
        _copy_layer(ref, i, bat.bank, s * LPS + layer)
    ref.quantize_k16_mxfp4()
    assert bat.quantize_k16_mxfp4() is bat and bat.kv_quant == Q and bat.bank.v is None and bat.bank.k is not None
    plan = StepPlan(policy=policy, phase="decode", evict=True, score_off=0, budget=rows - 3, n_split=n_split, range_start=7 if policy == "recency" else -1)
    info = bat.step_info([plan] * B, layer, order, n_split)
    assert info == ref.step_info(plan, 1, 0, B), (info, ref.step_info(plan, 1, 0, B))
    assert bool(info["fused"]) == one_launch and info["n_launches"] >= 1 and info["fused_order"] == 0, info
    if n_split > 1:
        assert info["n_split"] > 1, info
    for step in range(3):
        q, k, v = (torch.randn(B, hh, 1, D, generator=g).to(dtype).cuda() for hh in (Hq, H, H))
        o1, ids1 = ref.attend(plan, q, k, v)
        o2, ids2 = bat.attend([plan] * B, q, k, v, layer, active=order, n_split=n_split)
        torch.cuda.synchronize()
        assert torch.equal(o1, o2), (name, step, float((o1.float() - o2.float()).abs().max()))
        assert torch.equal(ids1, ids2), (name, step)
        for i, s in enumerate(order):
            lb = s * LPS + layer
            assert bat.bank.n_slots[lb] == ref.n_slots[i] and bat.bank.extent[lb] == ref.extent[i]
            for arr in ("slot_of_pos", "score_sum", "score_sq", "score_cnt") + PLANES:
                assert torch.equal(getattr(bat.bank, arr)[lb], getattr(ref, arr)[i]), (name, step, i, arr)
        assert int(bat.bank.arrive.abs().sum()) == 0
    for s in range(B):      # the other layers were never touched: planes as allocated
        for l in (0, 2):
            lb = s * LPS + l
            assert bat.bank.n_slots[lb] == 0 and not bool(bat.bank.k[lb].any()) and not bool(bat.bank.v4[lb].any())
            assert bool((bat.bank.v_exp[lb] == 127).all())


# ---- (b) ragged tables against the oracle on the bank's own contents --------------------------------------------------------------------
class _Check:
    """tests.test_hip_batch_kv6._Check for kv164 planes: batched steps, every entry held to the oracle on the bank's own contents."""

    def __init__(self, bat):
        self.bat, self.bank = bat, bat.bank
        self.states = {}
        self.probe = Probe()
        self.n_dec = self.n_stable = self.n_reseed = 0
        self.worst = 0.0

    def step(self, tag, layers, plans, oplans, widths, q, k, v, n_split=0, fresh=()):
        from oracle import easykv_oracle as O
        bat, bank = self.bat, self.bank
        H, D = bank.n_kv_heads, bank.head_dim
        rows = torch.arange(H)
        need = {l: widths[r] for r, l in enumerate(layers) if l not in self.states or l in fresh}
        self.states.update(_oracle_states(bank, need))
        before = [(bank.n_slots[l], bank.extent[l]) for l in layers]
        new_row = torch.stack([bank._slot_of_pos[l, :, bank.n_slots[l]] for l in layers]).cpu().long()
        out, ids = bat.attend(plans, q.cuda(), k.cuda(), v.cuda(), 0, active=layers, n_split=n_split)
        torch.cuda.synchronize()
        assert out.dtype == bank.dtype and int(bank.arrive.abs().sum()) == 0
        O.SELECT_HOOK = self.probe
        try:
            for r, l in enumerate(layers):
                plan = plans[r]
                # the appended row: K as it came, bit for bit, V by the kv4 rule, at the row the free list named
                assert torch.equal(bank.k[l][rows, new_row[r]].cpu().view(torch.int16), k[r, :, 0].view(torch.int16)), (tag, l, "appended K")
                kv4_ref.check_rows(v[r, :, 0], bank.v4[l][rows, new_row[r]], bank.v_exp[l][rows, new_row[r]], (tag, l))
                kd, vd = bank.dequantized_rows(l)
                kq, vq = kd[rows, new_row[r]].cpu().view(1, H, 1, D), vd[rows, new_row[r]].cpu().view(1, H, 1, D)
                o_ref, ids_ref = O.layer_step(self.states[l], q[r:r + 1].float(), kq, vq, oplans[r])
                err = float((out[r].float().cpu() - o_ref[0]).abs().max())
                self.worst = max(self.worst, err)
                assert out_close(out[r].float().cpu(), o_ref[0]), (tag, l, err)
                T, ext = before[r][0] + 1, before[r][1]
                if plan.evict:
                    unstable = self.probe.last_unstable
                    got = ids[r, :, 0].cpu().long() - plan.score_off      # (the library reports cache positions)
                    same = got == ids_ref[:, 0]
                    self.n_dec += H
                    self.n_stable += int((~unstable).sum())
                    assert bool(same[~unstable].all()), (tag, l, got.tolist(), ids_ref[:, 0].tolist())
                    if not bool(same.all()):
                        self.states.pop(l)
                        self.n_reseed += 1
                assert bank.n_slots[l] == (T - 1 if plan.evict else T) and bank.extent[l] == max(ext, T), (tag, l, bank.n_slots[l], bank.extent[l])
        finally:
            O.SELECT_HOOK = None
        return out, ids


def _ragged(shape, draw, policy, kind, n_split):
    from easykv_amd import KVBankBatch, StepPlan
    D, Hq, H, dtype = cases.SHAPES[shape]
    entries, tokens = cases.inputs(shape, draw)
    bat = KVBankBatch(len(entries), 1, Hq, H, D, cap=2049 + 40, dtype=dtype)
    for i, e in enumerate(entries):
        cases.fill_entry(bat.bank, i, e)
    if kind is not None:
        bat.quantize(kind)
    plans = [StepPlan(**cases.plan_kw(e, policy)) for e in entries]
    info = bat.step_info(plans, 0, None, n_split)
    assert bool(info["fused"]) == (n_split == 1) and (n_split == 1 or info["n_split"] >= 4), info
    return bat, entries, tokens, plans


@pytest.mark.parametrize("policy", cases.POLICIES)
@pytest.mark.parametrize("n_split", [1, 8], ids=["one_launch", "split"])
@pytest.mark.parametrize("draw", [0, 1], ids=["short_first", "short_last"])
@pytest.mark.parametrize("shape", list(cases.SHAPES))
def test_ragged_kv164_step_against_the_oracle(shape, draw, n_split, policy):
    from easykv_amd import StepPlan
    from oracle import easykv_oracle as O
    bat, entries, tokens, plans = _ragged(shape, draw, policy, Q, n_split)
    H = bat.bank.n_kv_heads
    assert {2, 17, 96, 300, 2049} <= {e["T"] for e in entries}
    widths = [e["W"] for e in entries]
    oplans = [O.StepPlan(**cases.plan_kw(e, policy)) for e in entries]
    assert {p.evict for p in plans} == {True, False} and any(p.score_off for p in plans)
    chk = _Check(bat)
    layers = list(range(len(entries)))
    for step, (q, k, v) in enumerate(tokens):
        grown = [i for i, e in enumerate(entries) if not e["evict"]]
        chk.step((shape, draw, n_split, policy, step), layers, plans, oplans, widths, q, k, v, n_split=n_split, fresh=grown if step else ())
        for i in grown:
            widths[i] += 1
            plans[i], oplans[i] = StepPlan(**cases.plan_kw(entries[i], policy, widths[i])), O.StepPlan(**cases.plan_kw(entries[i], policy, widths[i]))
        for i, e in enumerate(entries):
            assert bat.n_slots(i) == (e["T"] - 1 if e["evict"] else e["T"] + step), (e["T"], step, bat.n_slots(i))
    assert chk.n_dec == cases.STEPS * H * sum(e["evict"] for e in entries)
    print(f"[kv164-batch] ragged {shape} draw {draw} n_split {n_split} {policy}: {chk.n_stable} of {chk.n_dec} decisions well defined, "
          f"{chk.n_reseed} re-seeds, largest |out - oracle| {chk.worst:.3g}")
    assert chk.n_stable >= 0.9 * chk.n_dec, (chk.n_stable, chk.n_dec)


# ---- (c) the 16-bit twin of a ragged table ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_split", [1, 8], ids=["one_launch", "split"])
def test_ragged_16_bit_twin_decides_identically(n_split):
    from easykv_amd import StepPlan
    shape, draw, policy = "d128_gqa2_f16", 0, "roco"
    b8, entries, tokens, plans8 = _ragged(shape, draw, policy, None, n_split)      # (b8 / plans8: the 16-bit batch)
    b84, _, _, plans84 = _ragged(shape, draw, policy, Q, n_split)
    widths = [e["W"] for e in entries]
    for step, (q, k, v) in enumerate(tokens):
        q, k, v = q.cuda(), k.cuda(), v.cuda()
        o8, i8 = b8.attend(plans8, q, k, v, 0, n_split=n_split)
        o84, i84 = b84.attend(plans84, q, k, v, 0, n_split=n_split)
        ev = torch.tensor([p.evict for p in plans8], device="cuda")      # (an entry that keeps everything reports no id: its row is not written)
        assert bool(ev.any()) and not bool(ev.all()) and torch.equal(i8[ev], i84[ev]), (n_split, step, "evict_ids")
        assert b8.bank.n_slots == b84.bank.n_slots and b8.bank.extent == b84.bank.extent
        for arr in DECISION:
            a, b = getattr(b8.bank, arr), getattr(b84.bank, arr)
            if arr == "k":      # (the rows a layer has ever written; the rest of a bank is as allocated)
                for l, e in enumerate(b8.bank.extent):
                    assert torch.equal(a[l, :, :e].view(torch.int16), b[l, :, :e].view(torch.int16)), (n_split, step, arr, l)
                continue
            a, b = (a.view(torch.int32), b.view(torch.int32)) if a.dtype is torch.float32 else (a, b)
            assert torch.equal(a, b), (n_split, step, arr)
        for i, e in enumerate(entries):
            if not e["evict"]:
                widths[i] += 1
                plans8[i] = plans84[i] = StepPlan(**cases.plan_kw(e, policy, widths[i]))


# ---- (d) engine -----------------------------------------------------------------------------------------------------------------------------
def test_adopt_does_not_mix_formats_and_a_kv164_only_batch(monkeypatch):
    from easykv_amd import KVBankBatch, StepPlan, engine
    from easykv_amd._lib import EkvError
    monkeypatch.setattr(engine.KVBank, "use_slot_rows", False)
    L, Hq, H, D, rows = 2, 4, 4, 128, 90
    g = torch.Generator().manual_seed(6)
    bat = KVBankBatch(4, L, Hq, H, D, cap=256, kv_quant=Q)
    # K rows and the two V planes; a 16-bit V is never allocated
    assert bat.bank.k is not None and bat.bank.k.shape == (4 * L, H, bat.cap, D) and bat.bank.v is None and bat.kv_quant == Q
    assert bat.kv_bytes() == 4 * L * H * bat.cap * 324 and bat.bank.v4.shape == (4 * L, H, bat.cap, 64) and bat.bank.v_exp.shape == (4 * L, H, bat.cap, 4)
    assert not bool(bat.bank.v4.any()) and bool((bat.bank.v_exp == 127).all())
    solo = [_solo_bank(L, Hq, H, D, rows + 7 * i, 200, g) for i in range(2)]
    others = [_solo_bank(L, Hq, H, D, rows, 200, g).quantize(kind) for kind in ("fp8", "mxfp4", "mxfp6", "fp8_mxfp4")]
    for src in [solo[0]] + others:      # 16-bit, FP8, MXFP4, MXFP6 and FP8-key / MXFP4-value rows into a kv164 batch
        with pytest.raises(ValueError, match="kv_quant"):
            bat.adopt(0, src)
    for b in solo:
        b.quantize_k16_mxfp4()
    for kind in (None, "fp8", "mxfp4", "mxfp6", "fp8_mxfp4"):      # kv164 rows into a batch of any other format
        with pytest.raises(ValueError, match="kv_quant"):
            KVBankBatch(2, L, Hq, H, D, cap=256, **({"kv_quant": kind} if kind else {})).adopt(0, solo[0])
    for i, b in ((2, solo[0]), (0, solo[1])):
        bat.adopt(i, b)
        l0, c = i * L, b.cap
        for arr in PLANES + ("slot_of_pos", "score_sum", "score_sq", "score_cnt"):
            assert torch.equal(getattr(bat.bank, arr)[l0:l0 + L, :, :c], getattr(b, arr)), (i, arr)
        assert bat.bank.n_slots[l0:l0 + L] == b.n_slots and bat.bank.extent[l0:l0 + L] == b.extent
    # sequence(i) keeps the single-sequence behaviour: an immediate decode step is the solo bank's, bit for bit
    plan = StepPlan(policy="roco", phase="decode", evict=True, score_off=0, budget=rows, n_split=1)
    q, k, v = (torch.randn(L, hh, 1, D, generator=g).half().cuda() for hh in (Hq, H, H))
    o1, i1 = bat.sequence(2).attend(plan, q, k, v)
    o2, i2 = solo[0].attend(plan, q, k, v)
    assert torch.equal(o1, o2) and torch.equal(i1, i2)
    seq = bat.sequence(2)
    with pytest.raises(EkvError, match="row move"):
        seq.ordered_kv()
    with pytest.raises(EkvError, match="load_rows"):
        seq.load_rows(k, v)
    with pytest.raises(EkvError, match="quantised already"):
        bat.quantize_k16_mxfp4()
    with pytest.raises(EkvError, match="head_dim 128"):
        KVBankBatch(2, L, Hq, H, 64, cap=256, kv_quant=Q)
    KVBankBatch(2, L, 16, 2, D, cap=64, kv_quant=Q)      # GQA x 8 is taken


# ---- (e) generate_batch(kv_quant='k16_mxfp4') ---------------------------------------------------------------------------------------------
def test_generate_batch_equals_the_solo_runs(monkeypatch):
    """tests/test_hip_batch_kv6.py's case on kv164 rows: prompts of different lengths through generate_batch, each against its solo
    generate(kv_quant='k16_mxfp4') on deterministic logits: budget line, text, evicted ids, final length, outputs of every forward."""
    import easykv_amd
    from easykv_amd import engine
    from oracle.fake_model import make_streams
    from tests.batch_fake_model import BatchFakeModel
    from tests.native_fake_model import NativeFakeModel
    streams = make_streams(2, 4, 2, 128, 400, seed=11)
    cfg = dict(budget=40, kv_policy="roco", max_new_tokens=60, kv_quant=Q, _record_evictions=True)
    lengths = (16, 33, 64, 97)

    def solo(n, **over):
        model = NativeFakeModel(*streams)
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            res, cache = easykv_amd.generate(model, _ids(n), dict(cfg, **over), kv_mode="decoding", stride=1, return_cache=True)
        return model, res, cache, buf.getvalue().strip()

    model = BatchFakeModel(*streams)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        res, cache = easykv_amd.generate_batch(model, [_ids(n) for n in lengths], cfg, kv_mode="decoding", stride=1, return_cache=True)
    lines = buf.getvalue().strip().split("\n")
    bat = cache.bat
    assert bat.kv_quant == Q and bat.bank.k is not None and bat.bank.v is None and len(res) == len(lines) == len(lengths)
    assert bat.kv_bytes() == bat.bank.n_layers * bat.n_kv_heads * bat.cap * 324
    assert model.n_batched_forwards == cfg["max_new_tokens"] and bat.n_calls == model.n_batched_forwards * 2
    for i, n in enumerate(lengths):
        smodel, sres, scache, sline = solo(n)
        assert scache.kv_quant == Q
        solo_ev = _evictions(scache.evictions)
        # the precondition: the solo run again on the ordered score-row layout decides the same, so a differing id is never a near-tie
        monkeypatch.setattr(engine.KVBank, "use_slot_rows", False)
        _, sres2, scache2, sline2 = solo(n)
        monkeypatch.undo()
        ev2 = _evictions(scache2.evictions)
        assert sres2 == sres and sline2 == sline and len(ev2) == len(solo_ev) and all(np.array_equal(a, b) for a, b in zip(ev2, solo_ev)), (i, n, "precondition")
        assert res[i] == sres and lines[i] == sline, (i, n, res[i], sres, lines[i], sline)
        ours = _evictions(cache.evictions[i])
        assert len(ours) == len(solo_ev) > 0 and all(np.array_equal(a, b) for a, b in zip(ours, solo_ev)), (i, n, len(ours), len(solo_ev))
        assert bat.n_slots(i) == scache.get_seq_length(), (i, bat.n_slots(i), scache.get_seq_length())
        # the feature's promise at driver level: the evictions of the UNQUANTISED 16-bit run of the same prompt (the fake model's q / k / v
        # streams do not depend on the attention output, so the keys of the two runs are the same)
        _, _, scache16, _ = solo(n, kv_quant=None)
        ev16 = _evictions(scache16.evictions)
        assert scache16.kv_quant is None and len(ev16) == len(ours) and all(np.array_equal(a, b) for a, b in zip(ours, ev16)), (i, n, "16-bit run")
        assert len(model.logs[i]) == len(smodel.outputs_log)
        for f, (a, b) in enumerate(zip(model.logs[i], smodel.outputs_log)):
            assert a.shape == b.shape and out_close(a, b, 1e-3), (i, f, float((a - b).abs().max()))
