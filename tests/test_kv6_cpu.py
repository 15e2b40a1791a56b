"""MXFP6 K/V storage ("kv6", include/easykv_hip.h) on a CPU: the six calls of a uniform step exist (the batch calls: tests/test_batch_kv6_cpu.py), their dry runs answer as the 16-bit step of the same
shape wherever a kv6 bank takes the step and refuse everything else before a launch, the build links the new objects beside the
recorded ones, the driver quantises once at the prefill -> decode boundary, and the rule's restatement (tests/kv6_ref.py) and the
seeded cases of the GPU test have the properties that test relies on.  Dummy non-null pointers throughout: nothing is dereferenced."""
import ctypes
import os
import re

import pytest
import torch

from tests import kv6_cases as K
from tests import kv6_ref as R
from tests.test_dispatch_table import _case, _structs, cases
from tests.test_driver_cpu import api, _ids      # noqa: F401  (the stub-cache fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("ekv_kv6_quantize", "ekv_kv6_dequantize", "ekv_kv6_step_check", "ekv_kv6_step_info", "ekv_kv6_workspace_bytes",
         "ekv_kv6_step_attend")
F16, BF16 = 0, 1


def _lib():
    from easykv_amd import _build, _lib as L
    if not os.path.exists(_build.LIB):
        _build.build_lib()
    return L, L.load()


def test_kv6_calls_are_exported_and_declared():
    L, lib = _lib()
    header = open(os.path.join(ROOT, "include", "easykv_hip.h")).read()
    declared = set(re.findall(r"\b(ekv_[a-z0-9_]+)\s*\(", header))
    raw = ctypes.CDLL(L.LIB)
    for name in CALLS:
        assert name in declared and name in L.EXPORTS and hasattr(raw, name) and hasattr(lib, name), name
    assert lib.ekv_abi_version() == 8
    assert "typedef struct ekv_kv6 {" in header and "e2m3" in header and "E8M0" in header and "little-endian" in header and "INTERLEAVED" in header
    assert ctypes.sizeof(L.Kv6) == 4 * 8
    # argument checks come before any device access
    assert lib.ekv_kv6_step_check(None, None, F16, None) == -1
    assert lib.ekv_kv6_quantize(None, None, F16, 0, 1, 1, None) == -1
    assert lib.ekv_kv6_dequantize(None, None, 2, 0, 1, 1, None, None, None) == -1
    assert lib.ekv_kv6_workspace_bytes(None, None, F16, None) == 0
    # the conversions are head_dim 128's
    bank, _ = _structs(_case(head_dim=64))
    kv6 = L.Kv6(256, 256, 256, 256)
    assert lib.ekv_kv6_quantize(ctypes.byref(bank), ctypes.byref(kv6), F16, 0, 1, 1, None) == -2
    assert lib.ekv_kv6_dequantize(ctypes.byref(bank), ctypes.byref(kv6), 2, 0, 1, 1, 256, 256, None) == -2


def _answers(lib, bank, st, dtype, kv6):
    b, s = ctypes.byref(bank), ctypes.byref(st)
    info = (ctypes.c_int32 * 9)(*([-7] * 9))
    if kv6 is None:
        return [lib.ekv_step_check_typed(b, s, dtype), lib.ekv_step_info_typed(b, s, dtype, info, 9)] + list(info) + [lib.ekv_workspace_bytes_typed(b, s, dtype)]
    k = ctypes.byref(kv6)
    return [lib.ekv_kv6_step_check(b, s, dtype, k), lib.ekv_kv6_step_info(b, s, dtype, k, info, 9)] + list(info) + [lib.ekv_kv6_workspace_bytes(b, s, dtype, k)]


def test_kv6_dry_runs_over_the_dispatch_grid():
    L, lib = _lib()
    kv6 = L.Kv6(256, 256, 256, 256)
    n_ok = n_fused = n_split = n_gqa = 0
    for c in cases():
        bank, st = _structs(c)
        ref = _answers(lib, bank, st, F16, None)
        for dt in (F16, BF16):
            got = _answers(lib, bank, st, dt, kv6)
            takes = c["q_len"] == 1 and not c["rope_on_read"] and c["head_dim"] == 128 and c["hq"] // c["h"] <= 4
            if ref[0] == -1:                      # fp16's own EKV_E_ARG cases keep their code
                assert got[0] == -1, (c, got)
            elif ref[0] == 0 and takes:           # accepted, with the fp16 step's plan: splits, fused, launches, workspace
                assert got == ref, (c, got, ref)
                n_ok += dt == F16
                n_fused += dt == F16 and got[3] == 1
                n_split += dt == F16 and got[2] > 1
                n_gqa += dt == F16 and c["hq"] // c["h"] > 1
            else:                                 # chunk steps, RoPE-on-read, other head dims, GQA > 4, fp16's own refusals
                assert got[0] == -2, (c, got, ref)
                assert got[1] != 0 or (got[3] == 0 and got[10] == 0), (c, got)      # not fused, no launches
        for bad in (2, -1):
            assert lib.ekv_kv6_step_check(ctypes.byref(bank), ctypes.byref(st), bad, ctypes.byref(kv6)) == -1
            assert lib.ekv_kv6_step_info(ctypes.byref(bank), ctypes.byref(st), bad, ctypes.byref(kv6), (ctypes.c_int32 * 9)(), 9) == -1
    assert n_ok > 50 and n_fused > 5 and n_split > 5 and n_gqa > 0, (n_ok, n_fused, n_split, n_gqa)
    # the north-star shape: a fused fp16 step is a fused kv6 step on either score-row layout, and its phase order is F
    for extra in ({}, {"phases": 16, "phys_extent": 2112}):
        bank, st = _structs(_case(n_layers=32, **extra))
        ref, got = _answers(lib, bank, st, F16, None), _answers(lib, bank, st, F16, kv6)
        assert ref[0] == 0 and ref[3] == 1 and got == ref, (ref, got)
        info = (ctypes.c_int32 * 10)(*([-7] * 10))
        assert lib.ekv_kv6_step_info(ctypes.byref(bank), ctypes.byref(st), F16, ctypes.byref(kv6), info, 10) == 0 and info[9] == 0
    # the explicit refusals, each of a step the 16-bit call takes
    for kw in (dict(q_len=8, n_slots=2056, n_evict=8, roco_k1=1800, count_add2=16), dict(rope_on_read=1), dict(head_dim=32), dict(head_dim=64),
               dict(head_dim=96), dict(hq=40, h=8), dict(hq=64, h=8)):
        bank, st = _structs(_case(n_layers=32, **kw))
        assert lib.ekv_step_check(ctypes.byref(bank), ctypes.byref(st)) == 0, kw
        assert lib.ekv_kv6_step_check(ctypes.byref(bank), ctypes.byref(st), F16, ctypes.byref(kv6)) == -2, kw
    for kw in (dict(hq=24, h=8), dict(hq=32, h=8), dict(hq=16, h=8)):      # GQA x3 (padded build), x4, x2
        bank, st = _structs(_case(n_layers=32, **kw))
        assert lib.ekv_kv6_step_check(ctypes.byref(bank), ctypes.byref(st), F16, ctypes.byref(kv6)) == 0, kw
    # a descriptor with a missing plane is an argument error, whichever plane
    bank, st = _structs(_case(n_layers=32))
    for i in range(4):
        planes = [256] * 4
        planes[i] = None
        assert lib.ekv_kv6_step_check(ctypes.byref(bank), ctypes.byref(st), F16, ctypes.byref(L.Kv6(*planes))) == -1
    # the 16-bit row pointers are not needed any more
    bank.k = bank.v = None
    assert lib.ekv_kv6_step_check(ctypes.byref(bank), ctypes.byref(st), F16, ctypes.byref(kv6)) == 0


def test_added_objects_are_built_beside_the_recorded_ones():
    """The kv6 instances are easykv_amd._build.added_objects(): unique names, disjoint from objects() (which tests/test_instances_cpu.py
    holds to the recorded set), together one object per source and per line of the manifest and of the file it includes, all built and
    linked; the conversions live in the conversion unit of the MX formats, not in a source of their own."""
    import subprocess
    from easykv_amd import _build
    want = ["ekv_attn_decode_d128_plain_kv6", "ekv_attn_decode_d128_plain_kv6_bf16", "ekv_attn_decode_d128_plain_batch_kv6",
            "ekv_attn_decode_d128_plain_batch_kv6_bf16"]
    every, added = [n for n, _ in _build.objects()], [n for n, _ in _build.added_objects()]
    assert added == want and len(set(added)) == len(added) and not set(added) & set(every)
    assert not any("kv6" in n for n in every) and not os.path.exists(os.path.join(_build.CSRC, "ekv_kv6.hip"))
    lines = _build.added_instances()
    assert lines == [("EKV_DECODE", ("128", "plain", e, "kv6", b)) for b in ("single", "batch") for e in ("f16", "bf16")]
    assert not any("kv6" in w for _, w in _build.instances())      # (ekv_instances.def itself: the recorded lines, one for one)
    assert len(every) + len(added) == len(_build.sources()) + len(_build.instances()) + len(lines)
    # the manifest includes the added lines, so the X-macro readers see one manifest
    assert '#include "ekv_instances_added.def"' in open(_build.MANIFEST).read() and _build.ADDED_MANIFEST in _build.headers()
    args = dict(_build.added_objects())
    for n in want:
        assert "-DEKV_KV6=1" in args[n] and "-DEKV_D=128" in args[n] and args[n][-1].endswith("ekv_attn_decode.inc")
        assert ("-DEKV_BF16=1" in args[n]) == n.endswith("_bf16") and ("-DEKV_BATCH=1" in args[n]) == ("batch" in n)
    _build.build_lib()
    t = max(os.path.getmtime(_build.MANIFEST), os.path.getmtime(_build.ADDED_MANIFEST))
    for n in want + every:
        obj = os.path.join(_build.OBJ, n + ".o")
        assert os.path.exists(obj) and os.path.getmtime(obj) >= t, n
    syms = subprocess.run(["nm", "-D", "--defined-only", _build.LIB], capture_output=True, text=True).stdout
    for elem in ("f16", "bf16"):
        for b in ("single", "batch"):
            assert f"ekv_launch_decode_fused_d128_plain_{elem}_kv6_{b}" in syms and f"ekv_launch_attn_decode_d128_plain_{elem}_kv6_{b}" in syms


def test_reference_rule_properties():
    assert R.GRID.numel() == 32 and bool((R.GRID[1:] > R.GRID[:-1]).all()) and float(R.GRID[-1]) == 7.5
    assert R.GRID.tolist() == [i / 8 for i in range(16)] + [2 + i / 4 for i in range(8)] + [4 + i / 2 for i in range(8)]
    g = torch.Generator().manual_seed(3)
    for dtype in (torch.float16, torch.bfloat16):
        x = R.special_rows(16, 128, g, dtype)
        codes, exps = R.quantize(x)
        assert codes.shape == (x.shape[0], 96) and exps.shape == (x.shape[0], 4) and codes.dtype == exps.dtype == torch.uint8
        assert torch.equal(R.pack(R.unpack(codes)), codes)
        R.check_rows(x, codes, exps, dtype)
        e = exps.int() - 127
        blocks = x.float().view(-1, 4, 32)
        amax = blocks.abs().amax(-1)
        nz = amax > 0
        # e is the SMALLEST exponent that holds the block: amax <= 7.5 * 2^e, and amax > 7.5 * 2^(e - 1) unless clamped
        assert bool((amax <= 7.5 * torch.ldexp(torch.ones_like(amax), e)).all())
        assert bool(((amax > 3.75 * torch.ldexp(torch.ones_like(amax), e)) | (e == -126))[nz].all())
        assert bool((e[~nz] == 0).all()) and bool((exps != 255).all())
        back = R.dequant(codes, exps).view(-1, 4, 32)
        step = torch.ldexp(torch.ones_like(amax), e).unsqueeze(-1)
        # half a step of the grid at the value's magnitude: 1/16 below 2, 1/8 up to 4, 1/4 above (in units of 2^e)
        q = blocks.abs() / step
        bound = torch.where(q <= 2, torch.full_like(q, 0.0625), torch.where(q <= 4, torch.full_like(q, 0.125), torch.full_like(q, 0.25))) * step
        assert bool(((back - blocks).abs() <= bound).all())
        # a second pass is the identity: the values are fixed points of the rule, and so are codes and exponents of every block whose
        # largest code is 4 or more (a maximum that rounded down to 3.75 is 7.5 one exponent lower: the same value)
        c2, e2 = R.quantize(R.dequant(codes, exps))
        assert torch.equal(R.dequant(c2, e2)[(e > -126).repeat_interleave(32, -1)], back.view(-1, 128)[(e > -126).repeat_interleave(32, -1)])
        keep = (R.unpack(codes).view(-1, 4, 32) & 31).amax(-1) >= 24
        assert int(keep.sum()) > 0.8 * int(nz.sum())
        assert torch.equal(e2[keep], exps[keep]) and R.same_codes(c2.view(-1, 4, 24)[keep], codes.view(-1, 4, 24)[keep])
    # the ties of the rule, and a maximum of exactly 7.5 * 2^e
    x = torch.zeros(1, 32)
    x[0, :8] = torch.tensor([7.5, 1.9375, 3.875, 0.0625, 0.1875, 2.125, 2.375, 7.25]) * 0.125
    x[0, 8:11] = torch.tensor([-1.9375, -3.875, -0.0625]) * 0.125
    codes, exps = R.quantize(x)
    assert int(exps[0, 0]) == 127 - 3
    assert (R.dequant(codes, exps)[0, :11] * 8).tolist() == [7.5, 2.0, 4.0, 0.0, 0.25, 2.0, 2.5, 7.0, -2.0, -4.0, -0.0]
    assert R.unpack(codes)[0, :4].tolist() == [31, 16, 24, 0] and R.unpack(codes)[0, 8:11].tolist() == [48, 56, 32]
    # element 0 (7.5 -> code 31) in bits 0..5, element 1 (2 -> code 16) from bit 6: little-endian
    assert int(codes[0, 0]) == (31 | (16 << 6)) & 255 and int(codes[0, 1]) == ((16 >> 2) | (24 << 4)) & 255
    x[0, 0] = 7.5 * 0.125 * (1 + 2.0 ** -10)
    assert int(R.quantize(x)[1][0, 0]) == 127 - 2
    for ex in (-20, 0, 9):      # a maximum of exactly 7.5 * 2^e keeps e
        assert int(R.quantize(torch.full((1, 32), 7.5 * 2.0 ** ex))[1][0, 0]) == 127 + ex
    cz, ez = R.quantize(torch.zeros(2, 64))
    assert bool((cz == 0).all()) and bool((ez == 127).all())
    # the exponent as the kernels take it from the float's bits (ekv_fp6_block_exp) is the rule's
    amax = torch.cat([torch.rand(4096, generator=g) * 8, torch.tensor([7.5, 3.75, 1.875, 0.9375, 7.5 * 2.0 ** -20, 2.0 ** -24, 65504.0, 1e-30, 3e38,
                                                                       2.0 ** -130, 7.5 * (1 + 2.0 ** -22), 1.875 * (1 + 2.0 ** -23), 2.0 ** -126])])
    bits = amax.view(torch.int32).long()
    byte = (((bits + 0x0FFFFF) >> 23) - 2).clamp(1, 254)
    want = R.block_exp(amax.view(-1, 1).expand(-1, 32).contiguous())[:, 0].long() + 127
    assert torch.equal(byte, want)
    # checks that can fail: a code one step off, an exponent one too large
    x = torch.tensor([[1.0, 0.3, -0.7, 0.11] * 8])
    codes, exps = R.quantize(x)
    for bad_c, bad_e in ((codes ^ 1, exps), (codes, exps + 1)):
        with pytest.raises(AssertionError):
            R.check_rows(x, bad_c, bad_e)
    zero = torch.zeros(1, 32)
    cz, ez = R.quantize(zero)
    R.check_rows(zero, R.pack(R.unpack(cz) | 32), ez)      # -0 for +0 is the same value


def test_row_error_is_derived_below_half_of_mxfp4s():
    """On the rows of the fidelity case (standard normal fp16, tests/test_hip_kv6.py) the relative row RMS error of the MXFP6 rule is
    below 0.5 x the MXFP4 rule's.  Derived: both rules scale a block by a power of two under its maximum (7.5 against 6) and the e2m3
    grid is four times finer at equal magnitude, so the ratio is 0.25 up to the difference of the two maxima; measured 0.245; the
    margin is 2 x."""
    from tests import kv4_ref
    g = torch.Generator().manual_seed(21)
    x = torch.randn(2, 8, 256, 128, generator=g).half().float()
    rel = lambda ref: float(((ref.dequant(*ref.quantize(x)) - x).pow(2).sum(-1).sqrt() / x.pow(2).sum(-1).sqrt()).mean())
    e6, e4 = rel(R), rel(kv4_ref)
    print(f"[kv6-rule] relative row RMS error: MXFP6 {e6:.4f}, MXFP4 {e4:.4f}, ratio {e6 / e4:.3f}")
    assert e6 < 0.5 * e4, (e6, e4)


# ---- the driver, through the stub caches of tests/test_driver_cpu.py -------------------------------------------------------------------
def _model(hq=4, h=2, d=128, layers=2):
    from oracle.fake_model import make_streams
    from tests.native_fake_model import NativeFakeModel
    return NativeFakeModel(*make_streams(layers, hq, h, d, 64, seed=1), device="cpu")


def test_generate_quantises_once_at_the_boundary_and_refuses_before_a_cache(api, monkeypatch):
    import contextlib
    import io
    from types import SimpleNamespace
    from tests import test_driver_cpu as T
    events = []

    class Bank(T.StubBank):
        def quantize(self, kind):
            events.append((kind, self.n_slots[0]))
            self.kv_quant = kind
    monkeypatch.setattr(T, "StubBank", Bank)
    attend = T.StubCache.attend

    def logged(self, layer_idx, q, k, v):
        if layer_idx == 0:
            events.append(("forward", q.shape[2], self.bank.kv_quant))
        return attend(self, layer_idx, q, k, v)
    monkeypatch.setattr(T.StubCache, "attend", logged)
    gen = dict(kv_policy="roco", budget=8, max_new_tokens=4, eos_token_ids=[-1])
    model = _model()
    for mode, stride in (("decoding", 1), ("encoding", 4), ("auto", 4)):
        del events[:]
        with contextlib.redirect_stdout(io.StringIO()):
            text, cache = api.generate(model, _ids(16), dict(gen, kv_quant="mxfp6", budget=8 if mode != "encoding" else 0.5), kv_mode=mode,
                                       stride=stride, return_cache=True)
        assert cache.bank.kv_quant == "mxfp6" and len(text.split()) == 4
        quant = [i for i, e in enumerate(events) if e[0] == "mxfp6"]
        assert len(quant) == 1 and not any(e[0] == "fp8" for e in events), events
        before, after = events[:quant[0]], events[quant[0] + 1:]
        assert before and all(e[2] is None for e in before)                                   # the prefill runs on the 16-bit bank
        assert after and all(e[1] == 1 and e[2] == "mxfp6" for e in after), events            # every decode step on the quantised one
    # generate_batch takes the value: every prompt's bank quantised once, right after its own prefill, and an MXFP6-only batch bank
    made = []

    class Batch(T.StubBankBatch):
        def __init__(self, *a, kv_quant=None, **k):
            super().__init__(*a, **k)
            made.append(kv_quant)
    monkeypatch.setattr(api, "KVBankBatch", Batch)
    from oracle.fake_model import make_streams
    from tests.batch_fake_model import BatchFakeModel
    bmodel = BatchFakeModel(*make_streams(2, 4, 2, 128, 64, seed=1), device="cpu")
    del events[:]
    with contextlib.redirect_stdout(io.StringIO()):
        texts = api.generate_batch(bmodel, [_ids(16), _ids(20)], dict(gen, kv_quant="mxfp6"), kv_mode="decoding")
    assert len(texts) == 2 and all(len(t.split()) == 4 for t in texts) and made == ["mxfp6"]
    assert [e for e in events if e[0] == "mxfp6"] == [("mxfp6", 16), ("mxfp6", 20)], events
    T.StubCache.made = T.StubCacheBatch.made = 0
    ids = _ids(16)
    for m, extra, mode, match in (
            (model, dict(kv_quant="mxfp6", streaming=True), "decoding", "streaming"),
            (model, dict(kv_quant="mxfp6"), "ppl", "ppl"),
            (_model(d=64), dict(kv_quant="mxfp6"), "decoding", "needs head_dim 128"),
            (_model(d=32), dict(kv_quant="mxfp6"), "decoding", "needs head_dim 128"),
            (_model(hq=16, h=2), dict(kv_quant="mxfp6"), "decoding", "GQA factor of at most 4"),
            (model, dict(kv_quant="int4"), "decoding", "not 'int4'; 'mxfp6' is accepted as well")):
        with pytest.raises(ValueError, match=match):
            api.generate(m, ids, dict(gen, **extra), kv_mode=mode)
    for extra, mode, match in ((dict(kv_quant="mxfp6", streaming=True), "decoding", "streaming"), (dict(kv_quant="mxfp6"), "ppl", "ppl")):
        with pytest.raises(ValueError, match=match):
            api.generate_batch(model, [ids, _ids(20)], dict(gen, **extra), kv_mode=mode)
    with pytest.raises(ValueError, match="needs head_dim 128"):
        api.generate_batch(_model(d=64), [ids, _ids(20)], dict(gen, kv_quant="mxfp6"), kv_mode="decoding")
    with pytest.raises(ValueError, match="mxfp4"):      # (the batch driver's own MXFP4 refusal stays)
        api.generate_batch(model, [ids, _ids(20)], dict(gen, kv_quant="mxfp4"), kv_mode="decoding")
    model.layer_shard = SimpleNamespace(world=2, rank=0, begin=0, count=1)
    with pytest.raises(ValueError, match="layer-sharded"):
        api.generate(model, ids, dict(gen, kv_quant="mxfp6"), kv_mode="decoding")
    assert T.StubCache.made == T.StubCacheBatch.made == 0


# ---- precondition of the GPU test's scored cases, on the reference side alone --------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in K.STEPS if c[6] in K.SCORED], ids=[c[0] for c in K.STEPS if c[6] in K.SCORED])
def test_scored_cases_have_well_defined_decisions(case):
    """The oracle over the case's seeded inputs as tests/kv6_ref.py quantises them: at least 90 % of the decisions are well defined
    under tests.test_hip_fullsize.Probe (the cap tests/test_hip_kv6.py asserts on the GPU; kv8's)."""
    from oracle import easykv_oracle as O
    from tests.test_hip_fullsize import Probe
    name, L, hq, h, dtype, budget, policy, n_split, defer, slot, expect, steps = case
    k0, v0, warm, per_step = K.inputs(case)
    layers = sorted({0, L - 1})
    deq = lambda x: R.dequant(*R.quantize(x))
    states = {}
    for l in layers:
        st = O.LayerState(k=deq(k0[l]).unsqueeze(0), v=deq(v0[l]).unsqueeze(0))
        st.s, st.q, st.c = O.init_state_decoding((h,), budget)
        st.s[:, :budget] += warm[l]
        st.q[:, :budget] += warm[l] ** 2
        states[l] = st
    probe = Probe()
    O.SELECT_HOOK = probe
    n_dec = n_stable = 0
    try:
        for q, k, v, rs in per_step:
            for l in layers:
                O.layer_step(states[l], q[l:l + 1].float(), deq(k[l]).unsqueeze(0), deq(v[l]).unsqueeze(0), O.StepPlan(range_start=rs, **K.plan_kw(case)))
                n_dec += h
                n_stable += int((~probe.last_unstable).sum())
    finally:
        O.SELECT_HOOK = None
    print(f"[kv6-precondition] {name}: {n_stable}/{n_dec} = {n_stable / n_dec:.4f} of the decisions well defined")
    assert n_stable >= 0.9 * n_dec, (name, n_stable, n_dec)
