"""MXFP4 K/V storage ("kv4", include/easykv_hip.h) on a CPU: the six calls exist, their dry runs answer as the 16-bit step of the same
shape wherever a kv4 bank takes the step and refuse everything else before a launch, the build links the new objects beside the
recorded ones, the driver quantises once at the prefill -> decode boundary, and the rule's restatement (tests/kv4_ref.py) and the
seeded cases of the GPU test have the properties that test relies on.  Dummy non-null pointers throughout: nothing is dereferenced."""
import ctypes
import os
import re

import pytest
import torch

from tests import kv4_cases as K
from tests import kv4_ref as R
from tests.test_dispatch_table import _case, _structs, cases
from tests.test_driver_cpu import api, _ids      # noqa: F401  (the stub-cache fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("ekv_kv4_quantize", "ekv_kv4_dequantize", "ekv_kv4_step_check", "ekv_kv4_step_info", "ekv_kv4_workspace_bytes",
         "ekv_kv4_step_attend")
F16, BF16 = 0, 1


def _lib():
    from easykv_amd import _build, _lib as L
    if not os.path.exists(_build.LIB):
        _build.build_lib()
    return L, L.load()


def test_kv4_calls_are_exported_and_declared():
    L, lib = _lib()
    header = open(os.path.join(ROOT, "include", "easykv_hip.h")).read()
    declared = set(re.findall(r"\b(ekv_[a-z0-9_]+)\s*\(", header))
    raw = ctypes.CDLL(L.LIB)
    for name in CALLS:
        assert name in declared and name in L.EXPORTS and hasattr(raw, name) and hasattr(lib, name), name
    assert lib.ekv_abi_version() == 8
    assert "typedef struct ekv_kv4 {" in header and "e2m1" in header and "E8M0" in header and "low nibble" in header
    assert ctypes.sizeof(L.Kv4) == 4 * 8
    # argument checks come before any device access
    assert lib.ekv_kv4_step_check(None, None, F16, None) == -1
    assert lib.ekv_kv4_quantize(None, None, F16, 0, 1, 1, None) == -1
    assert lib.ekv_kv4_dequantize(None, None, 2, 0, 1, 1, None, None, None) == -1
    assert lib.ekv_kv4_workspace_bytes(None, None, F16, None) == 0
    # the conversions are head_dim 128's
    bank, _ = _structs(_case(head_dim=64))
    kv4 = L.Kv4(256, 256, 256, 256)
    assert lib.ekv_kv4_quantize(ctypes.byref(bank), ctypes.byref(kv4), F16, 0, 1, 1, None) == -2
    assert lib.ekv_kv4_dequantize(ctypes.byref(bank), ctypes.byref(kv4), 2, 0, 1, 1, 256, 256, None) == -2


def _answers(lib, bank, st, dtype, kv4):
    b, s = ctypes.byref(bank), ctypes.byref(st)
    info = (ctypes.c_int32 * 9)(*([-7] * 9))
    if kv4 is None:
        return [lib.ekv_step_check_typed(b, s, dtype), lib.ekv_step_info_typed(b, s, dtype, info, 9)] + list(info) + [lib.ekv_workspace_bytes_typed(b, s, dtype)]
    k = ctypes.byref(kv4)
    return [lib.ekv_kv4_step_check(b, s, dtype, k), lib.ekv_kv4_step_info(b, s, dtype, k, info, 9)] + list(info) + [lib.ekv_kv4_workspace_bytes(b, s, dtype, k)]


def test_kv4_dry_runs_over_the_dispatch_grid():
    L, lib = _lib()
    kv4 = L.Kv4(256, 256, 256, 256)
    n_ok = n_fused = n_split = n_gqa = 0
    for c in cases():
        bank, st = _structs(c)
        ref = _answers(lib, bank, st, F16, None)
        for dt in (F16, BF16):
            got = _answers(lib, bank, st, dt, kv4)
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
            assert lib.ekv_kv4_step_check(ctypes.byref(bank), ctypes.byref(st), bad, ctypes.byref(kv4)) == -1
            assert lib.ekv_kv4_step_info(ctypes.byref(bank), ctypes.byref(st), bad, ctypes.byref(kv4), (ctypes.c_int32 * 9)(), 9) == -1
    assert n_ok > 50 and n_fused > 5 and n_split > 5 and n_gqa > 0, (n_ok, n_fused, n_split, n_gqa)
    # the north-star shape: a fused fp16 step is a fused kv4 step on either score-row layout, and its phase order is F
    for extra in ({}, {"phases": 16, "phys_extent": 2112}):
        bank, st = _structs(_case(n_layers=32, **extra))
        ref, got = _answers(lib, bank, st, F16, None), _answers(lib, bank, st, F16, kv4)
        assert ref[0] == 0 and ref[3] == 1 and got == ref, (ref, got)
        info = (ctypes.c_int32 * 10)(*([-7] * 10))
        assert lib.ekv_kv4_step_info(ctypes.byref(bank), ctypes.byref(st), F16, ctypes.byref(kv4), info, 10) == 0 and info[9] == 0
    # the explicit refusals, each of a step the 16-bit call takes
    for kw in (dict(q_len=8, n_slots=2056, n_evict=8, roco_k1=1800, count_add2=16), dict(rope_on_read=1), dict(head_dim=32), dict(head_dim=64),
               dict(head_dim=96), dict(hq=40, h=8), dict(hq=64, h=8)):
        bank, st = _structs(_case(n_layers=32, **kw))
        assert lib.ekv_step_check(ctypes.byref(bank), ctypes.byref(st)) == 0, kw
        assert lib.ekv_kv4_step_check(ctypes.byref(bank), ctypes.byref(st), F16, ctypes.byref(kv4)) == -2, kw
    for kw in (dict(hq=24, h=8), dict(hq=32, h=8), dict(hq=16, h=8)):      # GQA x3 (padded build), x4, x2
        bank, st = _structs(_case(n_layers=32, **kw))
        assert lib.ekv_kv4_step_check(ctypes.byref(bank), ctypes.byref(st), F16, ctypes.byref(kv4)) == 0, kw
    # a descriptor with a missing plane is an argument error, whichever plane
    bank, st = _structs(_case(n_layers=32))
    for i in range(4):
        planes = [256] * 4
        planes[i] = None
        assert lib.ekv_kv4_step_check(ctypes.byref(bank), ctypes.byref(st), F16, ctypes.byref(L.Kv4(*planes))) == -1
    # the 16-bit row pointers are not needed any more
    bank.k = bank.v = None
    assert lib.ekv_kv4_step_check(ctypes.byref(bank), ctypes.byref(st), F16, ctypes.byref(kv4)) == 0


def test_new_objects_are_built_beside_the_recorded_ones():
    """The kv4 family and its conversion unit among easykv_amd._build.objects() (which tests/test_instances_cpu.py holds to the recorded
    set): the conversion unit is an ordinary source, the instances come from ordinary lines of the manifest."""
    from easykv_amd import _build
    want = ["ekv_kv4", "ekv_attn_decode_d128_plain_kv4", "ekv_attn_decode_d128_plain_kv4_bf16"]
    every = [n for n, _ in _build.objects()]
    assert [n for n in every if n == "ekv_kv4" or n.startswith("ekv_attn_decode_d128_plain_kv4")] == want and len(set(every)) == len(every)
    assert len(every) == len(_build.sources()) + len(_build.instances())      # one object per source + one per manifest line
    lines = [(fam, w) for fam, w in _build.instances() if "kv4" in w and "single" in w]
    assert lines == [("EKV_DECODE", ("128", "plain", "f16", "kv4", "single")), ("EKV_DECODE", ("128", "plain", "bf16", "kv4", "single"))]
    assert all(fam in _build.FAMILIES for fam, _ in lines)
    args = dict(_build.objects())
    assert "-DEKV_KV4=1" in args["ekv_attn_decode_d128_plain_kv4"] and "-DEKV_BF16=1" in args["ekv_attn_decode_d128_plain_kv4_bf16"]
    _build.build_lib()
    t = os.path.getmtime(_build.MANIFEST)
    for n in want:
        obj = os.path.join(_build.OBJ, n + ".o")
        assert os.path.exists(obj) and os.path.getmtime(obj) >= t, n
    import subprocess
    syms = subprocess.run(["nm", "-D", "--defined-only", _build.LIB], capture_output=True, text=True).stdout
    for elem in ("f16", "bf16"):
        assert f"ekv_launch_decode_fused_d128_plain_{elem}_kv4_single" in syms and f"ekv_launch_attn_decode_d128_plain_{elem}_kv4_single" in syms


def test_reference_rule_properties():
    g = torch.Generator().manual_seed(3)
    for dtype in (torch.float16, torch.bfloat16):
        x = R.special_rows(16, 128, g, dtype)
        codes, exps = R.quantize(x)
        assert codes.shape == (x.shape[0], 64) and exps.shape == (x.shape[0], 4) and codes.dtype == exps.dtype == torch.uint8
        R.check_rows(x, codes, exps, dtype)
        e = exps.int() - 127
        blocks = x.float().view(-1, 4, 32)
        amax = blocks.abs().amax(-1)
        nz = amax > 0
        # e is the SMALLEST exponent that holds the block: amax <= 6 * 2^e, and amax > 6 * 2^(e - 1) unless clamped
        assert bool((amax <= 6 * torch.ldexp(torch.ones_like(amax), e)).all())
        assert bool(((amax > 3 * torch.ldexp(torch.ones_like(amax), e)) | (e == -126))[nz].all())
        assert bool((e[~nz] == 0).all()) and bool((exps != 255).all())
        back = R.dequant(codes, exps).view(-1, 4, 32)
        step = torch.ldexp(torch.ones_like(amax), e).unsqueeze(-1)
        # half a step of the grid at the value's magnitude: 0.25 below 2, 0.5 up to 4, 1 above (in units of 2^e)
        q = blocks.abs() / step
        bound = torch.where(q <= 2, torch.full_like(q, 0.25), torch.where(q <= 4, torch.full_like(q, 0.5), torch.ones_like(q))) * step
        assert bool(((back - blocks).abs() <= bound).all())
        # a second pass is the identity: the codes are fixed points of the rule
        c2, e2 = R.quantize(R.dequant(codes, exps))
        keep = (R.unpack(codes).view(-1, 4, 32) & 7).amax(-1) >= 6      # (blocks whose maximum code is 6 keep their exponent)
        assert torch.equal(e2[keep], exps[keep]) and R.same_codes(c2.view(-1, 4, 16)[keep], codes.view(-1, 4, 16)[keep])
    # the ties of the rule, and a maximum of exactly 6 * 2^e
    x = torch.zeros(1, 32)
    x[0, :8] = torch.tensor([6.0, 1.25, 2.5, 5.0, 0.25, 0.75, 1.75, 3.5]) * 0.125
    x[0, 8:11] = torch.tensor([-1.25, -2.5, -5.0]) * 0.125
    codes, exps = R.quantize(x)
    assert int(exps[0, 0]) == 127 - 3
    assert (R.dequant(codes, exps)[0, :11] * 8).tolist() == [6.0, 1.0, 2.0, 4.0, 0.0, 1.0, 2.0, 4.0, -1.0, -2.0, -4.0]
    assert int(codes[0, 0]) == 7 | (2 << 4)      # element 0 (6 -> code 7) in the low nibble, element 1 (1 -> code 2) in the high nibble
    x[0, 0] = 6.0 * 0.125 * (1 + 2.0 ** -10)
    assert int(R.quantize(x)[1][0, 0]) == 127 - 2
    # the exponent as the kernels take it from the float's bits (ekv_fp4_block_exp) is the rule's
    amax = torch.cat([torch.rand(4096, generator=g) * 8, torch.tensor([6.0, 3.0, 1.5, 0.75, 6.0 * 2.0 ** -20, 2.0 ** -24, 65504.0, 1e-30, 3e38, 2.0 ** -130])])
    bits = amax.view(torch.int32).long()
    byte = (((bits + 0x3FFFFF) >> 23) - 2).clamp(1, 254)
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
    R.check_rows(zero, cz | 0x88, ez)      # -0 for +0 is the same value


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
            text, cache = api.generate(model, _ids(16), dict(gen, kv_quant="mxfp4", budget=8 if mode != "encoding" else 0.5), kv_mode=mode,
                                       stride=stride, return_cache=True)
        assert cache.bank.kv_quant == "mxfp4" and len(text.split()) == 4
        quant = [i for i, e in enumerate(events) if e[0] == "mxfp4"]
        assert len(quant) == 1 and not any(e[0] == "fp8" for e in events), events
        before, after = events[:quant[0]], events[quant[0] + 1:]
        assert before and all(e[2] is None for e in before)                                   # the prefill runs on the 16-bit bank
        assert after and all(e[1] == 1 and e[2] == "mxfp4" for e in after), events            # every decode step on the quantised one
    T.StubCache.made = 0
    ids = _ids(16)
    for m, extra, mode, match in (
            (model, dict(kv_quant="mxfp4", streaming=True), "decoding", "streaming"),
            (model, dict(kv_quant="mxfp4"), "ppl", "ppl"),
            (_model(d=64), dict(kv_quant="mxfp4"), "decoding", "needs head_dim 128"),
            (_model(d=32), dict(kv_quant="mxfp4"), "decoding", "needs head_dim 128"),
            (_model(hq=16, h=2), dict(kv_quant="mxfp4"), "decoding", "GQA factor of at most 4"),
            (model, dict(kv_quant="int4"), "decoding", "must be None or 'fp8' / 'mxfp4'")):
        with pytest.raises(ValueError, match=match):
            api.generate(m, ids, dict(gen, **extra), kv_mode=mode)
    with pytest.raises(ValueError, match="mxfp4"):
        api.generate_batch(model, [ids, _ids(20)], dict(gen, kv_quant="mxfp4"), kv_mode="decoding")
    model.layer_shard = SimpleNamespace(world=2, rank=0, begin=0, count=1)
    with pytest.raises(ValueError, match="layer-sharded"):
        api.generate(model, ids, dict(gen, kv_quant="mxfp4"), kv_mode="decoding")
    assert T.StubCache.made == T.StubCacheBatch.made == 0


# ---- precondition of the GPU test's scored cases, on the reference side alone --------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in K.STEPS if c[6] in K.SCORED], ids=[c[0] for c in K.STEPS if c[6] in K.SCORED])
def test_scored_cases_have_well_defined_decisions(case):
    """The oracle over the case's seeded inputs as tests/kv4_ref.py quantises them: at least 90 % of the decisions are well defined
    under tests.test_hip_fullsize.Probe (the cap tests/test_hip_kv4.py asserts on the GPU; kv8's)."""
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
    print(f"[kv4-precondition] {name}: {n_stable}/{n_dec} = {n_stable / n_dec:.4f} of the decisions well defined")
    assert n_stable >= 0.9 * n_dec, (name, n_stable, n_dec)
