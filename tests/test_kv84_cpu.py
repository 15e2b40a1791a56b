"""FP8 keys with MXFP4 values ("kv84", include/easykv_hip.h; kv_quant='fp8_mxfp4') on a CPU: the six calls of a uniform step exist (the
batch calls: tests/test_batch_kv84_cpu.py), their dry runs answer as the 16-bit step of the same shape wherever a kv84 bank takes the
step and refuse everything else before a launch, the build links the four new objects (easykv_amd._build.later_objects()) beside the
other two lists, the driver quantises once at the prefill -> decode boundary, and the seeded cases of the GPU test leave the oracle's
decisions well defined on rows quantised by the two rules.  Dummy non-null pointers throughout: nothing is dereferenced."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from tests import kv84_cases as K
from tests.test_dispatch_table import _case, _structs, cases
from tests.test_driver_cpu import api, _ids      # noqa: F401  (the stub-cache fixture)
from tests.test_kv6_cpu import _lib, _model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("ekv_kv84_quantize", "ekv_kv84_dequantize", "ekv_kv84_step_check", "ekv_kv84_step_info", "ekv_kv84_workspace_bytes",
         "ekv_kv84_step_attend")
OBJECTS = ["ekv_attn_decode_d128_plain_kv84", "ekv_attn_decode_d128_plain_kv84_bf16", "ekv_attn_decode_d128_plain_batch_kv84",
           "ekv_attn_decode_d128_plain_batch_kv84_bf16"]
F16, BF16 = 0, 1


def test_kv84_calls_are_exported_and_declared():
    L, lib = _lib()
    header = open(os.path.join(ROOT, "include", "easykv_hip.h")).read()
    declared = set(re.findall(r"\b(ekv_[a-z0-9_]+)\s*\(", header))
    raw = ctypes.CDLL(L.LIB)
    for name in CALLS:
        assert name in declared and name in L.EXPORTS and hasattr(raw, name) and hasattr(lib, name), name
    assert lib.ekv_abi_version() == 8
    assert "typedef struct ekv_kv84 {" in header
    # the header cites the two rules and restates neither
    section = header[header.index('("kv84";'):header.index("typedef struct ekv_kv84 {")]
    assert '"FP8 K/V storage"' in section and '"MXFP4 K/V storage"' in section and "amax" not in section and "448" not in section
    assert ctypes.sizeof(L.Kv84) == 4 * 8 and [f for f, _ in L.Kv84._fields_] == ["k_codes", "v_codes", "k_scale", "v_exp"]
    # argument checks come before any device access
    assert lib.ekv_kv84_step_check(None, None, F16, None) == -1
    assert lib.ekv_kv84_quantize(None, None, F16, 0, 1, 1, None) == -1
    assert lib.ekv_kv84_dequantize(None, None, 2, 0, 1, 1, None, None, None) == -1
    assert lib.ekv_kv84_workspace_bytes(None, None, F16, None) == 0
    # the conversions are head_dim 128's
    kv84 = L.Kv84(256, 256, 256, 256)
    for d in (32, 64, 96):
        bank, _ = _structs(_case(head_dim=d))
        assert lib.ekv_kv84_quantize(ctypes.byref(bank), ctypes.byref(kv84), F16, 0, 1, 1, None) == -2
        assert lib.ekv_kv84_dequantize(ctypes.byref(bank), ctypes.byref(kv84), 2, 0, 1, 1, 256, 256, None) == -2


def _answers(lib, bank, st, dtype, kv84):
    b, s = ctypes.byref(bank), ctypes.byref(st)
    info = (ctypes.c_int32 * 9)(*([-7] * 9))
    if kv84 is None:
        return [lib.ekv_step_check_typed(b, s, dtype), lib.ekv_step_info_typed(b, s, dtype, info, 9)] + list(info) + [lib.ekv_workspace_bytes_typed(b, s, dtype)]
    k = ctypes.byref(kv84)
    return [lib.ekv_kv84_step_check(b, s, dtype, k), lib.ekv_kv84_step_info(b, s, dtype, k, info, 9)] + list(info) + [lib.ekv_kv84_workspace_bytes(b, s, dtype, k)]


def test_kv84_dry_runs_over_the_dispatch_grid():
    L, lib = _lib()
    kv84 = L.Kv84(256, 256, 256, 256)
    n_ok = n_fused = n_split = n_gqa = n_wide = 0
    for c in cases():
        bank, st = _structs(c)
        ref = _answers(lib, bank, st, F16, None)
        for dt in (F16, BF16):
            got = _answers(lib, bank, st, dt, kv84)
            takes = c["q_len"] == 1 and not c["rope_on_read"] and c["head_dim"] == 128      # (every GQA factor: kv8's)
            if ref[0] == -1:                      # fp16's own EKV_E_ARG cases keep their code
                assert got[0] == -1, (c, got)
            elif ref[0] == 0 and takes:           # accepted, with the fp16 step's plan: splits, fused, launches, workspace
                assert got == ref, (c, got, ref)
                n_ok += dt == F16
                n_fused += dt == F16 and got[3] == 1
                n_split += dt == F16 and got[2] > 1
                n_gqa += dt == F16 and c["hq"] // c["h"] > 1
                n_wide += dt == F16 and c["hq"] // c["h"] > 4
            else:                                 # chunk steps, RoPE-on-read, other head dims, fp16's own refusals
                assert got[0] == -2, (c, got, ref)
                assert got[1] != 0 or (got[3] == 0 and got[10] == 0), (c, got)      # not fused, no launches
        for bad in (2, -1):
            assert lib.ekv_kv84_step_check(ctypes.byref(bank), ctypes.byref(st), bad, ctypes.byref(kv84)) == -1
            assert lib.ekv_kv84_step_info(ctypes.byref(bank), ctypes.byref(st), bad, ctypes.byref(kv84), (ctypes.c_int32 * 9)(), 9) == -1
    assert n_ok > 50 and n_fused > 5 and n_split > 5 and n_gqa > 0, (n_ok, n_fused, n_split, n_gqa, n_wide)
    # the north-star shape: a fused fp16 step is a fused kv84 step on either score-row layout, and its phase order is F
    for extra in ({}, {"phases": 16, "phys_extent": 2112}):
        bank, st = _structs(_case(n_layers=32, **extra))
        ref, got = _answers(lib, bank, st, F16, None), _answers(lib, bank, st, F16, kv84)
        assert ref[0] == 0 and ref[3] == 1 and got == ref, (ref, got)
        info = (ctypes.c_int32 * 10)(*([-7] * 10))
        assert lib.ekv_kv84_step_info(ctypes.byref(bank), ctypes.byref(st), F16, ctypes.byref(kv84), info, 10) == 0 and info[9] == 0
    # the explicit refusals, each of a step the 16-bit call takes
    for kw in (dict(q_len=8, n_slots=2056, n_evict=8, roco_k1=1800, count_add2=16), dict(rope_on_read=1), dict(head_dim=32), dict(head_dim=64),
               dict(head_dim=96)):
        bank, st = _structs(_case(n_layers=32, **kw))
        assert lib.ekv_step_check(ctypes.byref(bank), ctypes.byref(st)) == 0, kw
        assert lib.ekv_kv84_step_check(ctypes.byref(bank), ctypes.byref(st), F16, ctypes.byref(kv84)) == -2, kw
    # GQA factors as kv8 takes them: x2, x3, x4, x5, x8 answer what the kv8 call answers
    kv8 = L.Kv8(256, 256, 256, 256)
    for kw in (dict(hq=16, h=8), dict(hq=24, h=8), dict(hq=32, h=8), dict(hq=40, h=8), dict(hq=64, h=8)):
        bank, st = _structs(_case(n_layers=32, **kw))
        b, s = ctypes.byref(bank), ctypes.byref(st)
        assert lib.ekv_kv84_step_check(b, s, F16, ctypes.byref(kv84)) == lib.ekv_kv8_step_check(b, s, F16, ctypes.byref(kv8)) == 0, kw
    # a descriptor with a missing plane is an argument error, whichever plane
    bank, st = _structs(_case(n_layers=32))
    for i in range(4):
        planes = [256] * 4
        planes[i] = None
        assert lib.ekv_kv84_step_check(ctypes.byref(bank), ctypes.byref(st), F16, ctypes.byref(L.Kv84(*planes))) == -1
    # the 16-bit row pointers are not needed any more
    bank.k = bank.v = None
    assert lib.ekv_kv84_step_check(ctypes.byref(bank), ctypes.byref(st), F16, ctypes.byref(kv84)) == 0


def test_kv84_objects_are_among_the_later_objects_built_and_linked():
    """The kv84 instances are lines of ekv_instances_later.def: their four objects are among easykv_amd._build.later_objects(), apart
    from objects() and added_objects(), compiled with -DEKV_KV84=1 and linked.  Nothing here says that they are the whole list: the
    next feature appends its lines to that file."""
    from easykv_amd import _build
    every, added, later = dict(_build.objects()), dict(_build.added_objects()), dict(_build.later_objects())
    assert set(OBJECTS) <= set(later) and not set(later) & set(every) and not set(later) & set(added)
    assert len(later) == len(_build.later_objects()) == len(_build.later_instances())      # unique names, one object per line
    for b in ("single", "batch"):
        for e in ("f16", "bf16"):
            assert ("EKV_DECODE", ("128", "plain", e, "kv84", b)) in _build.later_instances()
    assert not any("kv84" in n for n in list(every) + list(added)) and not os.path.exists(os.path.join(_build.CSRC, "ekv_kv84.hip"))
    assert '#include "ekv_instances_later.def"' in open(_build.MANIFEST).read() and _build.LATER_MANIFEST in _build.headers()
    for n in OBJECTS:
        assert "-DEKV_KV84=1" in later[n] and "-DEKV_D=128" in later[n] and later[n][-1].endswith("ekv_attn_decode.inc")
        assert "-DEKV_KV8=1" not in later[n] and "-DEKV_KV4=1" not in later[n]
        assert ("-DEKV_BF16=1" in later[n]) == n.endswith("_bf16") and ("-DEKV_BATCH=1" in later[n]) == ("batch" in n)
    _build.build_lib()
    t = os.path.getmtime(_build.LATER_MANIFEST)
    for n in OBJECTS:
        obj = os.path.join(_build.OBJ, n + ".o")
        assert os.path.exists(obj) and os.path.getmtime(obj) >= t, n
    syms = subprocess.run(["nm", "-D", "--defined-only", _build.LIB], capture_output=True, text=True).stdout
    for elem in ("f16", "bf16"):
        for b in ("single", "batch"):
            assert f"ekv_launch_decode_fused_d128_plain_{elem}_kv84_{b}" in syms and f"ekv_launch_attn_decode_d128_plain_{elem}_kv84_{b}" in syms
    # the measurement tools know the new names
    for tool in ("kernel_regs.py", "isa_identity.py"):
        assert "later_objects" in open(os.path.join(ROOT, "tools", tool)).read(), tool


def test_row_format_entry():
    from easykv_amd import engine
    fmt = engine.ROW_FORMATS["fp8_mxfp4"]
    assert fmt["rows"] == "kv84" and fmt["head_dims"] == (128,) and fmt["max_rep"] is None and fmt["pair_bytes"](128) == 200
    assert [(n, tail(128), fill) for n, tail, _, fill in fmt["planes"]] == [("k8", (128,), 0), ("v4", (64,), 0), ("k_scale", (), 1), ("v_exp", (4,), 127)]
    assert [p[2] for p in fmt["planes"]] == [torch.uint8, torch.uint8, torch.float32, torch.uint8]
    assert engine.row_format("fp8_mxfp4") is fmt
    with pytest.raises(ValueError, match=r"must be None or 'fp8' / 'mxfp4', not 'int4'; 'mxfp6' is accepted as well, and 'fp8_mxfp4'$"):
        engine.row_format("int4")
    from easykv_amd import KVBank, KVBankBatch
    from easykv_amd._lib import EkvError
    assert callable(KVBank.quantize_fp8_mxfp4) and callable(KVBankBatch.quantize_fp8_mxfp4)
    for d in (64, 96):
        with pytest.raises(EkvError, match=rf"quantize_fp8_mxfp4\(\): FP8-key / MXFP4-value rows are built for head_dim 128, not {d}"):
            KVBank(2, 4, 4, d, 64, kv_quant="fp8_mxfp4")


# ---- the driver, through the stub caches of tests/test_driver_cpu.py -------------------------------------------------------------------
def test_generate_quantises_once_at_the_boundary_and_refuses_before_a_cache(api, monkeypatch):
    import contextlib
    import io
    from types import SimpleNamespace
    from tests import test_driver_cpu as T
    events = []
    Q = "fp8_mxfp4"

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
            text, cache = api.generate(model, _ids(16), dict(gen, kv_quant=Q, budget=8 if mode != "encoding" else 0.5), kv_mode=mode,
                                       stride=stride, return_cache=True)
        assert cache.bank.kv_quant == Q and len(text.split()) == 4
        quant = [i for i, e in enumerate(events) if e[0] == Q]
        assert len(quant) == 1 and not any(e[0] in ("fp8", "mxfp4") for e in events), events
        before, after = events[:quant[0]], events[quant[0] + 1:]
        assert before and all(e[2] is None for e in before)                                   # the prefill runs on the 16-bit bank
        assert after and all(e[1] == 1 and e[2] == Q for e in after), events                  # every decode step on the quantised one
    # a GQA factor of 8 is taken (kv8's factors)
    with contextlib.redirect_stdout(io.StringIO()):
        text = api.generate(_model(hq=16, h=2), _ids(16), dict(gen, kv_quant=Q), kv_mode="decoding")
    assert len(text.split()) == 4
    # generate_batch takes the value: every prompt's bank quantised once, right after its own prefill, and a batch bank of that format
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
        texts = api.generate_batch(bmodel, [_ids(16), _ids(20)], dict(gen, kv_quant=Q), kv_mode="decoding")
    assert len(texts) == 2 and all(len(t.split()) == 4 for t in texts) and made == [Q]
    assert [e for e in events if e[0] == Q] == [(Q, 16), (Q, 20)], events
    T.StubCache.made = T.StubCacheBatch.made = 0
    ids = _ids(16)
    for m, extra, mode, match in (
            (model, dict(kv_quant=Q, streaming=True), "decoding", "streaming"),
            (model, dict(kv_quant=Q), "ppl", "ppl"),
            (_model(d=64), dict(kv_quant=Q), "decoding", "needs head_dim 128"),
            (_model(d=32), dict(kv_quant=Q), "decoding", "needs head_dim 128"),
            (model, dict(kv_quant="int4"), "decoding", "not 'int4'; 'mxfp6' is accepted as well, and 'fp8_mxfp4'")):
        with pytest.raises(ValueError, match=match):
            api.generate(m, ids, dict(gen, **extra), kv_mode=mode)
    for extra, mode, match in ((dict(kv_quant=Q, streaming=True), "decoding", "streaming"), (dict(kv_quant=Q), "ppl", "ppl")):
        with pytest.raises(ValueError, match=match):
            api.generate_batch(model, [ids, _ids(20)], dict(gen, **extra), kv_mode=mode)
    with pytest.raises(ValueError, match="needs head_dim 128"):
        api.generate_batch(_model(d=64), [ids, _ids(20)], dict(gen, kv_quant=Q), kv_mode="decoding")
    with pytest.raises(ValueError, match="mxfp4"):      # (the batch driver's own MXFP4 refusal stays)
        api.generate_batch(model, [ids, _ids(20)], dict(gen, kv_quant="mxfp4"), kv_mode="decoding")
    model.layer_shard = SimpleNamespace(world=2, rank=0, begin=0, count=1)
    with pytest.raises(ValueError, match="layer-sharded"):
        api.generate(model, ids, dict(gen, kv_quant=Q), kv_mode="decoding")
    assert T.StubCache.made == T.StubCacheBatch.made == 0


# ---- precondition of the GPU test's scored cases, on the reference side alone --------------------------------------------------------
def test_cases_are_the_kv6_cases():
    from tests import kv6_cases
    assert K.STEPS is kv6_cases.STEPS and K.inputs is kv6_cases.inputs and K.SEED == 5
    assert {c[5] for c in K.STEPS} == {96, 300} and all(12 <= c[11] <= 48 for c in K.STEPS + K.TWIN_EXTRA)
    reps = {c[2] // c[3] for c in K.STEPS + K.TWIN_EXTRA}
    assert {1, 2, 3, 4, 8} <= reps


@pytest.mark.parametrize("case", [c for c in K.STEPS if c[6] in K.SCORED], ids=[c[0] for c in K.STEPS if c[6] in K.SCORED])
def test_scored_cases_have_well_defined_decisions(case):
    """The oracle over the case's seeded inputs, K as tests/kv8_ref.py and V as tests/kv4_ref.py quantise them: at least 90 % of the
    decisions are well defined under tests.test_hip_fullsize.Probe (the cap tests/test_hip_kv84.py asserts on the GPU).  With seed 5
    every decision is: 768/768, 704/704, 352/352, 192/192, 96/96 and 176/176."""
    from oracle import easykv_oracle as O
    from tests.test_hip_fullsize import Probe
    name, L, hq, h, dtype, budget, policy, n_split, defer, slot, expect, steps = case
    k0, v0, warm, per_step = K.inputs(case)
    layers = sorted({0, L - 1})
    states = {}
    for l in layers:
        kd, vd = K.dequant_ref(k0[l], v0[l])
        st = O.LayerState(k=kd.unsqueeze(0), v=vd.unsqueeze(0))
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
                kd, vd = K.dequant_ref(k[l], v[l])
                O.layer_step(states[l], q[l:l + 1].float(), kd.unsqueeze(0), vd.unsqueeze(0), O.StepPlan(range_start=rs, **K.plan_kw(case)))
                n_dec += h
                n_stable += int((~probe.last_unstable).sum())
    finally:
        O.SELECT_HOOK = None
    print(f"[kv84-precondition] {name}: {n_stable}/{n_dec} = {n_stable / n_dec:.4f} of the decisions well defined")
    assert n_stable >= 0.9 * n_dec, (name, n_stable, n_dec)
