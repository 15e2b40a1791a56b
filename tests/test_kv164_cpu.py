"""16-bit keys with MXFP4 values ("kv164", include/easykv_hip.h; kv_quant='k16_mxfp4') on a CPU: the six calls of a uniform step exist
(the batch calls: tests/test_batch_kv164_cpu.py), their dry runs answer as the 16-bit step of the same shape wherever a kv164 bank takes
the step — every GQA factor — and refuse everything else before a launch, the keys' pointer is asked for, the build links the four new
objects (easykv_amd._build.later_objects()) beside the other lists, the driver quantises once at the prefill -> decode boundary, and the
seeded cases of the GPU test leave the oracle's decisions well defined on UNQUANTISED keys.  Dummy non-null pointers throughout:
nothing is dereferenced."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from tests import kv164_cases as K
from tests.test_dispatch_table import _case, _structs, cases
from tests.test_driver_cpu import api, _ids      # noqa: F401  (the stub-cache fixture)
from tests.test_kv6_cpu import _lib, _model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("ekv_kv164_quantize", "ekv_kv164_dequantize", "ekv_kv164_step_check", "ekv_kv164_step_info", "ekv_kv164_workspace_bytes",
         "ekv_kv164_step_attend")
OBJECTS = ["ekv_attn_decode_d128_plain_kv164", "ekv_attn_decode_d128_plain_kv164_bf16", "ekv_attn_decode_d128_plain_batch_kv164",
           "ekv_attn_decode_d128_plain_batch_kv164_bf16"]
F16, BF16 = 0, 1
Q = "k16_mxfp4"


def test_kv164_calls_are_exported_and_declared():
    L, lib = _lib()
    header = open(os.path.join(ROOT, "include", "easykv_hip.h")).read()
    declared = set(re.findall(r"\b(ekv_[a-z0-9_]+)\s*\(", header))
    raw = ctypes.CDLL(L.LIB)
    for name in CALLS:
        assert name in declared and name in L.EXPORTS and hasattr(raw, name) and hasattr(lib, name), name
    assert lib.ekv_abi_version() == 8
    assert "typedef struct ekv_kv164 {" in header
    # the header cites the MXFP4 rule for the V planes and does not restate it
    section = header[header.index('("kv164";'):header.index("typedef struct ekv_kv164 {")]
    assert '"MXFP4 K/V storage"' in section and "amax" not in section and "e2m1" not in section
    assert ctypes.sizeof(L.Kv164) == 16 and [f for f, _ in L.Kv164._fields_] == ["v_codes", "v_exp"]
    # argument checks come before any device access
    assert lib.ekv_kv164_step_check(None, None, F16, None) == -1
    assert lib.ekv_kv164_quantize(None, None, F16, 0, 1, 1, None) == -1
    assert lib.ekv_kv164_dequantize(None, None, 2, 0, 1, 1, None, None) == -1
    assert lib.ekv_kv164_workspace_bytes(None, None, F16, None) == 0
    kv164 = L.Kv164(256, 256)
    bank, _ = _structs(_case())
    b = ctypes.byref(bank)
    for planes in ((None, 256), (256, None)):
        assert lib.ekv_kv164_quantize(b, ctypes.byref(L.Kv164(*planes)), F16, 0, 1, 1, None) == -1
        assert lib.ekv_kv164_dequantize(b, ctypes.byref(L.Kv164(*planes)), 2, 0, 1, 1, 256, None) == -1
    assert lib.ekv_kv164_quantize(b, ctypes.byref(kv164), 2, 0, 1, 1, None) == -1                   # a dtype that is no 16-bit type
    assert lib.ekv_kv164_quantize(b, ctypes.byref(kv164), F16, 0, 1, bank.cap + 1, None) == -1      # an extent past the bank
    assert lib.ekv_kv164_dequantize(b, ctypes.byref(kv164), 2, 0, 1, 1, None, None) == -1           # no output
    bank.v = None
    assert lib.ekv_kv164_quantize(b, ctypes.byref(kv164), F16, 0, 1, 1, None) == -1                 # the source rows
    # the conversions are head_dim 128's
    for d in (32, 64, 96):
        bank, _ = _structs(_case(head_dim=d))
        assert lib.ekv_kv164_quantize(ctypes.byref(bank), ctypes.byref(kv164), F16, 0, 1, 1, None) == -2
        assert lib.ekv_kv164_dequantize(ctypes.byref(bank), ctypes.byref(kv164), 2, 0, 1, 1, 256, None) == -2


def _answers(lib, bank, st, dtype, kv164):
    b, s = ctypes.byref(bank), ctypes.byref(st)
    info = (ctypes.c_int32 * 9)(*([-7] * 9))
    if kv164 is None:
        return [lib.ekv_step_check_typed(b, s, dtype), lib.ekv_step_info_typed(b, s, dtype, info, 9)] + list(info) + [lib.ekv_workspace_bytes_typed(b, s, dtype)]
    k = ctypes.byref(kv164)
    return [lib.ekv_kv164_step_check(b, s, dtype, k), lib.ekv_kv164_step_info(b, s, dtype, k, info, 9)] + list(info) + [lib.ekv_kv164_workspace_bytes(b, s, dtype, k)]


def test_kv164_dry_runs_over_the_dispatch_grid():
    L, lib = _lib()
    kv164 = L.Kv164(256, 256)
    n_ok = n_fused = n_split = n_gqa = n_wide = 0
    for c in cases():
        bank, st = _structs(c)
        ref = _answers(lib, bank, st, F16, None)
        for dt in (F16, BF16):
            got = _answers(lib, bank, st, dt, kv164)
            takes = c["q_len"] == 1 and not c["rope_on_read"] and c["head_dim"] == 128      # (every GQA factor: the 16-bit plan)
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
            assert lib.ekv_kv164_step_check(ctypes.byref(bank), ctypes.byref(st), bad, ctypes.byref(kv164)) == -1
            assert lib.ekv_kv164_step_info(ctypes.byref(bank), ctypes.byref(st), bad, ctypes.byref(kv164), (ctypes.c_int32 * 9)(), 9) == -1
    assert n_ok > 50 and n_fused > 5 and n_split > 5 and n_gqa > 0, (n_ok, n_fused, n_split, n_gqa, n_wide)
    # the north-star shape: a fused fp16 step is a fused kv164 step on either score-row layout, and its phase order is F
    for extra in ({}, {"phases": 16, "phys_extent": 2112}):
        bank, st = _structs(_case(n_layers=32, **extra))
        ref, got = _answers(lib, bank, st, F16, None), _answers(lib, bank, st, F16, kv164)
        assert ref[0] == 0 and ref[3] == 1 and got == ref, (ref, got)
        info = (ctypes.c_int32 * 10)(*([-7] * 10))
        assert lib.ekv_kv164_step_info(ctypes.byref(bank), ctypes.byref(st), F16, ctypes.byref(kv164), info, 10) == 0 and info[9] == 0
    # the explicit refusals, each of a step the 16-bit call takes
    for kw in (dict(q_len=8, n_slots=2056, n_evict=8, roco_k1=1800, count_add2=16), dict(rope_on_read=1), dict(head_dim=32), dict(head_dim=64),
               dict(head_dim=96)):
        bank, st = _structs(_case(n_layers=32, **kw))
        assert lib.ekv_step_check(ctypes.byref(bank), ctypes.byref(st)) == 0, kw
        assert lib.ekv_kv164_step_check(ctypes.byref(bank), ctypes.byref(st), F16, ctypes.byref(kv164)) == -2, kw
    # every GQA factor the 16-bit decode step takes: x2, x3, x4, x5, x8, x16 answer what the 16-bit call answers
    for kw in (dict(hq=16, h=8), dict(hq=24, h=8), dict(hq=32, h=8), dict(hq=40, h=8), dict(hq=64, h=8), dict(hq=64, h=4)):
        bank, st = _structs(_case(n_layers=32, **kw))
        assert _answers(lib, bank, st, F16, kv164) == _answers(lib, bank, st, F16, None), kw
        assert _answers(lib, bank, st, F16, None)[0] == 0 or kw == dict(hq=64, h=4), kw
    # a descriptor with a missing plane is an argument error, whichever plane; so is a missing descriptor
    bank, st = _structs(_case(n_layers=32))
    for planes in ((None, 256), (256, None), (None, None)):
        assert lib.ekv_kv164_step_check(ctypes.byref(bank), ctypes.byref(st), F16, ctypes.byref(L.Kv164(*planes))) == -1
    assert lib.ekv_kv164_step_check(ctypes.byref(bank), ctypes.byref(st), F16, None) == -1
    # the 16-bit V rows are not needed any more; the K rows are read, so they are asked for
    bank.v = None
    assert lib.ekv_kv164_step_check(ctypes.byref(bank), ctypes.byref(st), F16, ctypes.byref(kv164)) == 0
    bank.k = None
    assert lib.ekv_kv164_step_check(ctypes.byref(bank), ctypes.byref(st), F16, ctypes.byref(kv164)) == -1
    info = (ctypes.c_int32 * 9)(*([-7] * 9))
    assert lib.ekv_kv164_step_info(ctypes.byref(bank), ctypes.byref(st), F16, ctypes.byref(kv164), info, 9) == -1
    assert lib.ekv_kv164_step_attend(ctypes.byref(bank), ctypes.byref(st), F16, ctypes.byref(kv164), 256, 256, 256, 256, None, None, None, 256, 1 << 30, None) == -1


def test_kv164_objects_are_among_the_later_objects_built_and_linked():
    """The kv164 instances are lines of ekv_instances_later.def: their four objects are among easykv_amd._build.later_objects(), apart
    from objects() and added_objects(), compiled with -DEKV_KV164=1 and no other row switch, and linked.  Nothing here says that they
    are the whole list."""
    from easykv_amd import _build
    every, added, later = dict(_build.objects()), dict(_build.added_objects()), dict(_build.later_objects())
    assert set(OBJECTS) <= set(later) and not set(later) & set(every) and not set(later) & set(added)
    assert len(later) == len(_build.later_objects()) == len(_build.later_instances())      # unique names, one object per line
    for b in ("single", "batch"):
        for e in ("f16", "bf16"):
            assert ("EKV_DECODE", ("128", "plain", e, "kv164", b)) in _build.later_instances()
    assert not any("kv164" in n for n in list(every) + list(added)) and not os.path.exists(os.path.join(_build.CSRC, "ekv_kv164.hip"))
    for n in OBJECTS:
        assert "-DEKV_KV164=1" in later[n] and "-DEKV_D=128" in later[n] and later[n][-1].endswith("ekv_attn_decode.inc")
        assert not any(f"-DEKV_{w}=1" in later[n] for w in ("KV8", "KV4", "KV6", "KV84"))
        assert ("-DEKV_BF16=1" in later[n]) == n.endswith("_bf16") and ("-DEKV_BATCH=1" in later[n]) == ("batch" in n)
    _build.build_lib()
    t = os.path.getmtime(_build.LATER_MANIFEST)
    for n in OBJECTS:
        obj = os.path.join(_build.OBJ, n + ".o")
        assert os.path.exists(obj) and os.path.getmtime(obj) >= t, n
    syms = subprocess.run(["nm", "-D", "--defined-only", _build.LIB], capture_output=True, text=True).stdout
    for elem in ("f16", "bf16"):
        for b in ("single", "batch"):
            assert f"ekv_launch_decode_fused_d128_plain_{elem}_kv164_{b}" in syms and f"ekv_launch_attn_decode_d128_plain_{elem}_kv164_{b}" in syms


def test_row_format_entry():
    from easykv_amd import engine
    fmt = engine.ROW_FORMATS[Q]
    assert fmt["rows"] == "kv164" and fmt["head_dims"] == (128,) and fmt["max_rep"] is None and fmt["pair_bytes"](128) == 324
    assert [(n, tail(128), fill) for n, tail, _, fill in fmt["planes"]] == [("v4", (64,), 0), ("v_exp", (4,), 127)]
    assert [p[2] for p in fmt["planes"]] == [torch.uint8, torch.uint8] and fmt["keeps"] == ("k",) and fmt["desc"] is engine._lib.Kv164
    assert engine.row_format(Q) is fmt
    assert all("keeps" not in f for k, f in engine.ROW_FORMATS.items() if k != Q)      # every other format releases both 16-bit tensors
    with pytest.raises(ValueError, match=r"must be None or 'fp8' / 'mxfp4', not 'int4'; 'mxfp6' is accepted as well, and 'fp8_mxfp4'$"):
        engine.row_format("int4")
    from easykv_amd import KVBank, KVBankBatch
    from easykv_amd._lib import EkvError
    assert callable(KVBank.quantize_k16_mxfp4) and callable(KVBankBatch.quantize_k16_mxfp4)
    for d in (64, 96):
        with pytest.raises(EkvError, match=rf"quantize_k16_mxfp4\(\): 16-bit-key / MXFP4-value rows are built for head_dim 128, not {d}"):
            KVBank(2, 4, 4, d, 64, kv_quant=Q)


# ---- the driver, through the stub caches of tests/test_driver_cpu.py -------------------------------------------------------------------
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
            text, cache = api.generate(model, _ids(16), dict(gen, kv_quant=Q, budget=8 if mode != "encoding" else 0.5), kv_mode=mode,
                                       stride=stride, return_cache=True)
        assert cache.bank.kv_quant == Q and len(text.split()) == 4
        quant = [i for i, e in enumerate(events) if e[0] == Q]
        assert len(quant) == 1 and not any(e[0] in ("fp8", "mxfp4", "fp8_mxfp4") for e in events), events
        before, after = events[:quant[0]], events[quant[0] + 1:]
        assert before and all(e[2] is None for e in before)                                   # the prefill runs on the 16-bit bank
        assert after and all(e[1] == 1 and e[2] == Q for e in after), events                  # every decode step on the quantised one
    # GQA factors of 8 and 16 are taken (the 16-bit plan's factors)
    for hq, h in ((16, 2), (32, 2)):
        with contextlib.redirect_stdout(io.StringIO()):
            text = api.generate(_model(hq=hq, h=h), _ids(16), dict(gen, kv_quant=Q), kv_mode="decoding")
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
            (_model(d=32), dict(kv_quant=Q), "decoding", "needs head_dim 128")):
        with pytest.raises(ValueError, match=match):
            api.generate(m, ids, dict(gen, **extra), kv_mode=mode)
    for extra, mode, match in ((dict(kv_quant=Q, streaming=True), "decoding", "streaming"), (dict(kv_quant=Q), "ppl", "ppl")):
        with pytest.raises(ValueError, match=match):
            api.generate_batch(model, [ids, _ids(20)], dict(gen, **extra), kv_mode=mode)
    with pytest.raises(ValueError, match="needs head_dim 128"):
        api.generate_batch(_model(d=64), [ids, _ids(20)], dict(gen, kv_quant=Q), kv_mode="decoding")
    model.layer_shard = SimpleNamespace(world=2, rank=0, begin=0, count=1)
    with pytest.raises(ValueError, match="layer-sharded"):
        api.generate(model, ids, dict(gen, kv_quant=Q), kv_mode="decoding")
    with pytest.raises(ValueError, match="layer-sharded"):
        api.generate_batch(model, [ids, _ids(20)], dict(gen, kv_quant=Q), kv_mode="decoding")
    assert T.StubCache.made == T.StubCacheBatch.made == 0


# ---- precondition of the GPU test's scored cases, on the reference side alone --------------------------------------------------------
def test_cases_are_the_kv6_cases():
    from tests import kv6_cases, kv84_cases
    assert K.STEPS is kv6_cases.STEPS and K.inputs is kv6_cases.inputs and K.SEED == 5 and K.TWIN_EXTRA is kv84_cases.TWIN_EXTRA
    assert len(K.STEPS) == 12 and {c[5] for c in K.STEPS} == {96, 300} and all(12 <= c[11] <= 48 for c in K.STEPS + K.TWIN_EXTRA)
    reps = {c[2] // c[3] for c in K.STEPS + K.TWIN_EXTRA}
    assert {1, 2, 3, 4, 8} <= reps
    # the 4-wave extras of the twin test: GQA x 8 and GQA x 2
    assert {c[2] // c[3] for c in K.TWIN_EXTRA if "4-wave" in c[0]} == {8, 2}


WELL_DEFINED = {"fused 8-wave slot-indexed roco": (768, 768), "fused 8-wave ordered h2o GQA4 bf16": (704, 704),
                "fused 4-wave slot-indexed tova GQA3": (352, 352), "split roco": (192, 192), "split tova GQA4 bf16": (96, 96),
                "deferred roco GQA2": (176, 176)}


@pytest.mark.parametrize("case", [c for c in K.STEPS if c[6] in K.SCORED], ids=[c[0] for c in K.STEPS if c[6] in K.SCORED])
def test_scored_cases_have_well_defined_decisions(case):
    """The oracle over the case's seeded inputs on UNQUANTISED K (V, as tests/kv4_ref.py quantises it, cannot touch a decision): at least
    90 % of the decisions are well defined under tests.test_hip_fullsize.Probe (the cap tests/test_hip_kv164.py asserts on the GPU).
    With seed 5 every decision is: 768/768, 704/704, 352/352, 192/192, 96/96 and 176/176."""
    from oracle import easykv_oracle as O
    from tests.test_hip_fullsize import Probe
    name, L, hq, h, dtype, budget, policy, n_split, defer, slot, expect, steps = case
    k0, v0, warm, per_step = K.inputs(case)
    layers = sorted({0, L - 1})
    states = {}
    for l in layers:
        kd, vd = K.dequant_ref(k0[l], v0[l])
        assert torch.equal(kd, k0[l].float())
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
    print(f"[kv164-precondition] {name}: {n_stable}/{n_dec} = {n_stable / n_dec:.4f} of the decisions well defined")
    assert n_stable >= 0.9 * n_dec, (name, n_stable, n_dec)
    assert name in WELL_DEFINED and n_dec == WELL_DEFINED[name][1], (name, n_dec)
