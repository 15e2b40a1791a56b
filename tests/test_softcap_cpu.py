"""Soft-capped logits and the free softmax scale without a GPU: dry runs of the capped call family (ekv_cap_*) through the C ABI over fake
banks (nothing is dereferenced, nothing is launched), the new manifest lines, the Python refusals, the driver over the stub caches of
tests/test_driver_cpu.py, and the planner driven over a capped grid by a stand-alone program under AddressSanitizer + UBSan
(tests/plan_softcap_main.cpp; the sanitizer runtimes are linked into the program, which runs as a child process).

What the plans must say: a capped decode step plans field for field as the uncapped call of the same step (DESIGN.md §3.17 names no
field that differs: phase order and resident rows are kept); a capped chunk step or dense prefix runs on the 16x16x32 kernel in blocks
of at most 32 folded rows at head_dim 128 as at 256 — never on the wide, the logits-in-LDS or the logits-resident kernel; RoPE-on-read,
head_dim 32 / 64 / 96, a GQA factor above 32 in a chunk step and a cap that is <= 0, NaN or infinite are refused with zero launches and
zero workspace bytes."""
import contextlib
import ctypes
import io
import math
import os
import re
import shutil
import subprocess
from types import SimpleNamespace

import pytest
import torch

from tests.test_dispatch_table import _case, _chunk, _structs, cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMPILERS = [c for c in ("g++", "/opt/rocm/llvm/bin/clang++") if shutil.which(c)]
INFO = ("n_split", "one_launch", "two_pass", "wide", "n_qblocks", "qb_rows", "n_col_parts", "fold_in_kernel", "n_launches", "fused_order")
F16, BF16 = 0, 1
OK, ARG, UNSUPPORTED = 0, -1, -2
CALLS = ("ekv_cap_step_check", "ekv_cap_step_info", "ekv_cap_workspace_bytes", "ekv_cap_step_attend", "ekv_softcap_eval")


@pytest.fixture(scope="module")
def lib():
    from easykv_amd import _build, _lib
    if not os.path.exists(_build.LIB):
        _build.build_lib()
    return _lib.load()


def _plain(lib, bank, st, dtype):
    b, s = ctypes.byref(bank), ctypes.byref(st)
    info = (ctypes.c_int32 * 10)(*([-7] * 10))
    return [lib.ekv_step_check_typed(b, s, dtype), lib.ekv_step_info_typed(b, s, dtype, info, 10)] + list(info) + [lib.ekv_workspace_bytes_typed(b, s, dtype)]


def _capped(lib, bank, st, dtype, cap):
    b, s = ctypes.byref(bank), ctypes.byref(st)
    info = (ctypes.c_int32 * 10)(*([-7] * 10))
    return [lib.ekv_cap_step_check(b, s, dtype, cap), lib.ekv_cap_step_info(b, s, dtype, cap, info, 10)] + list(info) + [lib.ekv_cap_workspace_bytes(b, s, dtype, cap)]


def _refused(got, code=UNSUPPORTED):
    """The capped call's answer is `code`, with zero launches and zero bytes."""
    d = dict(zip(INFO, got[2:12]))
    return got[0] == code and got[12] == 0 and (got[1] != 0 or (d["n_launches"] == 0 and d["one_launch"] == 0))


def test_capped_calls_are_exported_and_declared(lib):
    from easykv_amd import _lib as L
    header = open(os.path.join(ROOT, "include", "easykv_hip.h")).read()
    declared = set(re.findall(r"\b(ekv_[a-z0-9_]+)\s*\(", header))
    raw = ctypes.CDLL(L.LIB)
    for name in CALLS:
        assert name in declared and name in L.EXPORTS and hasattr(raw, name), name
    assert lib.ekv_abi_version() == 8
    assert "cap * tanh((q.k / sm_div) / cap)" in header and "NORMATIVE" in header
    # argument checks come before any device access
    assert lib.ekv_cap_step_check(None, None, F16, 50.0) == ARG
    assert lib.ekv_cap_workspace_bytes(None, None, F16, 50.0) == 0
    assert lib.ekv_softcap_eval(None, 4, 1.0, 50.0, None, None) == ARG and lib.ekv_softcap_eval(None, 0, 1.0, 50.0, None, None) == OK
    assert lib.ekv_softcap_eval(None, -1, 1.0, 50.0, None, None) == ARG


def test_capped_dry_runs_over_the_dispatch_grid(lib):
    n = dict(decode_ok=0, fused=0, split=0, chunk_ok=0, chunk_33_128=0, refused=0, arg=0)
    for c in cases():
        bank, st = _structs(c)
        rep = c["hq"] // c["h"]
        for dt, cap in ((F16, 50.0), (BF16, 2.0)):
            ref, got = _plain(lib, bank, st, dt), _capped(lib, bank, st, dt, cap)
            served = c["head_dim"] in (128, 256) and not c["rope_on_read"]
            if ref[0] == ARG:                                   # the plain call's own argument errors keep their code
                assert _refused(got, ARG), (c, got)
                n["arg"] += 1
            elif c["q_len"] == 1:
                if ref[0] == OK and served:                     # a decode step: the uncapped call's plan, every field and the workspace
                    assert got == ref, (c, got, ref)
                    n["decode_ok"] += 1
                    n["fused"] += got[3] == 1
                    n["split"] += got[2] > 1
                else:
                    assert _refused(got), (c, got, ref)
                    n["refused"] += 1
            else:
                d = dict(zip(INFO, got[2:12]))
                if not served or rep > 32 or ref[0] != OK:
                    # (a step the plain call refuses for its width, strides or phases is refused here as well: the checks are shared)
                    assert _refused(got) or (ref[0] != OK and served and rep <= 32 and got[0] in (OK, UNSUPPORTED)), (c, got, ref)
                    n["refused"] += got[0] != OK
                if got[0] == OK:
                    # blocks of at most 32 folded rows on the 16x16 kernel; never the wide, the logits-in-LDS or the resident kernel (the
                    # last reports one launch with two_pass = 1; the second one launch of a step the one-pass kernel cannot end itself)
                    assert d["wide"] == 0 and d["qb_rows"] * rep <= 32 and d["n_qblocks"] == -(-c["q_len"] // d["qb_rows"]), (c, d)
                    assert not (d["one_launch"] and d["two_pass"]), (c, d)
                    assert not d["one_launch"] or (d["n_qblocks"] == 1 and d["n_split"] == 1 and d["n_launches"] == 1), (c, d)
                    assert got[12] > 0 and (d["n_launches"] >= 1 or (ref[0] == OK and ref[10] == 0)), (c, got, ref)      # (phases that leave nothing to launch)
                    n["chunk_ok"] += 1
                    n["chunk_33_128"] += 33 <= rep * c["q_len"] <= 128
        for bad in (0.0, -2.0, float("inf"), float("nan")):
            assert _refused(_capped(lib, bank, st, F16, bad), ARG), (c, bad)
        assert lib.ekv_cap_step_check(ctypes.byref(bank), ctypes.byref(st), 2, 50.0) == ARG
    print("capped dry runs over the dispatch grid:", n)
    assert n["decode_ok"] > 100 and n["fused"] > 10 and n["split"] > 10 and n["chunk_ok"] > 100 and n["chunk_33_128"] > 20 and n["refused"] > 100, n


def test_capped_plans_and_refusals_by_name(lib):
    # the north-star decode step, on either score-row layout: the uncapped plan, phase order included
    for extra in ({}, {"phases": 16, "phys_extent": 2112}):
        bank, st = _structs(_case(n_layers=32, **extra))
        ref, got = _plain(lib, bank, st, F16), _capped(lib, bank, st, F16, 50.0)
        assert ref[0] == OK and ref[3] == 1 and got == ref, (ref, got)
    # resident rows: the plain call's answer is the capped launch's (the cap changes no plan of a decode step)
    bank, st = _structs(_case(n_layers=32, phases=16, phys_extent=2112))
    assert lib.ekv_step_resident_rows(ctypes.byref(bank), ctypes.byref(st), F16) >= 0
    # chunk steps at head_dim 128 that the plain call sends to the logits-in-LDS, the resident and the wide kernel
    for c, what in ((_chunk(32, 32, 32, 8, 2056), "lds"), (_chunk(32, 32, 8, 16, 1232), "resident"), (_chunk(32, 32, 32, 96, 5002), "wide")):
        bank, st = _structs(c)
        ref, got = _plain(lib, bank, st, F16), _capped(lib, bank, st, F16, 30.0)
        rd, gd = dict(zip(INFO, ref[2:12])), dict(zip(INFO, got[2:12]))
        assert ref[0] == OK and got[0] == OK, (what, ref, got)
        assert (rd["wide"] == 1 or rd["one_launch"] == 1) and gd["wide"] == 0, (what, rd, gd)
        assert gd["qb_rows"] * (c["hq"] // c["h"]) <= 32 and gd["n_qblocks"] == -(-c["q_len"] // gd["qb_rows"]), (what, gd)
    # the dense prefix at head_dim 128: blocks of 32 rows
    bank, st = _structs(_chunk(32, 32, 32, 4906, 0, policy=0, accumulate=0, n_evict=0))
    got = _capped(lib, bank, st, F16, 50.0)
    gd = dict(zip(INFO, got[2:12]))
    assert got[0] == OK and (gd["wide"], gd["qb_rows"], gd["n_qblocks"]) == (0, 32, 154), gd
    # the refusals, each accepted by the plain call
    refusals = [_case(n_layers=32, rope_on_read=1), _chunk(32, 32, 32, 16, 4096, rope_on_read=1)] + \
               [_case(n_layers=32, head_dim=d) for d in (32, 64, 96)] + [_chunk(32, 32, 32, 16, 4096, d=d) for d in (32, 64, 96)] + \
               [_chunk(4, 40, 1, 8, 400)]
    for c in refusals:
        bank, st = _structs(c)
        assert _plain(lib, bank, st, F16)[0] == OK, c
        assert _refused(_capped(lib, bank, st, F16, 50.0)), c
    # ... while a decode step of GQA factor 40 is served (groups of 8 query heads)
    bank, st = _structs(_case(n_layers=4, hq=40, h=1))
    assert _capped(lib, bank, st, F16, 50.0) == _plain(lib, bank, st, F16)


def test_manifest_holds_the_capped_lines():
    from easykv_amd import _build
    later = dict(_build.later_objects())
    names = [f"ekv_attn_decode_d{d}_cap{e}" for d in (128, 256) for e in ("", "_bf16")] + \
            [f"ekv_attn_chunk_cap_d{d}_m{m}{e}" for d in (128, 256) for m in (0, 1, 2) for e in ("", "_bf16")] + ["ekv_softcap_eval"]
    for name in names:
        assert name in later, name
        assert name == "ekv_softcap_eval" or "-DEKV_SOFTCAP=1" in later[name], name
    assert "-DEKV_D=128" in later["ekv_attn_decode_d128_cap"] and "-DEKV_ROPE=false" in later["ekv_attn_decode_d128_cap"]
    assert "-DEKV_CHUNK_MODE=2" in later["ekv_attn_chunk_cap_d256_m2_bf16"] and "-DEKV_BF16=1" in later["ekv_attn_chunk_cap_d256_m2_bf16"]
    # no other object is built with the switch, and the pinned lists do not know the capped ones
    assert sorted(n for n, a in _build.objects() + _build.added_objects() + _build.later_objects() if "-DEKV_SOFTCAP=1" in a) == sorted(names[:-1])
    assert not [n for n, _ in _build.objects() + _build.added_objects() if "cap" in n]
    assert os.path.exists(_build.LIB) or True


def test_make_step_writes_the_scale(monkeypatch):
    """KVBank.make_step: sm_scale=None writes sqrt(head_dim) exactly as before (the ekv_step is byte-identical), a scale writes 1 / scale."""
    from easykv_amd import engine
    from easykv_amd.engine import KVBank, StepPlan

    def bare(scale):
        b = KVBank.__new__(KVBank)
        b.n_layers, b.n_q_heads, b.n_kv_heads, b.head_dim, b.cap = 2, 4, 2, 128, 256
        b.n_slots, b.extent, b.sm_scale = [70, 70], [70, 70], scale
        return b
    plan = StepPlan(policy="roco", phase="decode", evict=True, budget=64)
    a, b, c = (bare(s).make_step(plan, 1, 0, 2) for s in (None, 128 ** -0.5, 144 ** -0.5))
    ref = bytes(a)
    a.sm_div = math.sqrt(128)
    assert bytes(a) == ref                       # what the bank wrote before the scale existed
    assert abs(b.sm_div - math.sqrt(128)) < 1e-5 and c.sm_div == 12.0
    c.sm_div = a.sm_div
    assert bytes(c) == ref                       # nothing but sm_div differs


def test_python_refusals_come_before_anything_is_allocated(monkeypatch):
    from easykv_amd import _lib, engine
    from easykv_amd._lib import EkvError
    loaded = []
    monkeypatch.setattr(_lib, "load", lambda: loaded.append(1))      # (the first thing a bank does before it allocates)
    for kw, match in ((dict(kv_quant="fp8"), "quantised"), (dict(kv_quant="k16_mxfp4"), "quantised"), (dict(long_rows=True), "long")):
        with pytest.raises(EkvError, match=match):
            engine.KVBank(2, 4, 2, 128, 256, logit_cap=50.0, **kw)
    for d in (32, 64, 96):
        with pytest.raises(EkvError, match="head_dim"):
            engine.KVBank(2, 4, 2, d, 256, logit_cap=50.0)
    for bad in (0.0, -1.0, float("inf"), float("nan"), "50"):
        with pytest.raises(ValueError, match="logit_cap"):
            engine.KVBank(2, 4, 2, 128, 256, logit_cap=bad)
    for bad in (0.0, -0.1, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="sm_scale"):
            engine.KVBank(2, 4, 2, 128, 256, sm_scale=bad)
    with pytest.raises(EkvError, match="batch"):
        engine.KVBankBatch(2, 2, 4, 2, 128, 256, logit_cap=50.0)
    assert loaded == []
    # a capped bank refuses quantize*() and set_rope() (a bank object without storage: the refusals read nothing else)
    b = engine.KVBank.__new__(engine.KVBank)
    b.logit_cap, b.long_rows, b._fmt, b.head_dim, b.n_q_heads, b.n_kv_heads = 50.0, False, None, 128, 4, 2
    for name in ("quantize_fp8", "quantize_mxfp4", "quantize_mxfp6", "quantize_fp8_mxfp4", "quantize_k16_mxfp4"):
        with pytest.raises(EkvError, match="logit_cap"):
            getattr(b, name)()
    with pytest.raises(EkvError, match="soft-capped"):
        b.set_rope(torch.zeros(4, 128), torch.zeros(4, 128))


# ---- the driver over the stub caches ------------------------------------------------------------------------------------------------------
def _model(d=128, **cfg):
    from oracle.fake_model import make_streams
    from tests.native_fake_model import NativeFakeModel
    model = NativeFakeModel(*make_streams(2, 4, 2, d, 96, seed=3), device="cpu")
    for k, v in cfg.items():
        setattr(model.config, k, v)
    return model


def test_driver_hands_cap_and_scale_to_the_cache(monkeypatch):
    from easykv_amd import api
    import tests.test_driver_cpu as TD
    seen = []

    class Cache(TD.StubCache):
        def __init__(self, *a, logit_cap=None, sm_scale=None, **k):
            seen.append((logit_cap, sm_scale))
            self.logit_cap, self.sm_scale = logit_cap, sm_scale
            super().__init__(*a, **k)
    monkeypatch.setattr(api, "BudgetedKVCache", Cache)
    ids = torch.arange(40).view(1, -1) % 16
    gen = dict(budget=16, kv_policy="roco", max_new_tokens=4)
    for cfg, want in ((dict(attn_logit_softcapping=50.0, query_pre_attn_scalar=144), (50.0, 144 ** -0.5)),
                      (dict(attn_logit_softcapping=2.0), (2.0, None)),
                      (dict(attn_logit_softcapping=None, query_pre_attn_scalar=128), (None, None)),      # the standard scale is not named
                      (dict(query_pre_attn_scalar=224), (None, 224 ** -0.5))):
        seen.clear()
        with contextlib.redirect_stdout(io.StringIO()):
            api.generate(_model(**cfg), ids, gen, kv_mode="decoding", stride=1)
        assert seen == [want], (cfg, seen)
    # a model without either key builds its cache exactly as before: the stub of tests/test_driver_cpu.py takes neither keyword
    monkeypatch.setattr(api, "BudgetedKVCache", TD.StubCache)
    with contextlib.redirect_stdout(io.StringIO()):
        api.generate(_model(), ids, gen, kv_mode="decoding", stride=1)


def test_driver_refusals_of_a_capped_model_come_before_any_bank(monkeypatch):
    from easykv_amd import api, engine
    made = []
    monkeypatch.setattr(engine.KVBank, "__init__", lambda self, *a, **k: made.append(1))
    ids = torch.arange(40).view(1, -1) % 16
    gen = dict(budget=16, kv_policy="roco", max_new_tokens=4)
    model = _model(attn_logit_softcapping=50.0)
    for extra, match in ((dict(streaming=True), "streaming"), (dict(kv_quant="fp8"), "kv_quant"), (dict(long_rows=True), "long_rows")):
        with pytest.raises(ValueError, match=match):
            api.generate(model, ids, dict(gen, **extra), kv_mode="decoding", stride=1)
    with pytest.raises(ValueError, match="attn_logit_softcapping"):
        api.generate_batch(model, [ids, ids], gen, kv_mode="decoding", stride=1)
    with pytest.raises(ValueError, match="head_dim"):
        api.generate(_model(d=64, attn_logit_softcapping=50.0), ids, gen, kv_mode="decoding", stride=1)
    with pytest.raises(ValueError, match="finite"):
        api.generate(_model(attn_logit_softcapping=0.0), ids, gen, kv_mode="decoding", stride=1)
    assert made == [] and model.outputs_log == []


def test_generate_batch_takes_a_scale_without_a_cap(monkeypatch):
    from easykv_amd import api
    import tests.test_driver_cpu as TD
    seen = {}

    class Cache(TD.StubCache):
        def __init__(self, *a, sm_scale=None, **k):
            seen.setdefault("cache", []).append(sm_scale)
            super().__init__(*a, **k)

    class Batch(TD.StubBankBatch):
        def __init__(self, *a, sm_scale=None, **k):
            seen["batch"] = sm_scale
            super().__init__(*a, **k)
    monkeypatch.setattr(api, "BudgetedKVCache", Cache)
    monkeypatch.setattr(api, "KVBankBatch", Batch)
    monkeypatch.setattr(api, "BudgetedKVCacheBatch", TD.StubCacheBatch)
    from tests.batch_fake_model import BatchFakeModel
    from oracle.fake_model import make_streams
    model = BatchFakeModel(*make_streams(2, 4, 2, 128, 96, seed=3), device="cpu")
    model.config.query_pre_attn_scalar = 144
    ids = [torch.arange(n).view(1, -1) % 16 for n in (20, 28)]
    with contextlib.redirect_stdout(io.StringIO()):
        api.generate_batch(model, ids, dict(budget=8, kv_policy="roco", max_new_tokens=4), kv_mode="decoding", stride=1)
    assert seen == dict(cache=[144 ** -0.5] * 2, batch=144 ** -0.5), seen


def test_seam_holds_the_modules_arithmetic_against_the_caches(monkeypatch):
    from easykv_amd import api, hf
    q = torch.zeros(1, 2, 1, 128)

    class Cache:
        streaming = False

        def __init__(self, logit_cap=None, sm_scale=None):
            self.logit_cap, self.sm_scale = logit_cap, sm_scale

        def attend(self, layer, q, k, v):
            return q
    mod = SimpleNamespace(layer_idx=0)

    def call(cache, **kw):
        monkeypatch.setattr(api, "active_cache", lambda: cache)
        return hf._easykv_attention(mod, q, q, q, **kw)
    std = 128 ** -0.5
    # a cache without either: today's check and today's message
    call(Cache(), scaling=std)
    call(Cache())
    with pytest.raises(ValueError, match="standard 1/sqrt"):
        call(Cache(), scaling=144 ** -0.5)
    with pytest.raises(ValueError, match="soft-caps"):
        call(Cache(), scaling=std, softcap=50.0)
    # a capped, scaled cache: both must agree with the module's
    c = Cache(50.0, 144 ** -0.5)
    call(c, scaling=144 ** -0.5, softcap=50.0, sliding_window=4096)
    call(c, scaling=144 ** -0.5 * (1 + 5e-4), softcap=50.0)
    for kw in (dict(scaling=std, softcap=50.0), dict(softcap=50.0), dict(scaling=144 ** -0.5), dict(scaling=144 ** -0.5, softcap=30.0)):
        with pytest.raises(ValueError, match="easykv_amd attention"):
            call(c, **kw)
    # a scaled cache without a cap (Gemma-style query_pre_attn_scalar)
    call(Cache(None, 144 ** -0.5), scaling=144 ** -0.5)
    with pytest.raises(ValueError, match="scales its logits"):
        call(Cache(None, 144 ** -0.5), scaling=std)


# ---- the planner as a stand-alone program under the sanitizers ---------------------------------------------------------------------------
@pytest.fixture(scope="module", params=COMPILERS or [None], ids=lambda c: os.path.basename(c) if c else "none")
def program(request, tmp_path_factory):
    if request.param is None:
        pytest.skip("no host C++ compiler on this machine")
    exe = str(tmp_path_factory.mktemp("plan_softcap") / "plan_softcap_main")
    static = ["-static-libasan", "-static-libubsan"] if os.path.basename(request.param) == "g++" else []
    cmd = [request.param, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", *static,
           "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", os.path.join(ROOT, "tests", "plan_softcap_main.cpp"),
           os.path.join(ROOT, "easykv_amd", "csrc", "ekv_plan.cpp"), "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    return exe


CAP_OF = {0: 0.0, -1000: -1.0, -1: float("inf"), -2: float("nan")}


def test_capped_planner_grid_ends_clean_and_answers_as_the_library(program, lib):
    from easykv_amd import _lib as L
    r = subprocess.run([program], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-4000:])      # (a sanitizer report ends the program with a non-zero status)
    lines = r.stdout.splitlines()
    assert len(lines) > 20000
    n = dict(decode_same=0, chunk_ok=0, chunk_128_on_16x16=0, refused=0, arg=0, prefix=0)
    bad = []
    for ln in lines:
        left, right = ln.split("=>")
        capped, plain = right.split("|")
        d, hq, h, layers, cap_rows, q_len, T, policy, n_evict, win_lo, win_tail, roco_k1, range_start, rope, n_split, two_pass, dtype, milli = (int(x) for x in left.split())
        got, ref = [int(x) for x in capped.split()], [int(x) for x in plain.split()]
        assert len(got) == 13 and len(ref) == 12
        softcap = CAP_OF.get(milli, milli / 1000.0)
        bank = L.Bank(256, 256, 256, 256, 256, 256, layers, hq, h, d, cap_rows, 256, 256, 256)
        st = L.Step()
        st.layer_count, st.q_len, st.n_slots, st.policy, st.n_evict, st.win_lo, st.win_tail, st.roco_k1 = layers, q_len, T, policy, n_evict, win_lo, win_tail, roco_k1
        st.range_start, st.rope_on_read, st.n_split, st.two_pass, st.roco_tail, st.causal, st.sm_div = range_start, rope, n_split, two_pass, 10, 1, 12.0
        st.accumulate = 1 if (q_len == 1 or policy != 0) else 0
        st.count_add, st.count_tail_step = (1.0, 0.0) if q_len == 1 else (float(q_len), -1.0)
        want = _capped(lib, bank, st, dtype, softcap)
        want_plain = _plain(lib, bank, st, dtype)
        if [x & (2 ** 64 - 1) for x in want] != [x & (2 ** 64 - 1) for x in got] or \
                [x & (2 ** 64 - 1) for x in want_plain[:1] + want_plain[2:]] != [x & (2 ** 64 - 1) for x in ref]:
            bad.append((ln, want, want_plain))
        info, rep = dict(zip(INFO, got[2:12])), hq // h
        if milli <= 0:
            assert _refused(got, ARG), ln
            n["arg"] += 1
        elif rope or d == 64 or (q_len > 1 and rep > 32):
            assert _refused(got), ln
            n["refused"] += 1
        elif q_len == 1:
            assert got[:1] + got[2:] == ref, ln      # a decode step: the plain call's answers, field for field
            n["decode_same"] += got[0] == OK
        elif got[0] == OK:
            assert info["wide"] == 0 and info["qb_rows"] * rep <= 32 and info["n_qblocks"] == -(-q_len // info["qb_rows"]), ln
            assert not (info["one_launch"] and info["two_pass"]) and got[12] > 0, ln
            n["chunk_ok"] += 1
            n["chunk_128_on_16x16"] += d == 128 and 33 <= rep * q_len <= 128
            n["prefix"] += q_len == T
        else:
            assert _refused(got, got[0]), ln
    assert not bad, (len(bad), bad[:2])
    print(f"capped planner grid: {len(lines)} calls, {n}")
    assert min(n.values()) > 50, n
