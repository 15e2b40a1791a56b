"""Attention sinks without a GPU: dry runs of the sink call family (ekv_sink_*) through the C ABI over fake banks (nothing is dereferenced,
nothing is launched), the new manifest lines, the Python refusals, the driver over the stub caches of tests/test_driver_cpu.py, the seam,
and the planner driven over a sink grid by a stand-alone program under AddressSanitizer + UBSan (tests/plan_sink_main.cpp; the sanitizer
runtimes are linked into the program, which runs as a child process).

What the plans must say: a sink decode step plans as the plain call of the same step — splits, launches, workspace —
except that the mixed phase orders and the resident rows are COMPILED OUT of the sink instances, so info [9] (the phase order) is 0; a
sink chunk step or dense prefix runs on the 16x16x32 kernel in blocks of at most 32 folded rows — never on the wide, the logits-in-LDS or
the logits-resident kernel; RoPE-on-read, a head_dim other than 64 / 128, a GQA factor above 32 in a chunk step
(EKV_E_UNSUPPORTED) and NULL sinks (EKV_E_ARG) are refused with zero launches and zero workspace bytes."""
import contextlib
import ctypes
import io
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
CALLS = ("ekv_sink_step_check", "ekv_sink_step_info", "ekv_sink_workspace_bytes", "ekv_sink_step_attend")
SINKS = ctypes.c_void_p(256)      # (a dummy non-null pointer: the dry runs only test it for NULL)


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


def _sink(lib, bank, st, dtype, sinks=SINKS):
    b, s = ctypes.byref(bank), ctypes.byref(st)
    info = (ctypes.c_int32 * 10)(*([-7] * 10))
    return [lib.ekv_sink_step_check(b, s, dtype, sinks), lib.ekv_sink_step_info(b, s, dtype, sinks, info, 10)] + list(info) + [lib.ekv_sink_workspace_bytes(b, s, dtype, sinks)]


def _order_f(ref):
    """The plain call's answers with the phase order (info [9]) set to F: what the sink call of a decode step must answer."""
    return ref[:11] + [0] + ref[12:]


def _refused(got, code=UNSUPPORTED):
    """The sink call's answer is `code`, with zero launches and zero bytes."""
    d = dict(zip(INFO, got[2:12]))
    return got[0] == code and got[12] == 0 and (got[1] != 0 or (d["n_launches"] == 0 and d["one_launch"] == 0))


def test_sink_calls_are_exported_and_declared(lib):
    from easykv_amd import _lib as L
    header = open(os.path.join(ROOT, "include", "easykv_hip.h")).read()
    declared = set(re.findall(r"\b(ekv_[a-z0-9_]+)\s*\(", header))
    raw = ctypes.CDLL(L.LIB)
    for name in CALLS:
        assert name in declared and name in L.EXPORTS and hasattr(raw, name), name
    assert lib.ekv_abi_version() == 8
    assert "p_j = exp(s_j - M) / (sum_i exp(s_i - M) + exp(a - M))" in header and "M   = max(max_j s_j, a)" in header
    # argument checks come before any device access
    assert lib.ekv_sink_step_check(None, None, F16, SINKS) == ARG
    assert lib.ekv_sink_workspace_bytes(None, None, F16, SINKS) == 0
    # no public struct changed (tests/test_host_cpu.py pins ekv_bank and ekv_step): the sinks are an argument of the four calls
    assert not re.search(r"sinks\s*;", header)


def test_sink_dry_runs_over_the_dispatch_grid(lib):
    n = dict(decode_ok=0, fused=0, split=0, ordered=0, chunk_ok=0, chunk_33_128=0, refused=0, arg=0)
    for c in cases():
        bank, st = _structs(c)
        rep = c["hq"] // c["h"]
        served = c["head_dim"] in (64, 128) and not c["rope_on_read"]
        for dt in (F16, BF16):
            ref, got = _plain(lib, bank, st, dt), _sink(lib, bank, st, dt)
            if ref[0] == ARG:                                   # the plain call's own argument errors keep their code
                assert _refused(got, ARG), (c, got)
                n["arg"] += 1
            elif c["q_len"] == 1:
                if ref[0] == OK and served:                     # a decode step: the plain call's plan and workspace, in phase order F
                    assert got == _order_f(ref), (c, got, ref)
                    n["decode_ok"] += 1
                    n["fused"] += got[3] == 1
                    n["split"] += got[2] > 1
                    n["ordered"] += ref[11] != 0               # (steps whose plain call mixes the phase orders)
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
                    # blocks of at most 32 folded rows on the 16x16 kernel; never the wide, the logits-in-LDS or the resident kernel
                    assert d["wide"] == 0 and d["qb_rows"] * rep <= 32 and d["n_qblocks"] == -(-c["q_len"] // d["qb_rows"]), (c, d)
                    assert not (d["one_launch"] and d["two_pass"]), (c, d)
                    assert not d["one_launch"] or (d["n_qblocks"] == 1 and d["n_split"] == 1 and d["n_launches"] == 1), (c, d)
                    assert got[12] > 0 and (d["n_launches"] >= 1 or (ref[0] == OK and ref[10] == 0)), (c, got, ref)
                    n["chunk_ok"] += 1
                    n["chunk_33_128"] += 33 <= rep * c["q_len"] <= 128
        assert _refused(_sink(lib, bank, st, F16, None), ARG), c                                       # NULL sinks
        assert lib.ekv_sink_step_check(ctypes.byref(bank), ctypes.byref(st), 2, SINKS) == ARG          # ... behind the element type
        assert lib.ekv_sink_step_check(ctypes.byref(bank), ctypes.byref(st), 2, None) == ARG
    print("sink dry runs over the dispatch grid:", n)
    assert n["decode_ok"] > 100 and n["fused"] > 10 and n["split"] > 10 and n["chunk_ok"] > 100 and n["chunk_33_128"] > 20 and n["refused"] > 100, n


def test_sink_plans_and_refusals_by_name(lib):
    # the north-star decode step on either score-row layout: the plain plan, with the phase orders and the resident rows compiled out
    # (the choice this test pins — info [9] = 0 where the plain call mixes the orders)
    for extra in ({}, {"phases": 16, "phys_extent": 2112}):
        bank, st = _structs(_case(n_layers=32, **extra))
        ref, got = _plain(lib, bank, st, F16), _sink(lib, bank, st, F16)
        assert ref[0] == OK and ref[3] == 1 and got == _order_f(ref), (ref, got)
    bank, st = _structs(_case(n_layers=4, n_split=1, phases=16, phys_extent=2112))      # (4-wave slot-indexed launch: the plain call's order K candidates)
    ref, got = _plain(lib, bank, st, F16), _sink(lib, bank, st, F16)
    assert got == _order_f(ref) and got[11] == 0, (ref, got)
    # gpt-oss's shape: head_dim 64, 64 query heads over 8 KV heads, all 24 / 36 layers in one call
    for layers in (24, 36):
        bank, st = _structs(_case(n_layers=layers, head_dim=64, hq=64, h=8))
        ref, got = _plain(lib, bank, st, BF16), _sink(lib, bank, st, BF16)
        assert ref[0] == OK and got == _order_f(ref), (ref, got)
    # chunk steps that the plain call sends to the logits-in-LDS, the resident and the wide kernel
    for c, what in ((_chunk(32, 32, 32, 8, 2056), "lds"), (_chunk(32, 32, 8, 16, 1232), "resident"), (_chunk(32, 32, 32, 96, 5002), "wide"),
                    (_chunk(24, 64, 8, 8, 2056, d=64), "gpt-oss stride 8")):
        bank, st = _structs(c)
        ref, got = _plain(lib, bank, st, F16), _sink(lib, bank, st, F16)
        rd, gd = dict(zip(INFO, ref[2:12])), dict(zip(INFO, got[2:12]))
        assert ref[0] == OK and got[0] == OK, (what, ref, got)
        assert (rd["wide"] == 1 or rd["one_launch"] == 1) and gd["wide"] == 0, (what, rd, gd)
        assert gd["qb_rows"] * (c["hq"] // c["h"]) <= 32 and gd["n_qblocks"] == -(-c["q_len"] // gd["qb_rows"]), (what, gd)
    # one unsplit block: one pass with the scorer as the kernel's tail, one launch
    bank, st = _structs(_chunk(2, 16, 2, 4, 200, d=64, n_split=1))
    gd = dict(zip(INFO, _sink(lib, bank, st, F16)[2:12]))
    assert (gd["one_launch"], gd["two_pass"], gd["n_qblocks"], gd["n_launches"]) == (1, 0, 1, 1), gd
    # the dense prefix at head_dim 128: blocks of 32 rows
    bank, st = _structs(_chunk(32, 32, 32, 4906, 0, policy=0, accumulate=0, n_evict=0))
    got = _sink(lib, bank, st, F16)
    gd = dict(zip(INFO, got[2:12]))
    assert got[0] == OK and (gd["wide"], gd["qb_rows"], gd["n_qblocks"]) == (0, 32, 154), gd
    # the refusals, each accepted by the plain call
    refusals = [_case(n_layers=32, rope_on_read=1), _chunk(32, 32, 32, 16, 4096, rope_on_read=1)] + \
               [_case(n_layers=32, head_dim=d) for d in (32, 96, 256)] + [_chunk(32, 32, 32, 16, 4096, d=d) for d in (32, 96, 256)] + \
               [_chunk(4, 40, 1, 8, 400)]
    for c in refusals:
        bank, st = _structs(c)
        assert _plain(lib, bank, st, F16)[0] == OK, c
        assert _refused(_sink(lib, bank, st, F16)), c
    # the head-mean TOVA row (encoding / ppl mode) is served: its launch is in the plan, as in the plain call's
    for d, hq, h in ((128, 32, 32), (64, 16, 2)):
        bank, st = _structs(_chunk(2, hq, h, 4, 300, d=d, policy=3, tova_head_mean=1))
        ref, got = _plain(lib, bank, st, F16), _sink(lib, bank, st, F16)
        assert ref[0] == OK and got[0] == OK and got[10] >= 2 and got[12] > 0, (ref, got)
    # ... while a decode step of GQA factor 40 is served (groups of 8 query heads)
    bank, st = _structs(_case(n_layers=4, hq=40, h=1))
    assert _sink(lib, bank, st, F16) == _order_f(_plain(lib, bank, st, F16))


def test_manifest_holds_exactly_the_sink_lines():
    from easykv_amd import _build
    later = dict(_build.later_objects())
    names = [f"ekv_attn_decode_d{d}_sink{e}" for d in (64, 128) for e in ("", "_bf16")] + \
            [f"ekv_decode_score_sink{e}" for e in ("", "_bf16")] + \
            [f"ekv_attn_chunk_sink_d{d}_m{m}{e}" for d in (64, 128) for m in (0, 1, 2) for e in ("", "_bf16")] + ["ekv_tova_headmean_sink"]
    for name in names:
        assert name in later and "-DEKV_SINK=1" in later[name], name
    assert "-DEKV_D=64" in later["ekv_attn_decode_d64_sink"] and "-DEKV_ROPE=false" in later["ekv_attn_decode_d64_sink"]
    assert "-DEKV_CHUNK_MODE=2" in later["ekv_attn_chunk_sink_d128_m2_bf16"] and "-DEKV_BF16=1" in later["ekv_attn_chunk_sink_d128_m2_bf16"]
    # no other object is built with the switch, no sink object with another feature's, and the pinned lists do not know the sink ones
    everything = _build.objects() + _build.added_objects() + _build.later_objects()
    assert sorted(n for n, a in everything if "-DEKV_SINK=1" in a) == sorted(names)
    assert sorted(n for n, _ in everything if "sink" in n) == sorted(names)
    assert not [n for n in names if any(sw in " ".join(later[n]) for sw in ("EKV_SOFTCAP", "EKV_KV", "EKV_BATCH", "EKV_ROPE=true"))]
    assert not [n for n, _ in _build.objects() + _build.added_objects() if "sink" in n]
    fams = [f for f, _ in _build.later_instances() if "SINK" in f]
    assert fams.count("EKV_DECODE_SINK") == 4 and fams.count("EKV_DECODE_SCORE_SINK") == 2 and fams.count("EKV_CHUNK_SINK") == 12
    assert fams.count("EKV_TOVA_MEAN_SINK") == 1 and "-DEKV_SS_NT=512" in later["ekv_tova_headmean_sink"]
    assert all(f in _build.FAMILIES for f in fams)


def test_python_refusals_come_before_anything_is_allocated(monkeypatch):
    from easykv_amd import _lib, engine
    from easykv_amd._lib import EkvError
    loaded = []
    monkeypatch.setattr(_lib, "load", lambda: loaded.append(1))      # (the first thing a bank does before it allocates)
    sinks = torch.zeros(2, 4)
    for kw, match in ((dict(kv_quant="fp8"), "quantised"), (dict(kv_quant="k16_mxfp4"), "quantised"), (dict(long_rows=True), "long"),
                      (dict(logit_cap=50.0), "capped")):
        with pytest.raises(EkvError, match=match):
            engine.KVBank(2, 4, 2, 128, 256, sinks=sinks, **kw)
    for d in (32, 96, 256):
        with pytest.raises(EkvError, match="head_dim"):
            engine.KVBank(2, 4, 2, d, 256, sinks=sinks)
    for bad in (torch.zeros(2, 5), torch.zeros(4, 2), torch.zeros(8), [[0.0] * 4] * 2):
        with pytest.raises(ValueError, match="shape"):
            engine.KVBank(2, 4, 2, 128, 256, sinks=bad)
    for v in (float("inf"), float("-inf"), float("nan")):
        bad = torch.zeros(2, 4)
        bad[1, 2] = v
        with pytest.raises(ValueError, match="finite"):
            engine.KVBank(2, 4, 2, 64, 256, sinks=bad)
    with pytest.raises(EkvError, match="batch"):
        engine.KVBankBatch(2, 2, 4, 2, 128, 256, sinks=sinks)
    assert loaded == []
    # a sink bank refuses quantize*() and set_rope() (a bank object without storage: the refusals read nothing else)
    b = engine.KVBank.__new__(engine.KVBank)
    b.sinks, b.logit_cap, b.long_rows, b._fmt, b.head_dim, b.n_q_heads, b.n_kv_heads = sinks, None, False, None, 128, 4, 2
    for name in ("quantize_fp8", "quantize_mxfp4", "quantize_mxfp6", "quantize_fp8_mxfp4", "quantize_k16_mxfp4"):
        with pytest.raises(EkvError, match="sinks"):
            getattr(b, name)()
    with pytest.raises(EkvError, match="sink"):
        b.set_rope(torch.zeros(4, 128), torch.zeros(4, 128))
    assert b.resident_rows(engine.StepPlan(policy="roco", phase="decode")) == 0


# ---- the driver over the stub caches ------------------------------------------------------------------------------------------------------
def _model(d=64, hq=4, h=2, sinks=None, **cfg):
    from oracle.fake_model import make_streams
    from tests.native_fake_model import NativeFakeModel
    model = NativeFakeModel(*make_streams(2, hq, h, d, 96, seed=3), device="cpu")
    for k, v in cfg.items():
        setattr(model.config, k, v)
    if sinks is not None:      # what a stock gpt-oss has: one module per layer with a `sinks` parameter and an integer layer_idx
        mods = [SimpleNamespace(sinks=torch.nn.Parameter(sinks[i].clone()), layer_idx=i) for i in range(sinks.shape[0])]
        mods += [SimpleNamespace(sinks=torch.zeros(3), layer_idx=0), SimpleNamespace(sinks=None, layer_idx=1), SimpleNamespace(weight=1)]
        model.modules = lambda: iter(mods)
    return model


def test_driver_collects_the_sinks_and_hands_them_to_the_cache(monkeypatch):
    from easykv_amd import api
    import tests.test_driver_cpu as TD
    seen = []

    class Cache(TD.StubCache):
        def __init__(self, *a, sinks=None, **k):
            seen.append(sinks)
            self.sinks = sinks
            super().__init__(*a, **k)
    monkeypatch.setattr(api, "BudgetedKVCache", Cache)
    ids = torch.arange(40).view(1, -1) % 16
    gen = dict(budget=16, kv_policy="roco", max_new_tokens=4)
    sinks = torch.randn(2, 4, generator=torch.Generator().manual_seed(11)) + 1
    for model, cfg in ((_model(sinks=sinks), gen), (_model(), dict(gen, attention_sinks=sinks)), (_model(), dict(gen, attention_sinks=sinks.tolist())),
                       (_model(d=128, sinks=sinks.half()), gen)):
        seen.clear()
        with contextlib.redirect_stdout(io.StringIO()):
            api.generate(model, ids, cfg, kv_mode="decoding", stride=1)
        assert len(seen) == 1 and seen[0].dtype == torch.float32 and tuple(seen[0].shape) == (2, 4), seen
        assert torch.allclose(seen[0], sinks, atol=2e-3), seen
    assert torch.equal(api._collect_sinks(_model(sinks=sinks), {}, 2, 4), sinks)
    assert api._collect_sinks(_model(), {}, 2, 4) is None
    # a model without sinks builds its cache exactly as before: the stub of tests/test_driver_cpu.py takes no such keyword
    monkeypatch.setattr(api, "BudgetedKVCache", TD.StubCache)
    with contextlib.redirect_stdout(io.StringIO()):
        api.generate(_model(), ids, gen, kv_mode="decoding", stride=1)
    # a wrong shape, or sinks on some layers only
    with pytest.raises(ValueError, match="attention_sinks"):
        api.generate(_model(), ids, dict(gen, attention_sinks=torch.zeros(2, 5)), kv_mode="decoding", stride=1)
    with pytest.raises(ValueError, match="all or none"):
        api._collect_sinks(_model(sinks=sinks[:1]), {}, 2, 4)


def test_driver_refusals_of_a_sink_model_come_before_any_bank(monkeypatch):
    from easykv_amd import api, engine
    made = []
    monkeypatch.setattr(engine.KVBank, "__init__", lambda self, *a, **k: made.append(1))
    ids = torch.arange(40).view(1, -1) % 16
    gen = dict(budget=16, kv_policy="roco", max_new_tokens=4)
    sinks = torch.zeros(2, 4)
    model = _model(sinks=sinks)
    for extra, match in ((dict(streaming=True), "streaming"), (dict(kv_quant="fp8"), "kv_quant"), (dict(long_rows=True), "long_rows")):
        with pytest.raises(ValueError, match=match):
            api.generate(model, ids, dict(gen, **extra), kv_mode="decoding", stride=1)
    with pytest.raises(ValueError, match="attention sinks"):
        api.generate_batch(model, [ids, ids], gen, kv_mode="decoding", stride=1)
    with pytest.raises(ValueError, match="attention sinks"):
        api.generate_batch(_model(), [ids, ids], dict(gen, attention_sinks=sinks), kv_mode="decoding", stride=1)
    with pytest.raises(ValueError, match="attn_logit_softcapping"):
        api.generate(_model(d=128, sinks=sinks, attn_logit_softcapping=50.0), ids, gen, kv_mode="decoding", stride=1)
    with pytest.raises(ValueError, match="head_dim"):
        api.generate(_model(d=96, sinks=sinks), ids, gen, kv_mode="decoding", stride=1)
    sharded = _model(sinks=sinks)
    sharded.layer_shard = SimpleNamespace(world=2, begin=0, count=1, end=1, n_layers=2, rank=0)
    with pytest.raises(ValueError, match="layer-sharded"):
        api.generate(sharded, ids, gen, kv_mode="decoding", stride=1)
    assert made == [] and model.outputs_log == []


def test_seam_raises_on_each_mismatch_and_is_silent_without_sinks(monkeypatch):
    from easykv_amd import api, hf
    q = torch.zeros(1, 4, 1, 64)
    rows = torch.randn(2, 4, generator=torch.Generator().manual_seed(5))

    class Cache:
        streaming, sm_scale, logit_cap, layer_begin = False, None, None, 0

        def __init__(self, sinks=None):
            self.sinks, self._sinks_checked, self.calls = sinks, set(), 0

        def attend(self, layer, q, k, v):
            self.calls += 1
            return q

    def call(cache, layer=0, **kw):
        monkeypatch.setattr(api, "active_cache", lambda: cache)
        return hf._easykv_attention(SimpleNamespace(layer_idx=layer), q, q, q, **kw)
    std = 64 ** -0.5
    # neither side has sinks: today's checks and today's messages
    plain = Cache()
    call(plain, scaling=std, sliding_window=128)
    call(plain)
    with pytest.raises(ValueError, match="standard 1/sqrt"):
        call(plain, scaling=80 ** -0.5)
    assert plain.calls == 2 and plain._sinks_checked == set()
    # 1. the module passes sinks, the cache has none
    with pytest.raises(ValueError, match="cache has none"):
        call(Cache(), scaling=std, s_aux=rows[0])
    # 2. the cache has sinks, the module passes none
    with pytest.raises(ValueError, match="passes none"):
        call(Cache(rows), scaling=std)
    # 3. another layer's row          4. another number of heads
    with pytest.raises(ValueError, match="differ"):
        call(Cache(rows), layer=0, scaling=std, s_aux=rows[1])
    with pytest.raises(ValueError, match="attention sinks"):
        call(Cache(rows), scaling=std, s_aux=rows[0][:3])
    # agreement, within 1e-3 relative, in the model's dtype; checked once per (cache, layer)
    c = Cache(rows)
    call(c, layer=0, scaling=std, s_aux=torch.nn.Parameter(rows[0] * (1 + 5e-4)), sliding_window=128)
    call(c, layer=1, scaling=std, s_aux=rows[1])
    assert c._sinks_checked == {0, 1} and c.calls == 2
    # the second time nothing of s_aux is read: no comparison, so no host sync in the decode loop (an object without a tensor's methods passes)
    call(c, layer=0, scaling=std, s_aux=SimpleNamespace())
    assert c.calls == 3
    with pytest.raises(AttributeError):
        call(Cache(rows), layer=0, scaling=std, s_aux=SimpleNamespace())


# ---- the planner as a stand-alone program under the sanitizers ---------------------------------------------------------------------------
@pytest.fixture(scope="module", params=COMPILERS or [None], ids=lambda c: os.path.basename(c) if c else "none")
def program(request, tmp_path_factory):
    if request.param is None:
        pytest.skip("no host C++ compiler on this machine")
    exe = str(tmp_path_factory.mktemp("plan_sink") / "plan_sink_main")
    static = ["-static-libasan", "-static-libubsan"] if os.path.basename(request.param) == "g++" else []
    cmd = [request.param, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", *static,
           "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", os.path.join(ROOT, "tests", "plan_sink_main.cpp"),
           os.path.join(ROOT, "easykv_amd", "csrc", "ekv_plan.cpp"), "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    return exe


def test_sink_planner_grid_ends_clean_and_answers_as_the_library(program, lib):
    from easykv_amd import _lib as L
    r = subprocess.run([program], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-4000:])      # (a sanitizer report ends the program with a non-zero status)
    lines = r.stdout.splitlines()
    assert len(lines) > 20000
    n = dict(decode_same=0, chunk_ok=0, chunk_on_16x16=0, refused=0, arg=0, prefix=0, one_pass_tail=0, two_pass=0)
    bad = []
    for ln in lines:
        left, right = ln.split("=>")
        sink, plain = right.split("|")
        (d, hq, h, layers, cap_rows, q_len, T, policy, n_evict, win_lo, win_tail, roco_k1, range_start, rope, n_split, two_pass, dtype, head_mean,
         null) = (int(x) for x in left.split())
        got, ref = [int(x) for x in sink.split()], [int(x) for x in plain.split()]
        assert len(got) == 13 and len(ref) == 12
        bank = L.Bank(256, 256, 256, 256, 256, 256, layers, hq, h, d, cap_rows, 256, 256, 256)
        st = L.Step()
        st.layer_count, st.q_len, st.n_slots, st.policy, st.n_evict, st.win_lo, st.win_tail, st.roco_k1 = layers, q_len, T, policy, n_evict, win_lo, win_tail, roco_k1
        st.range_start, st.rope_on_read, st.n_split, st.two_pass, st.roco_tail, st.causal, st.sm_div = range_start, rope, n_split, two_pass, 10, 1, 8.0
        st.tova_head_mean = head_mean
        st.accumulate = 1 if (q_len == 1 or policy != 0) else 0
        st.count_add, st.count_tail_step = (1.0, 0.0) if q_len == 1 else (float(q_len), -1.0)
        want = _sink(lib, bank, st, dtype, None if null else SINKS)
        want_plain = _plain(lib, bank, st, dtype)
        if [x & (2 ** 64 - 1) for x in want] != [x & (2 ** 64 - 1) for x in got] or \
                [x & (2 ** 64 - 1) for x in want_plain[:1] + want_plain[2:]] != [x & (2 ** 64 - 1) for x in ref]:
            bad.append((ln, want, want_plain))
        info, rep = dict(zip(INFO, got[2:12])), hq // h
        if null:
            assert _refused(got, ARG), ln
            n["arg"] += 1
        elif rope or d not in (64, 128) or (q_len > 1 and rep > 32):
            assert _refused(got), ln
            n["refused"] += 1
        elif q_len == 1:
            assert got[:1] + got[2:11] + got[12:] == ref[:10] + ref[11:] and got[11] == 0, ln      # the plain call's answers, in phase order F
            n["decode_same"] += got[0] == OK
        elif got[0] == OK:
            assert info["wide"] == 0 and info["qb_rows"] * rep <= 32 and info["n_qblocks"] == -(-q_len // info["qb_rows"]), ln
            assert not (info["one_launch"] and info["two_pass"]) and got[12] > 0, ln
            n["chunk_ok"] += 1
            n["chunk_on_16x16"] += 33 <= rep * q_len <= 128
            n["prefix"] += q_len == T
            n["one_pass_tail"] += info["one_launch"] == 1
            n["two_pass"] += info["two_pass"] == 1
        else:
            assert _refused(got, got[0]), ln
    assert not bad, (len(bad), bad[:2])
    print(f"sink planner grid: {len(lines)} calls, {n}")
    assert min(n.values()) > 50, n
