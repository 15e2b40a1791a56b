"""Sliding windows without a GPU: dry runs of the window call family (ekv_win_*) through the C ABI over fake banks (nothing is
dereferenced, nothing is launched), the new manifest lines, the Python refusals, the reference helper, and the seeded cases of the GPU
test run on the oracle alone.

What the plans must say: a window decode step plans as the SINK call of the same step, with or without sinks — the plain
call's splits, launches and workspace in phase order F without resident rows (info [9] = 0), no launch of its own for the token
positions; a chunk step or dense prefix plans as the sink call's (the 16x16x32 kernel in blocks of at most 32 folded rows, wide = 0);
RoPE-on-read, a head_dim other than 128 (no sinks) or 64 (sinks) and whatever the sink call refuses are refused
with zero launches and zero workspace bytes (EKV_E_UNSUPPORTED); a NULL struct, NULL tok_pos / windows, a negative
q_pos0 and a negative entry of the host copy of the windows are argument errors (EKV_E_ARG)."""
import ctypes
import os
import re

import pytest
import torch

from tests.test_dispatch_table import _case, _chunk, _structs, cases
from tests.test_sink_cpu import ARG, BF16, F16, INFO, OK, SINKS, UNSUPPORTED, _order_f, _plain, _refused, _sink

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("ekv_win_step_check", "ekv_win_step_info", "ekv_win_workspace_bytes", "ekv_win_step_attend")
PTR = 256      # (a dummy non-null pointer: the dry runs only test it for NULL)


@pytest.fixture(scope="module")
def lib():
    from easykv_amd import _build, _lib
    if not os.path.exists(_build.LIB):
        _build.build_lib()
    return _lib.load()


def _win_struct(n_layers, sinks=False, host=None, tok_pos=PTR, windows=PTR, q_pos0=7):
    from easykv_amd._lib import Win
    arr = (ctypes.c_int32 * n_layers)(*(host if host is not None else [0] * n_layers))
    w = Win(tok_pos, windows, arr if host is not None else None, PTR if sinks else None, q_pos0)
    w._keep = arr
    return w


def _win(lib, bank, st, dtype, w):
    b, s = ctypes.byref(bank), ctypes.byref(st)
    wp = ctypes.byref(w) if w is not None else None
    info = (ctypes.c_int32 * 10)(*([-7] * 10))
    return [lib.ekv_win_step_check(b, s, dtype, wp), lib.ekv_win_step_info(b, s, dtype, wp, info, 10)] + list(info) + [lib.ekv_win_workspace_bytes(b, s, dtype, wp)]


def test_window_calls_are_exported_and_declared(lib):
    from easykv_amd import _lib as L
    header = open(os.path.join(ROOT, "include", "easykv_hip.h")).read()
    declared = set(re.findall(r"\b(ekv_[a-z0-9_]+)\s*\(", header))
    raw = ctypes.CDLL(L.LIB)
    for name in CALLS:
        assert name in declared and name in L.EXPORTS and hasattr(raw, name), name
    assert lib.ekv_abi_version() == 8
    assert "the key is attended  iff  W_l == 0  or  p_q - p_k < W_l" in header and "A masked key is still LIVE" in header
    # the struct of the header and the ctypes one: the same fields in the same order
    body = re.search(r"typedef struct ekv_win \{(.*?)\} ekv_win;", header, re.S).group(1)
    assert re.findall(r"\*?\s*(\w+);", body) == [f[0] for f in L.Win._fields_]
    # argument checks come before any device access
    assert lib.ekv_win_step_check(None, None, F16, None) == ARG
    assert lib.ekv_win_workspace_bytes(None, None, F16, None) == 0
    # no existing public struct changed (tests/test_host_cpu.py pins ekv_bank and ekv_step)
    for name in ("ekv_bank", "ekv_step"):
        assert "tok_pos" not in re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), header, re.S).group(1)


def test_window_dry_runs_over_the_dispatch_grid(lib):
    n = dict(alone_ok=0, sink_ok=0, fused=0, split=0, ordered=0, refused=0, arg=0, chunk_ok=0)
    for c in cases():
        bank, st = _structs(c)
        for dt in (F16, BF16):
            ref = _plain(lib, bank, st, dt)
            for with_sinks in (False, True):
                got = _win(lib, bank, st, dt, _win_struct(c["n_layers"], with_sinks, host=[3] + [0] * (c["n_layers"] - 1)))
                served = c["head_dim"] == (64 if with_sinks else 128) and not c["rope_on_read"]
                snk = _sink(lib, bank, st, dt)
                if ref[0] == ARG:                                   # the plain call's own argument errors keep their code
                    assert _refused(got, ARG), (c, got)
                    n["arg"] += 1
                elif snk[0] == OK and served:
                    # every field is the sink call's of the same step — with sinks or without; a decode step: the plain call's in phase order F
                    assert got == snk and (c["q_len"] > 1 or got == _order_f(ref)), (c, got, ref)
                    d = dict(zip(INFO, got[2:12]))
                    assert c["q_len"] == 1 or (d["wide"] == 0 and d["qb_rows"] * (c["hq"] // c["h"]) <= 32), (c, d)
                    n["sink_ok" if with_sinks else "alone_ok"] += 1
                    n["fused"] += got[3] == 1
                    n["split"] += got[2] > 1
                    n["ordered"] += ref[11] != 0               # (steps whose plain call mixes the phase orders)
                    n["chunk_ok"] += c["q_len"] > 1
                else:
                    assert _refused(got), (c, got, ref)
                    n["refused"] += 1
        L = c["n_layers"]
        for w in (None, _win_struct(L, tok_pos=None), _win_struct(L, windows=None), _win_struct(L, q_pos0=-1), _win_struct(L, host=[0] * (L - 1) + [-1]),
                  _win_struct(L, True, host=[-5] + [0] * (L - 1))):
            assert _refused(_win(lib, bank, st, F16, w), ARG), c
        assert lib.ekv_win_step_check(ctypes.byref(bank), ctypes.byref(st), 2, ctypes.byref(_win_struct(L))) == ARG      # ... behind the element type
    print("window dry runs over the dispatch grid:", n)
    assert n["alone_ok"] > 50 and n["sink_ok"] > 20 and n["fused"] > 10 and n["split"] > 10 and n["refused"] > 100 and n["chunk_ok"] > 100, n


def test_window_plans_and_refusals_by_name(lib):
    # the north-star decode step on either score-row layout: the sink call's plan (phase orders and resident rows compiled out)
    for extra in ({}, {"phases": 16, "phys_extent": 2112}):
        bank, st = _structs(_case(n_layers=32, **extra))
        ref, got = _plain(lib, bank, st, F16), _win(lib, bank, st, F16, _win_struct(32))
        assert ref[0] == OK and ref[3] == 1 and got == _order_f(ref) == _sink(lib, bank, st, F16), (ref, got)
    # gpt-oss's shape: head_dim 64, 64 query heads over 8 KV heads, all 24 / 36 layers in one call, windows on every other layer
    for layers in (24, 36):
        bank, st = _structs(_case(n_layers=layers, head_dim=64, hq=64, h=8))
        got = _win(lib, bank, st, BF16, _win_struct(layers, True, host=[128, 0] * (layers // 2)))
        assert got[0] == OK and got == _sink(lib, bank, st, BF16), got
        assert _refused(_win(lib, bank, st, BF16, _win_struct(layers, False)))      # ... and has no window-alone instance
    # the refusals, each accepted by the sink call (or, at head_dim 128 without sinks, the plain one)
    for c, sinks in ((_case(n_layers=32, head_dim=64, hq=64, h=8), False), (_case(n_layers=32), True),
                     (_chunk(2, 16, 2, 4, 200, d=64, n_split=1), False), (_chunk(32, 32, 32, 16, 4096), True)):
        bank, st = _structs(c)
        assert _sink(lib, bank, st, F16)[0] == OK, c
        assert _refused(_win(lib, bank, st, F16, _win_struct(c["n_layers"], sinks))), c
    # chunk steps and the dense prefix: the sink call's plan — one unsplit block in one launch with the scorer tail, blocks of 32 rows
    for c, sinks in ((_chunk(2, 16, 2, 4, 200, d=64, n_split=1), True), (_chunk(32, 32, 32, 16, 4096), False),
                     (_chunk(32, 32, 32, 4906, 0, policy=0, accumulate=0, n_evict=0), False), (_chunk(24, 64, 8, 8, 2056, d=64), True),
                     # ... and the head-mean TOVA row (encoding / ppl mode): its launch is in the plan, as in the sink call's
                     (_chunk(2, 32, 32, 4, 300, policy=3, tova_head_mean=1), False), (_chunk(2, 16, 2, 4, 300, d=64, policy=3, tova_head_mean=1), True)):
        bank, st = _structs(c)
        got = _win(lib, bank, st, F16, _win_struct(c["n_layers"], sinks))
        assert got[0] == OK and got == _sink(lib, bank, st, F16) and dict(zip(INFO, got[2:12]))["wide"] == 0, (c, got)
    for c in (_case(n_layers=32, rope_on_read=1), _case(n_layers=32, head_dim=256), _case(n_layers=32, head_dim=96)):
        bank, st = _structs(c)
        assert _plain(lib, bank, st, F16)[0] == OK, c
        assert _refused(_win(lib, bank, st, F16, _win_struct(32))), c
    # a decode step of GQA factor 40 is served (groups of 8 query heads), as the sink call serves it
    bank, st = _structs(_case(n_layers=4, hq=40, h=1))
    assert _win(lib, bank, st, F16, _win_struct(4)) == _order_f(_plain(lib, bank, st, F16))


def test_manifest_holds_exactly_the_window_lines():
    from easykv_amd import _build
    later = dict(_build.later_objects())
    names = [f"ekv_attn_decode_d128_win{e}" for e in ("", "_bf16")] + [f"ekv_attn_decode_d64_saux_win{e}" for e in ("", "_bf16")]
    chunk = [f"ekv_attn_chunk_win_d128_m{m}{e}" for m in (0, 1, 2) for e in ("", "_bf16")] + \
            [f"ekv_attn_chunk_saux_win_d64_m{m}{e}" for m in (0, 1, 2) for e in ("", "_bf16")]
    for name in names:
        assert name in later and later[name][-1].endswith("ekv_attn_decode.inc") and "-DEKV_ROPE=false" in later[name], name
    for name in chunk:
        assert name in later and later[name][-1].endswith("ekv_attn_chunk.inc") and f"-DEKV_CHUNK_MODE={name.split('_m')[1][0]}" in later[name], name
    names = names[:2] + chunk[:6] + names[2:] + chunk[6:]
    everything = _build.objects() + _build.added_objects() + _build.later_objects()
    assert sorted(n for n, a in everything if any(x.startswith("-DEKV_WINDOW") for x in a)) == sorted(names)
    assert sorted(n for n, _ in everything if "win" in n) == sorted(names)
    assert all("-DEKV_WINDOW=1" in later[n] and "-DEKV_D=128" in later[n] for n in names[:8])
    assert all("-DEKV_WINDOW=2" in later[n] and "-DEKV_D=64" in later[n] for n in names[8:])      # (window + sinks as one switch: _build.py)
    assert not [n for n in names if any(sw in " ".join(later[n]) for sw in ("EKV_SOFTCAP", "EKV_KV", "EKV_BATCH", "EKV_ROPE=true"))]
    fams = [f for f, _ in _build.later_instances() if "WIN" in f]
    assert fams.count("EKV_DECODE_WIN") == 2 and fams.count("EKV_DECODE_SINK_WIN") == 2 and len(fams) == 16
    assert fams.count("EKV_CHUNK_WIN") == 6 and fams.count("EKV_CHUNK_SINK_WIN") == 6
    assert all(f in _build.FAMILIES for f in fams)
    for src, marks in (("ekv_attn_decode.inc", ('#error "window decode instances',)), ("ekv_decode_stream.h", ("win.tok_pos[head_row + slot_new] = win.q_pos0",)),
                       ("ekv_attn_chunk.inc", ('#error "window chunk instances', "win.tok_pos[head_row + s_slot[j - t0]] = win.q_pos0 + (j - t_new)"))):
        text = open(os.path.join(_build.CSRC, src)).read()
        assert all(m in text for m in marks), src


def test_python_refusals_come_before_anything_is_allocated(monkeypatch):
    from easykv_amd import _lib, api, engine
    from easykv_amd._lib import EkvError
    loaded = []
    monkeypatch.setattr(_lib, "load", lambda: loaded.append(1))      # (the first thing a bank does before it allocates)
    for kw, match in ((dict(kv_quant="fp8"), "quantised"), (dict(kv_quant="k16_mxfp4"), "quantised"), (dict(long_rows=True), "long"),
                      (dict(logit_cap=50.0), "capped")):
        with pytest.raises(EkvError, match=match):
            engine.KVBank(2, 4, 2, 128, 256, windows=[4, 0], **kw)
    for d, sinks in ((64, None), (256, None), (128, torch.zeros(2, 4)), (96, torch.zeros(2, 4))):
        with pytest.raises(EkvError, match="head_dim"):
            engine.KVBank(2, 4, 2, d, 256, windows=[4, 0], **({} if sinks is None else dict(sinks=sinks)))
    for bad in ([4], [4, 0, 0], [[4, 0]], torch.zeros(2), torch.zeros(3, dtype=torch.int32), [4.0, 0], [True, 0], 4, "40"):
        with pytest.raises(ValueError, match="integers"):
            engine.KVBank(2, 4, 2, 128, 256, windows=bad)
    for bad in ([-1, 0], torch.tensor([0, -128])):
        with pytest.raises(ValueError, match=">= 0"):
            engine.KVBank(2, 4, 2, 128, 256, windows=bad)
    with pytest.raises(EkvError, match="batch"):
        engine.KVBankBatch(2, 2, 4, 2, 128, 256, windows=[4, 0])
    with pytest.raises(ValueError, match="streaming"):
        api.BudgetedKVCache(2, 4, 2, 128, 256, "cpu", streaming=True, windows=[4, 0])
    assert loaded == []
    # a window bank refuses quantize*(), set_rope() and compact_inplace() (a bank object without storage: the refusals read nothing else)
    b = engine.KVBank.__new__(engine.KVBank)
    b.windows, b.sinks, b.logit_cap, b.long_rows, b._fmt, b.head_dim, b.n_q_heads, b.n_kv_heads = (4, 0), None, None, False, None, 128, 4, 2
    for name in ("quantize_fp8", "quantize_mxfp4", "quantize_mxfp6", "quantize_fp8_mxfp4", "quantize_k16_mxfp4"):
        with pytest.raises(EkvError, match="windows"):
            getattr(b, name)()
    with pytest.raises(EkvError, match="window"):
        b.set_rope(torch.zeros(4, 128), torch.zeros(4, 128))
    with pytest.raises(EkvError, match="rows do not move"):
        b.compact_inplace(torch.zeros(2, 2, 1, dtype=torch.int32))
    assert b.resident_rows(engine.StepPlan(policy="roco", phase="decode")) == 0
    # ... and a step during a hipGraph capture: q_pos0 is a host scalar the graph would freeze
    b._tokens, b._win = [0, 0], _lib.Win()
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
    b._set_q_pos(0, 2, None)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(EkvError, match="captured graph would freeze"):
        b._set_q_pos(0, 2, None)
    monkeypatch.undo()
    monkeypatch.setattr(_lib, "load", lambda: loaded.append(1))
    # a bank without windows: the new keywords raise, nothing else changed
    b.windows = None
    with pytest.raises(EkvError, match="without windows"):
        b.ordered_tok_pos()
    with pytest.raises(EkvError, match="without windows"):
        b.load_rows(torch.zeros(2, 2, 3, 128), torch.zeros(2, 2, 3, 128), tok_pos=torch.zeros(2, 2, 3))


def test_the_reference_helper():
    from oracle import easykv_oracle as O
    from tests import sink_ref, window_ref
    g = torch.Generator().manual_seed(3)
    Hq, H, T, D = 4, 2, 9, 16
    q, k, v = torch.randn(1, Hq, 1, D, generator=g), torch.randn(1, H, T, D, generator=g), torch.randn(1, H, T, D, generator=g)
    sinks = torch.randn(Hq, generator=g)
    # W = 0: the oracle's own function, or the sink core's results
    assert window_ref.make_core(0) is O.attention_core
    with window_ref.patched(0):
        assert O.attention_core is window_ref.make_core(0)
    a, b = window_ref.make_core(0, sinks=sinks)(q, k, v), sink_ref.make_core(sinks)(q, k, v)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    # per head: head 0 keeps positions 0..8, head 1 has lost 3 old ones; query at 8, W = 4
    key_pos = torch.tensor([[0, 1, 2, 3, 4, 5, 6, 7, 8], [0, 1, 2, 3, 4, 8, 9, 10, 11]])
    for sk in (None, sinks):
        o, p = window_ref.make_core(4, key_pos, [11], sk)(q, k, v)
        assert bool((p[0, :2, 0, :8] == 0).all()) and bool((p[0, :2, 0, 8] > 0).all())      # head 0: only position 8 is within 4 of 11
        assert bool((p[0, 2:, 0, :5] == 0).all()) and bool((p[0, 2:, 0, 5:] > 0).all())      # head 1: positions 8..11
        # ... and equals the plain / sink attention over the attended keys alone
        for h, keep in ((0, slice(8, 9)), (1, slice(5, 9))):
            ref = sink_ref.make_core(None if sk is None else sk[2 * h:2 * h + 2])(q[:, 2 * h:2 * h + 2], k[:, h:h + 1, keep], v[:, h:h + 1, keep])
            assert torch.allclose(o[:, 2 * h:2 * h + 2], ref[0], atol=1e-6) and torch.allclose(p[:, 2 * h:2 * h + 2, :, keep], ref[1], atol=1e-6)
    track = [0.0]
    window_ref.make_core(4, key_pos, [11], None, track)(q, k, v)
    assert track[0] > 0
    pos = [[0, 1, 2, 3], [5, 6, 7, 8]]
    window_ref.drop_positions(pos, torch.tensor([[1], [3]]))
    assert pos == [[0, 2, 3], [5, 6, 7]]


# ---- the seeded cases of the GPU test leave the oracle's decisions well defined -----------------------------------------------------------
def _decode_cases():
    from tests.test_hip_window import DECODE_CASES
    return DECODE_CASES


def _chunk_cases():
    from tests.test_hip_window import CHUNK_CASES
    return CHUNK_CASES


@pytest.mark.parametrize("case", _chunk_cases(), ids=[c[0] for c in _chunk_cases()])
def test_chunk_cases_stay_inside_the_decision_cap_on_the_oracle_alone(case):
    from tests.test_hip_window import run_chunk_case
    n_checked, n_total, dist = run_chunk_case(*case, oracle_only=True)
    assert n_checked >= 10 and 2 * n_checked >= n_total and dist >= 1e-2, (case[0], n_checked, n_total, dist)


@pytest.mark.parametrize("case", _decode_cases(), ids=[c[0] for c in _decode_cases()])
def test_decode_cases_stay_inside_the_decision_cap_on_the_oracle_alone(case):
    """The decision cap is a condition, not a measurement: each oracle-compared case of tests/test_hip_window.py, run on the reference
    alone, compares at least 10 decisions and at least half of all (run_decode_case asserts _enough), and its windowed attention is at
    least 1e-2 away from the full one."""
    from tests.test_hip_window import run_decode_case
    n_checked, n_total, dist = run_decode_case(*case, oracle_only=True)
    assert n_checked >= 10 and 2 * n_checked >= n_total and dist >= 1e-2, (case[0], n_checked, n_total, dist)


def _driver_cases():
    from tests.test_hip_window import DRIVER_CASES
    return DRIVER_CASES


@pytest.mark.parametrize("case", _driver_cases(), ids=[f"{c[0]}-{c[2]}" for c in _driver_cases()])
def test_driver_cases_stay_inside_the_decision_cap_on_the_oracle_alone(case):
    from tests.test_hip_window import run_driver_case
    n_checked, n_total, dist = run_driver_case(*case, oracle_only=True)
    assert n_checked >= 10 and 2 * n_checked >= n_total and dist >= 1e-2, (case, n_checked, n_total, dist)


# ---- the driver and the seam --------------------------------------------------------------------------------------------------------------
def test_driver_reads_the_windows_and_hands_them_to_the_cache(monkeypatch):
    import contextlib
    import io
    from easykv_amd import api
    import tests.test_driver_cpu as TD
    from tests.test_sink_cpu import _model
    seen = []

    class Cache(TD.StubCache):
        def __init__(self, *a, windows=None, sinks=None, **k):
            seen.append((windows, sinks))
            self.windows, self.sinks = windows, sinks
            super().__init__(*a, **k)
    monkeypatch.setattr(api, "BudgetedKVCache", Cache)
    ids = torch.arange(40).view(1, -1) % 16
    gen = dict(budget=16, kv_policy="roco", max_new_tokens=4)
    sinks = torch.zeros(2, 4)
    for model, cfg, want in ((_model(d=128), dict(gen, sliding_window=[8, 0]), [8, 0]),
                             (_model(d=128, sliding_window=32, layer_types=["full_attention", "sliding_attention"]), dict(gen, sliding_window="model"), [0, 32]),
                             (_model(d=128, sliding_window=32), dict(gen, sliding_window="model"), [32, 32]),
                             (_model(d=64, sinks=sinks, sliding_window=128, layer_types=["sliding_attention", "full_attention"]), dict(gen, sliding_window="model"), [128, 0]),
                             (_model(d=128), dict(gen, sliding_window=torch.tensor([0, 0])), [0, 0])):
        seen.clear()
        with contextlib.redirect_stdout(io.StringIO()):
            api.generate(model, ids, cfg, kv_mode="decoding", stride=1)
        assert len(seen) == 1 and seen[0][0] == want, seen
    # absent or None: today's behaviour — the stub of tests/test_driver_cpu.py takes no such keyword, and a model's own window is ignored
    monkeypatch.setattr(api, "BudgetedKVCache", TD.StubCache)
    for cfg in (gen, dict(gen, sliding_window=None)):
        with contextlib.redirect_stdout(io.StringIO()):
            api.generate(_model(d=128, sliding_window=32), ids, cfg, kv_mode="decoding", stride=1)
    assert api._collect_windows(_model(sliding_window=32), {}, 2) is None
    for bad in ("yes", [8], [8, -1], [8.0, 0], 8, [[8, 0]]):
        with pytest.raises(ValueError, match="sliding_window"):
            api.generate(_model(d=128), ids, dict(gen, sliding_window=bad), kv_mode="decoding", stride=1)
    with pytest.raises(ValueError, match="config.sliding_window"):
        api.generate(_model(d=128), ids, dict(gen, sliding_window="model"), kv_mode="decoding", stride=1)
    with pytest.raises(ValueError, match="layer_types"):
        api.generate(_model(d=128, sliding_window=8, layer_types=["sliding_attention"]), ids, dict(gen, sliding_window="model"), kv_mode="decoding", stride=1)


def test_driver_refusals_of_a_window_run_come_before_any_bank(monkeypatch):
    from types import SimpleNamespace
    from easykv_amd import api, engine
    from tests.test_sink_cpu import _model
    made = []
    monkeypatch.setattr(engine.KVBank, "__init__", lambda self, *a, **k: made.append(1))
    ids = torch.arange(40).view(1, -1) % 16
    gen = dict(budget=16, kv_policy="roco", max_new_tokens=4, sliding_window=[8, 0])
    for extra, match in ((dict(streaming=True), "streaming"), (dict(kv_quant="fp8"), "kv_quant"), (dict(long_rows=True), "long_rows"),
                         (dict(hipgraph=True), "a captured graph would freeze")):
        with pytest.raises(ValueError, match=match):
            api.generate(_model(d=128), ids, dict(gen, **extra), kv_mode="decoding", stride=1)
    with pytest.raises(ValueError, match="attn_logit_softcapping"):
        api.generate(_model(d=128, attn_logit_softcapping=50.0), ids, gen, kv_mode="decoding", stride=1)
    with pytest.raises(ValueError, match="head_dim 128"):
        api.generate(_model(d=64), ids, gen, kv_mode="decoding", stride=1)
    with pytest.raises(ValueError, match="head_dim 64"):
        api.generate(_model(d=128, sinks=torch.zeros(2, 4)), ids, gen, kv_mode="decoding", stride=1)
    sharded = _model(d=128)
    sharded.layer_shard = SimpleNamespace(world=2, begin=0, count=1, end=1, n_layers=2, rank=0)
    with pytest.raises(ValueError, match="layer-sharded"):
        api.generate(sharded, ids, gen, kv_mode="decoding", stride=1)
    with pytest.raises(ValueError, match="sliding_window"):
        api.generate_batch(_model(d=128), [ids, ids], gen, kv_mode="decoding", stride=1)
    assert made == []


def test_the_seam_holds_the_modules_window_against_the_caches(monkeypatch):
    from types import SimpleNamespace
    from easykv_amd import api, hf
    calls = []

    def cache(windows, layer_begin=0):
        c = SimpleNamespace(sm_scale=None, logit_cap=None, sinks=None, windows=windows, streaming=False, layer_begin=layer_begin, _windows_checked=set())
        c.attend = lambda layer, q, k, v: calls.append(layer) or torch.zeros(1, 4, q.shape[2], 128)
        return c
    q = torch.zeros(1, 4, 3, 128)
    k = torch.zeros(1, 2, 3, 128)
    mod = [SimpleNamespace(layer_idx=i) for i in range(3)]
    c = cache((8, 0))
    monkeypatch.setattr(api, "active_cache", lambda: c)
    hf._easykv_attention(mod[0], q, k, k, sliding_window=8)
    hf._easykv_attention(mod[1], q, k, k, sliding_window=None)
    hf._easykv_attention(mod[1], q, k, k)
    assert c._windows_checked == {0, 1}
    hf._easykv_attention(mod[0], q, k, k, sliding_window=99)      # (once per (cache, layer): the decode loop gains no check)
    for layer, theirs in ((0, None), (0, 4), (0, 0), (1, 8)):
        c = cache((8, 0))
        with pytest.raises(ValueError, match="sliding window"):
            hf._easykv_attention(mod[layer], q, k, k, sliding_window=theirs)
    c = cache((8, 0))
    with pytest.raises(ValueError, match="outside"):
        hf._easykv_attention(mod[2], q, k, k, sliding_window=8)
    c = cache((0, 8), layer_begin=1)      # (a cache that owns layers 1 .. 2)
    hf._easykv_attention(mod[2], q, k, k, sliding_window=8)
    # without windows on the cache the module's window is ignored, as before
    c = cache(None)
    n = len(calls)
    hf._easykv_attention(mod[0], q, k, k, sliding_window=8)
    assert len(calls) == n + 1 and c._windows_checked == set()
