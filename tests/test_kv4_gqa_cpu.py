"""MXFP4 rows at GQA factors up to 16 ("kv4 gqa", include/easykv_hip.h) on a CPU: calls, dry runs, objects, driver routing, and the
precondition of the seeded cases of tests/test_hip_kv4_gqa.py (which draws them from here)."""
import ctypes
import os
import re

import pytest
import torch

from tests import kv4_cases as K
from tests import kv4_ref as R
from tests.test_dispatch_table import _case, _structs, cases
from tests.test_driver_cpu import api, _ids      # noqa: F401  (the stub-cache fixture)
from tests.test_kv4_cpu import _lib, _model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F16, BF16 = 0, 1
BF, HF = torch.bfloat16, torch.float16

# The GPU table, in the tuple of tests/kv4_cases.py (T = budget + 1).  rep 5 / 8 / 12 / 16: padded columns, half-full groupings, the full
# tile.  T 5 / 17 / 64 / 257: a partial tile, a one-row tail tile, whole tiles, a tail after many; T 257 in splits of 128 positions leaves
# the last split no live row, T 301 gives three splits with live rows.  Three steps: an evicted slot is reused by the next append.
CASES = [
    ("rep5 T5 full", 2, 10, 2, HF, 4, "full", 1, False, False, None, 3),
    ("rep8 T17 h2o bf16", 2, 16, 2, BF, 16, "h2o_head", 1, False, False, None, 3),
    ("rep12 T64 roco deferred", 2, 24, 2, HF, 63, "roco", 1, True, False, None, 3),
    ("rep16 T257 h2o bf16 split, empty last split", 2, 32, 2, BF, 256, "h2o_head", 3, False, False, None, 3),
    ("rep8 T257 roco split deferred", 2, 16, 2, HF, 256, "roco", 3, True, False, None, 3),
    ("rep16 T301 roco split, exponents 14 / -20", 2, 32, 2, HF, 300, "roco", 3, False, False, None, 3),
    ("rep8 T4097 full unsplit, 54 KB of LDS", 2, 16, 2, HF, 4096, "full", 1, False, False, None, 3),      # (above the 48 KB default of a launch)
]


_kv4_inputs = K.inputs


def inputs(case):
    """tests.kv4_cases.inputs; the 'exponents' case gets a V block at exponent 14 (6 * 2^14 is not finite in fp16) and a K block at -20."""
    k0, v0, warm, per_step = _kv4_inputs(case)
    if "exponents" in case[0]:
        v0[0, 0, 3, 32:64] *= 100.0
        v0[0, 0, 3, 40] = 60000.0
        k0[0, 1, 5, 64:96] = (k0[0, 1, 5, 64:96].float() * 2.0 ** -20).to(k0.dtype)
        _, ev = R.quantize(v0[0, 0, 3].float().view(1, -1))
        _, ek = R.quantize(k0[0, 1, 5].float().view(1, -1))
        assert int(ev[0, 1]) == 127 + 14 and int(ek[0, 2]) <= 127 - 20
    return k0, v0, warm, per_step


def _answers(lib, prefix, bank, st, dtype, kv4):
    b, s = ctypes.byref(bank), ctypes.byref(st)
    info = (ctypes.c_int32 * 10)(*([-7] * 10))
    if kv4 is None:
        return [lib.ekv_step_check_typed(b, s, dtype), lib.ekv_step_info_typed(b, s, dtype, info, 10)] + list(info) + [lib.ekv_workspace_bytes_typed(b, s, dtype)]
    f = lambda what: getattr(lib, prefix + what)
    k = ctypes.byref(kv4)
    return [f("step_check")(b, s, dtype, k), f("step_info")(b, s, dtype, k, info, 10)] + list(info) + [f("workspace_bytes")(b, s, dtype, k)]


EXTRA = [dict(hq=40, h=8), dict(hq=64, h=8), dict(hq=96, h=8), dict(hq=128, h=8), dict(hq=64, h=8, policy=0, n_evict=0),
         dict(hq=64, h=8, phases=1 | 4, layer_count=1, defer_layers=32), dict(hq=128, h=8, phases=8, defer_layers=32), dict(hq=48, h=8, n_split=1),
         # refused: GQA x 17, a chunk step, RoPE-on-read, other head dims, slot-indexed score rows
         dict(hq=136, h=8), dict(hq=64, h=8, q_len=8, n_slots=2056, n_evict=8, roco_k1=1800, count_add2=16), dict(hq=64, h=8, rope_on_read=1),
         dict(hq=64, h=8, head_dim=64), dict(hq=40, h=8, head_dim=96), dict(hq=64, h=8, phases=16, phys_extent=2112)]


def test_dry_runs_are_the_kv4_call_or_the_16_bit_split_plan():
    L, lib = _lib()
    declared = set(re.findall(r"\b(ekv_[a-z0-9_]+)\s*\(", open(os.path.join(ROOT, "include", "easykv_hip.h")).read()))
    for what in L.STEP_CALLS:      # the four calls: declared, exported, bound
        name = L.KV4_GQA_CALLS[what]
        assert name == "ekv_kv4_gqa_" + what and name in declared and name in L.EXPORTS and hasattr(ctypes.CDLL(L.LIB), name) and hasattr(lib, name), name
    assert lib.ekv_kv4_gqa_step_check(None, None, F16, None) == -1 and lib.ekv_kv4_gqa_workspace_bytes(None, None, F16, None) == 0
    kv4 = L.Kv4(256, 256, 256, 256)
    n_same = n_mfma = n_fold = n_refused = 0
    for c in cases() + [_case(n_layers=32, **kw) for kw in EXTRA]:
        bank, st = _structs(c)
        rep = c["hq"] // c["h"]
        for dt in (F16, BF16):
            got = _answers(lib, "ekv_kv4_gqa_", bank, st, dt, kv4)
            if rep <= 4:      # IS the kv4 call: code, info, workspace
                assert got == _answers(lib, "ekv_kv4_", bank, st, dt, kv4), (c, got)
                n_same += 1
                continue
            _, st2 = _structs(c)
            if st2.phases & ~48 == 0:
                st2.phases |= 1 | 2      # the whole-step form plans as attention + scorer
            ref = _answers(lib, None, bank, st2, dt, None)
            takes = c["q_len"] == 1 and not c["rope_on_read"] and c["head_dim"] == 128 and rep <= 16
            if ref[0] == -1:
                assert got[0] == -1, (c, got)
            elif ref[0] == 0 and takes:      # the 16-bit split plan in every field: splits, launches, in-kernel fold, workspace
                assert got == ref and got[3] == 0 and got[10] >= 1, (c, got, ref)
                n_mfma += 1
                n_fold += got[10] == 1
            else:
                assert got[0] == -2 and got[-1] == 0 and (got[1] != 0 or (got[3] == 0 and got[10] == 0)), (c, got, ref)      # nothing planned, no bytes
                n_refused += 1
    assert n_same > 50 and n_mfma >= 12 and n_fold >= 1 and n_refused >= 10, (n_same, n_mfma, n_fold, n_refused)
    # missing planes are argument errors at every factor; the plain kv4 refusals are what they were
    bank, st = _structs(_case(n_layers=32, hq=64, h=8))
    for i in range(4):
        planes = [256] * 4
        planes[i] = None
        assert lib.ekv_kv4_gqa_step_check(ctypes.byref(bank), ctypes.byref(st), F16, ctypes.byref(L.Kv4(*planes))) == -1
    assert lib.ekv_kv4_step_check(ctypes.byref(bank), ctypes.byref(st), F16, ctypes.byref(kv4)) == -2
    # a split's key range is bounded by the kernel's LDS (31 360 positions): the plan takes the fewest splits that fit, whatever was asked
    for T, asked, want in ((31360, 1, 1), (31361, 1, 2), (100000, 2, 4), (100000, 8, 8)):
        c = _case(n_layers=32, hq=64, h=8, policy=0, n_evict=0, n_slots=T, cap=(T + 127) // 64 * 64, n_split=asked)
        bank, st = _structs(c)
        got = _answers(lib, "ekv_kv4_gqa_", bank, st, F16, kv4)
        st.phases = 1 | 2
        ref = _answers(lib, None, bank, st, F16, None)
        assert ref[:3] == [0, 0, asked] and got[:3] == [0, 0, want] and got[10] >= 1 and (got == ref) == (want == asked), (T, got, ref)


def test_the_two_objects_are_built_beside_the_pinned_lists():
    import subprocess
    from easykv_amd import _build
    want = ["ekv_attn_decode_mxg_d128", "ekv_attn_decode_mxg_d128_bf16"]
    later = [n for n, _ in _build.later_objects()]
    pinned = [n for n, _ in _build.objects() + _build.added_objects()]
    assert [n for n in later if "mxg" in n] == want and not any("mxg" in n for n in pinned)
    assert ("EKV_DECODE_MXG", ("f16", "128")) in _build.later_instances() and "EKV_DECODE_MXG" in _build.FAMILIES
    assert "ekv_attn_decode_mxg.hip" in _build.LATER_SOURCES and all("mxg" not in os.path.basename(s) for s in _build.sources())
    _build.build_lib()
    for n in want + ["ekv_attn_decode_mxg"]:
        assert os.path.exists(os.path.join(_build.OBJ, n + ".o")), n
    syms = subprocess.run(["nm", "-D", "--defined-only", _build.LIB], capture_output=True, text=True).stdout
    assert "ekv_launch_attn_decode_mxg_d128_f16" in syms and "ekv_launch_attn_decode_mxg_d128_bf16" in syms


def test_generate_routes_by_the_grouped_key_and_refuses_before_a_cache(api, monkeypatch):
    import contextlib
    import io
    from types import SimpleNamespace
    from tests import test_driver_cpu as T
    events = []

    class Bank(T.StubBank):
        def quantize(self, kind):
            events.append(("plain", kind))
            self.kv_quant = kind

        def quantize_mxfp4(self, grouped=False):
            events.append(("mxfp4", grouped, self.n_slots[0]))
            self.kv_quant = "mxfp4"
    monkeypatch.setattr(T, "StubBank", Bank)
    gen = dict(kv_policy="roco", budget=8, max_new_tokens=4, eos_token_ids=[-1], kv_quant="mxfp4")
    ids = _ids(16)
    with contextlib.redirect_stdout(io.StringIO()):      # GQA x 8
        text, cache = api.generate(_model(hq=16, h=2), ids, dict(gen, kv_quant_grouped=True), kv_mode="decoding", return_cache=True)
    assert len(text.split()) == 4 and cache.bank.kv_quant == "mxfp4"
    assert len(events) == 1 and events[0][:2] == ("mxfp4", True), events      # one conversion, at the boundary, through the grouped argument
    del events[:]
    with contextlib.redirect_stdout(io.StringIO()):
        api.generate(_model(), ids, gen, kv_mode="decoding")
    assert events == [("plain", "mxfp4")]      # without the key: the conversion it always was
    T.StubCache.made = 0
    big, m8 = _model(hq=34, h=2), _model(hq=16, h=2)
    both = "kv_quant_grouped"
    for m, extra, mode, match in (
            (m8, dict(kv_quant_grouped=True, kv_quant="fp8"), "decoding", "kv_quant_grouped'] = True needs generation_config\\['kv_quant'] = 'mxfp4'"),
            (m8, dict(kv_quant_grouped=1.5), "decoding", "must be False or True"),
            (m8, dict(kv_quant_grouped=True, streaming=True), "decoding", both + ".*streaming"),
            (m8, dict(kv_quant_grouped=True), "ppl", both + ".*ppl"),
            (m8, dict(kv_quant_grouped=True, long_rows=True), "decoding", "long_rows.*" + both),
            (m8, dict(kv_quant_grouped=True, sliding_window=[4, 0]), "decoding", "sliding_window.*" + both),
            (_model(hq=16, h=2, d=64), dict(kv_quant_grouped=True), "decoding", both + ".*needs head_dim 128"),
            (big, dict(kv_quant_grouped=True), "decoding", both + ".*GQA factor of at most 16"),
            (m8, dict(), "decoding", "GQA factor of at most 4")):      # the plain key's refusal is unchanged
        with pytest.raises(ValueError, match=match):
            api.generate(m, ids, dict(gen, **extra), kv_mode=mode)
    with pytest.raises(ValueError, match="generate_batch.*kv_quant_grouped"):
        api.generate_batch(m8, [ids, _ids(20)], dict(gen, kv_quant_grouped=True), kv_mode="decoding")
    capped = _model(hq=16, h=2)
    capped.config.attn_logit_softcapping = 30.0
    with pytest.raises(ValueError, match="attn_logit_softcapping.*" + both):
        api.generate(capped, ids, dict(gen, kv_quant_grouped=True), kv_mode="decoding")
    with pytest.raises(ValueError, match="sinks.*" + both):
        api.generate(m8, ids, dict(gen, kv_quant_grouped=True, attention_sinks=torch.zeros(2, 16)), kv_mode="decoding")
    m8.layer_shard = SimpleNamespace(world=2, rank=0, begin=0, count=1)
    with pytest.raises(ValueError, match=both + ".*layer-sharded"):
        api.generate(m8, ids, dict(gen, kv_quant_grouped=True), kv_mode="decoding")
    assert T.StubCache.made == T.StubCacheBatch.made == 0


@pytest.mark.parametrize("case", [c for c in CASES if c[6] in K.SCORED], ids=[c[0] for c in CASES if c[6] in K.SCORED])
def test_scored_cases_have_well_defined_decisions(case, monkeypatch):
    """The oracle alone over the case's seeded inputs as tests/kv4_ref.py quantises them: at least 90 % of the decisions are well defined
    under tests.test_hip_fullsize.Probe — the body and the cap of tests/test_kv4_cpu.py's precondition, over this file's inputs."""
    from tests.test_kv4_cpu import test_scored_cases_have_well_defined_decisions as precondition
    monkeypatch.setattr(K, "inputs", inputs)
    precondition(case)
