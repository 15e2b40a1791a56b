"""FP8 rows at GQA factors up to 16 on the MFMA decode kernel ("kv8 gqa", include/easykv_hip.h) on a CPU: calls, dry runs, objects, driver
routing, and the precondition of the seeded cases of tests/test_hip_kv8_gqa.py (which draws them from here)."""
import ctypes
import os
import re

import pytest
import torch

from tests import kv4_cases as K
from tests import kv8_ref as R
from tests.test_dispatch_table import _case, _structs, cases
from tests.test_driver_cpu import api, _ids      # noqa: F401  (the stub-cache fixture)
from tests.test_kv4_cpu import _lib, _model
from tests.test_kv4_gqa_cpu import EXTRA as _KV4_EXTRA, _answers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F16, BF16, BF, HF = 0, 1, torch.bfloat16, torch.float16

# The GPU table, in the tuple of tests/kv4_cases.py with the head_dim in the `expect` field (T = budget + 1): a partial tile, one-row
# tail tiles, whole tiles, padded columns, an odd factor, the full tile; three steps, so an evicted slot is reused by the next append.
CASES = [
    ("rep5 T5 full d128", 2, 10, 2, HF, 4, "full", 1, False, False, 128, 3),
    ("rep8 T17 h2o d128 bf16", 2, 16, 2, BF, 16, "h2o_head", 1, False, False, 128, 3),
    ("rep7 T33 tova d64 bf16", 2, 14, 2, BF, 32, "tova", 1, False, False, 64, 3),
    ("rep12 T64 roco d64 deferred", 2, 24, 2, HF, 63, "roco", 1, True, False, 64, 3),
    ("rep16 T257 h2o d64 bf16 split, last split the appended row alone", 2, 32, 2, BF, 256, "h2o_head", 3, False, False, 64, 3),
    ("rep8 T257 roco d128 split deferred", 2, 16, 2, HF, 256, "roco", 3, True, False, 128, 3),
    ("rep16 T301 roco d128 split, scales 134 / 2^-20", 2, 32, 2, HF, 300, "roco", 3, False, False, 128, 3),
    ("rep8 T4097 full d128 unsplit, 54 KB of LDS", 2, 16, 2, HF, 4096, "full", 1, False, False, 128, 3),      # (above the 48 KB default of a launch)
]


def inputs(case):
    """The input scheme of tests.kv4_cases.inputs (its seed, its order of draws) at the case's head_dim; the 'scales' case gets a V row
    that holds 60000 (scale ~ 134, the row's other codes at most a few subnormal steps) and a K row scaled by 2^-20."""
    name, L, hq, h, dtype, budget, policy, n_split, defer, slot, D, steps = case
    g, vs = torch.Generator().manual_seed(K.SEED), K.v_scale(dtype)
    k0 = torch.randn(L, h, budget, D, generator=g).to(dtype)
    v0 = (torch.randn(L, h, budget, D, generator=g) * vs).to(dtype)
    warm = torch.rand(L, h, budget, generator=g) * 1e-3 if policy in K.SCORED else None
    if "scales" in name:
        v0[0, 0, 3, 40] = 60000.0
        k0[0, 1, 5] = (k0[0, 1, 5].float() * 2.0 ** -20).to(dtype)
        assert 133 < float(R.quantize(v0[0, 0, 3])[1]) < 135 and float(R.quantize(k0[0, 1, 5])[1]) < 2.0 ** -20
    draw = lambda n, s=1.0: (torch.randn(L, n, 1, D, generator=g) * s).to(dtype)
    return k0, v0, warm, ((draw(hq), draw(h), draw(h, vs), -1) for _ in range(steps))


GQA = [kw for kw in _KV4_EXTRA if "head_dim" not in kw]      # GQA x 5 .. 16 forms, and refused: x 17, a chunk step, RoPE-on-read, slot rows
EXTRA = [dict(kw, head_dim=d) for kw in GQA for d in (64, 128)] + [dict(hq=40, h=8, head_dim=96), dict(hq=64, h=8, head_dim=256)]      # (other head dims: refused)


def test_dry_runs_are_the_kv8_call_or_the_16_bit_split_plan():
    L, lib = _lib()
    declared = set(re.findall(r"\b(ekv_[a-z0-9_]+)\s*\(", open(os.path.join(ROOT, "include", "easykv_hip.h")).read()))
    for what in L.STEP_CALLS:      # the four calls: declared, exported, bound
        name = L.KV8_GQA_CALLS[what]
        assert name == "ekv_kv8_gqa_" + what and name in declared and name in L.EXPORTS and hasattr(ctypes.CDLL(L.LIB), name) and hasattr(lib, name), name
    assert lib.ekv_kv8_gqa_step_check(None, None, F16, None) == -1 and lib.ekv_kv8_gqa_workspace_bytes(None, None, F16, None) == 0
    kv8 = L.Kv8(256, 256, 256, 256)
    n_same = n_mfma = n_fold = n_refused = 0
    for c in cases() + [_case(n_layers=32, **kw) for kw in EXTRA]:
        bank, st = _structs(c)
        rep = c["hq"] // c["h"]
        for dt in (F16, BF16):
            got = _answers(lib, "ekv_kv8_gqa_", bank, st, dt, kv8)
            plain = _answers(lib, "ekv_kv8_", bank, st, dt, kv8)
            if rep <= 4:      # IS the kv8 call: code, info, workspace
                assert got == plain, (c, got)
                n_same += 1
                continue
            _, st2 = _structs(c)
            if st2.phases & ~48 == 0:
                st2.phases |= 1 | 2      # the whole-step form plans as attention + scorer
            ref = _answers(lib, None, bank, st2, dt, None)
            takes = c["q_len"] == 1 and not c["rope_on_read"] and c["head_dim"] in (64, 128) and rep <= 16
            if ref[0] == -1:
                assert got[0] == -1, (c, got)
            elif ref[0] == 0 and takes:      # the 16-bit split plan in every field: splits, launches, in-kernel fold, workspace
                assert got == ref and got[3] == 0 and got[10] >= 1, (c, got, ref)
                n_mfma += 1
                n_fold += got[10] == 1
            else:
                assert got[0] == -2 and got[-1] == 0 and (got[1] != 0 or (got[3] == 0 and got[10] == 0)), (c, got, ref)      # nothing planned, no bytes
                n_refused += 1
    assert n_same > 50 and n_mfma >= 24 and n_fold >= 2 and n_refused >= 12, (n_same, n_mfma, n_fold, n_refused)
    # missing planes are argument errors at every factor; the plain kv8 call answers GQA x 8 as it did (on its own plan)
    for hq in (16, 64):
        bank, st = _structs(_case(n_layers=32, hq=hq, h=8))
        for i in range(4):
            planes = [256] * 4
            planes[i] = None
            assert lib.ekv_kv8_gqa_step_check(ctypes.byref(bank), ctypes.byref(st), F16, ctypes.byref(L.Kv8(*planes))) == -1
    assert lib.ekv_kv8_step_check(ctypes.byref(bank), ctypes.byref(st), F16, ctypes.byref(kv8)) == 0
    # a split's key range is bounded by the kernel's LDS (31 360 positions at head_dim 128, 35 456 at 64): the fewest splits that fit
    for d, T, asked, want in ((128, 31360, 1, 1), (128, 31361, 1, 2), (64, 35456, 1, 1), (64, 35457, 1, 2), (128, 100000, 2, 4), (64, 100000, 2, 3), (128, 100000, 8, 8)):
        c = _case(n_layers=32, hq=64, h=8, head_dim=d, policy=0, n_evict=0, n_slots=T, cap=(T + 127) // 64 * 64, n_split=asked)
        bank, st = _structs(c)
        got = _answers(lib, "ekv_kv8_gqa_", bank, st, F16, kv8)
        st.phases = 1 | 2
        ref = _answers(lib, None, bank, st, F16, None)
        assert ref[:3] == [0, 0, asked] and got[:3] == [0, 0, want] and got[10] >= 1 and (got == ref) == (want == asked), (d, T, got, ref)


def test_the_four_objects_are_built_beside_the_pinned_lists():
    import subprocess
    from easykv_amd import _build
    want = ["ekv_attn_decode_g8_d64", "ekv_attn_decode_g8_d64_bf16", "ekv_attn_decode_g8_d128", "ekv_attn_decode_g8_d128_bf16"]
    later = [n for n, _ in _build.later_objects()]
    pinned = [n for n, _ in _build.objects() + _build.added_objects()]
    assert [n for n in later if "_g8_" in n] == want and not any("_g8_" in n for n in pinned) and len(set(later)) == len(later)
    assert ("EKV_DECODE_G8", ("bf16", "64")) in _build.later_instances() and "EKV_DECODE_G8" in _build.FAMILIES and "ekv_attn_decode_g8.hip" in _build.LATER_SOURCES
    _build.build_lib()
    for n in want + ["ekv_attn_decode_g8"]:
        assert os.path.exists(os.path.join(_build.OBJ, n + ".o")), n
    syms = subprocess.run(["nm", "-D", "--defined-only", _build.LIB], capture_output=True, text=True).stdout
    assert all(f"ekv_launch_attn_decode_g8_d{d}_{e}" in syms for d in (64, 128) for e in ("f16", "bf16"))


def test_generate_routes_by_the_gqa_key_and_refuses_before_a_cache(api, monkeypatch):
    import contextlib
    import io
    from types import SimpleNamespace
    from tests import test_driver_cpu as T
    events = []

    class Bank(T.StubBank):
        def quantize(self, kind):
            events.append(("plain", kind))
            self.kv_quant = kind

        def quantize_fp8(self, chunks=False, grouped=False):
            events.append(("fp8", chunks, grouped, self.n_slots[0]))
            self.kv_quant = "fp8"
    monkeypatch.setattr(T, "StubBank", Bank)
    gen = dict(kv_policy="roco", budget=8, max_new_tokens=4, eos_token_ids=[-1], kv_quant="fp8")
    ids = _ids(16)
    with contextlib.redirect_stdout(io.StringIO()):      # GQA x 8
        text, cache = api.generate(_model(hq=16, h=2), ids, dict(gen, kv_quant_gqa=True), kv_mode="decoding", return_cache=True)
    assert len(text.split()) == 4 and cache.bank.kv_quant == "fp8"
    assert len(events) == 1 and events[0][:3] == ("fp8", False, True), events      # one conversion, at the boundary, through the grouped argument
    del events[:]
    with contextlib.redirect_stdout(io.StringIO()):
        api.generate(_model(hq=16, h=2), ids, gen, kv_mode="decoding")
    assert events == [("plain", "fp8")]      # without the key: the conversion it always was, at any factor
    T.StubCache.made = 0
    big, m8 = _model(hq=34, h=2), _model(hq=16, h=2)
    both = "kv_quant'] = 'fp8' with generation_config\\['kv_quant_gqa"
    for m, extra, mode, match in (
            (m8, dict(kv_quant_gqa=True, kv_quant="mxfp4"), "decoding", "kv_quant_gqa'] = True needs generation_config\\['kv_quant'] = 'fp8'"),
            (m8, dict(kv_quant_gqa=1.5), "decoding", "kv_quant_gqa'] must be False or True"),
            (m8, dict(kv_quant_gqa=True, kv_quant_prefill=True), "decoding", "kv_quant_gqa.*'fp8'.*kv_quant_prefill"),
            (m8, dict(kv_quant_gqa=True, streaming=True), "decoding", both + ".*streaming"),
            (m8, dict(kv_quant_gqa=True), "ppl", both + ".*ppl"),
            (m8, dict(kv_quant_gqa=True, long_rows=True), "decoding", "long_rows.*" + both),
            (m8, dict(kv_quant_gqa=True, sliding_window=[4, 0]), "decoding", "sliding_window.*" + both),
            (_model(hq=16, h=2, d=96), dict(kv_quant_gqa=True), "decoding", both + ".*needs head_dim 64 or 128"),
            (big, dict(kv_quant_gqa=True), "decoding", both + ".*GQA factor of at most 16")):
        with pytest.raises(ValueError, match=match):
            api.generate(m, ids, dict(gen, **extra), kv_mode=mode)
    with pytest.raises(ValueError, match="generate_batch.*kv_quant_gqa.*'fp8'"):
        api.generate_batch(m8, [ids, _ids(20)], dict(gen, kv_quant_gqa=True), kv_mode="decoding")
    capped = _model(hq=16, h=2)
    capped.config.attn_logit_softcapping = 30.0
    with pytest.raises(ValueError, match="attn_logit_softcapping.*" + both):
        api.generate(capped, ids, dict(gen, kv_quant_gqa=True), kv_mode="decoding")
    with pytest.raises(ValueError, match="sinks.*" + both):
        api.generate(m8, ids, dict(gen, kv_quant_gqa=True, attention_sinks=torch.zeros(2, 16)), kv_mode="decoding")
    m8.layer_shard = SimpleNamespace(world=2, rank=0, begin=0, count=1)
    with pytest.raises(ValueError, match=both + ".*layer-sharded"):
        api.generate(m8, ids, dict(gen, kv_quant_gqa=True), kv_mode="decoding")
    assert T.StubCache.made == T.StubCacheBatch.made == 0


@pytest.mark.parametrize("case", [c for c in CASES if c[6] in K.SCORED], ids=[c[0] for c in CASES if c[6] in K.SCORED])
def test_scored_cases_have_well_defined_decisions(case):
    """The oracle alone over the case's seeded inputs as tests/kv8_ref.py quantises them: at least 90 % of the decisions are well defined
    under tests.test_hip_fullsize.Probe (the cap tests/test_hip_kv8_gqa.py asserts on the GPU; the scheme of tests/test_kv4_cpu.py's)."""
    from oracle import easykv_oracle as O
    from tests.test_hip_fullsize import Probe
    name, L, hq, h, dtype, budget, policy, *_ = case
    k0, v0, warm, per_step = inputs(case)
    deq = lambda x: R.dequant(*R.quantize(x)).unsqueeze(0)
    states = [O.LayerState(k=deq(k0[l]), v=deq(v0[l])) for l in range(L)]
    for l, st in enumerate(states):
        st.s, st.q, st.c = O.init_state_decoding((h,), budget)
        st.s[:, :budget] += warm[l]
        st.q[:, :budget] += warm[l] ** 2
    O.SELECT_HOOK = probe = Probe()
    n_dec = n_stable = 0
    try:
        for q, k, v, rs in per_step:
            for l in range(L):
                O.layer_step(states[l], q[l:l + 1].float(), deq(k[l]), deq(v[l]), O.StepPlan(range_start=rs, **K.plan_kw(case)))
                n_dec += h
                n_stable += int((~probe.last_unstable).sum())
    finally:
        O.SELECT_HOOK = None
    assert n_stable >= 0.9 * n_dec, (name, n_stable, n_dec)
