"""FP8 K/V storage ("kv8", include/easykv_hip.h) on a CPU: the six calls exist, their dry runs answer as the 16-bit step of the same
shape wherever a kv8 bank takes the step and refuse everything else before a launch, and the reference rule (tests/kv8_ref.py) has
the properties the GPU quantiser is held to.  Dummy non-null pointers throughout: nothing is dereferenced, nothing is launched."""
import ctypes
import os
import re

import numpy as np
import torch

from tests import kv8_ref as R
from tests.test_dispatch_table import _case, _structs, cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("ekv_kv8_quantize", "ekv_kv8_dequantize", "ekv_kv8_step_check", "ekv_kv8_step_info", "ekv_kv8_workspace_bytes",
         "ekv_kv8_step_attend")
F16, BF16 = 0, 1


def _lib():
    from easykv_amd import _build, _lib as L
    if not os.path.exists(_build.LIB):
        _build.build_lib()
    return L, L.load()


def test_kv8_calls_are_exported_and_declared():
    L, lib = _lib()
    header = open(os.path.join(ROOT, "include", "easykv_hip.h")).read()
    declared = set(re.findall(r"\b(ekv_[a-z0-9_]+)\s*\(", header))
    raw = ctypes.CDLL(L.LIB)
    for name in CALLS:
        assert name in declared and name in L.EXPORTS and hasattr(raw, name) and hasattr(lib, name), name
    assert lib.ekv_abi_version() == 8
    assert "typedef struct ekv_kv8 {" in header and "e4m3fn" in header and "amax / 448" in header
    assert ctypes.sizeof(L.Kv8) == 4 * 8
    # argument checks come before any device access
    assert lib.ekv_kv8_step_check(None, None, F16, None) == -1
    assert lib.ekv_kv8_quantize(None, None, F16, 0, 1, 1, None) == -1
    assert lib.ekv_kv8_dequantize(None, None, 2, 0, 1, 1, None, None, None) == -1
    assert lib.ekv_kv8_workspace_bytes(None, None, F16, None) == 0


def _answers(lib, bank, st, dtype, kv8):
    b, s = ctypes.byref(bank), ctypes.byref(st)
    info = (ctypes.c_int32 * 9)(*([-7] * 9))
    if kv8 is None:
        return [lib.ekv_step_check_typed(b, s, dtype), lib.ekv_step_info_typed(b, s, dtype, info, 9)] + list(info) + [lib.ekv_workspace_bytes_typed(b, s, dtype)]
    k = ctypes.byref(kv8)
    return [lib.ekv_kv8_step_check(b, s, dtype, k), lib.ekv_kv8_step_info(b, s, dtype, k, info, 9)] + list(info) + [lib.ekv_kv8_workspace_bytes(b, s, dtype, k)]


def test_kv8_dry_runs_over_the_dispatch_grid():
    L, lib = _lib()
    kv8 = L.Kv8(256, 256, 256, 256)
    cs = cases()
    n_ok = n_fused = n_split = 0
    for c in cs:
        bank, st = _structs(c)
        ref = _answers(lib, bank, st, F16, None)
        for dt in (F16, BF16):
            got = _answers(lib, bank, st, dt, kv8)
            takes = c["q_len"] == 1 and not c["rope_on_read"] and c["head_dim"] in (64, 128)
            if ref[0] == -1:                      # fp16's own EKV_E_ARG cases keep their code
                assert got[0] == -1, (c, got)
            elif ref[0] == 0 and takes:           # accepted, with the fp16 step's plan: splits, fused, launches, workspace
                assert got == ref, (c, got, ref)
                n_ok += dt == F16
                n_fused += dt == F16 and got[3] == 1
                n_split += dt == F16 and got[2] > 1
            else:                                 # chunk steps, RoPE-on-read, head_dim 32 / 96 / unbuilt, fp16's own refusals
                assert got[0] == -2, (c, got, ref)
                assert got[1] != 0 or (got[3] == 0 and got[10] == 0), (c, got)      # not fused, no launches
        for bad in (2, -1):
            assert lib.ekv_kv8_step_check(ctypes.byref(bank), ctypes.byref(st), bad, ctypes.byref(kv8)) == -1
            assert lib.ekv_kv8_step_info(ctypes.byref(bank), ctypes.byref(st), bad, ctypes.byref(kv8), (ctypes.c_int32 * 9)(), 9) == -1
    assert n_ok > 100 and n_fused > 10 and n_split > 10, (n_ok, n_fused, n_split)
    # the north-star shape (32 layers x 32 heads, T = 2049, cap 2112): a fused fp16 step is a fused kv8 step, on either score-row layout
    for extra in ({}, {"phases": 16, "phys_extent": 2112}):
        bank, st = _structs(_case(n_layers=32, **extra))
        ref, got = _answers(lib, bank, st, F16, None), _answers(lib, bank, st, F16, kv8)
        assert ref[0] == 0 and ref[3] == 1 and got == ref, (ref, got)
    # the explicit refusals
    for kw in (dict(q_len=8, n_slots=2056, n_evict=8, roco_k1=1800, count_add2=16), dict(rope_on_read=1), dict(head_dim=32), dict(head_dim=96)):
        bank, st = _structs(_case(n_layers=32, **kw))
        assert lib.ekv_step_check(ctypes.byref(bank), ctypes.byref(st)) == 0, kw
        assert lib.ekv_kv8_step_check(ctypes.byref(bank), ctypes.byref(st), F16, ctypes.byref(kv8)) == -2, kw
    # a descriptor with a missing plane is an argument error
    bank, st = _structs(_case(n_layers=32))
    assert lib.ekv_kv8_step_check(ctypes.byref(bank), ctypes.byref(st), F16, ctypes.byref(L.Kv8(256, 256, None, 256))) == -1
    # the 16-bit row pointers are not needed any more
    bank.k = bank.v = None
    assert lib.ekv_kv8_step_check(ctypes.byref(bank), ctypes.byref(st), F16, ctypes.byref(kv8)) == 0


def test_reference_rule_properties():
    g = torch.Generator().manual_seed(3)
    for dtype in (torch.float16, torch.bfloat16):
        for d in (64, 128):
            x = R.special_rows(64, d, g, dtype)
            codes, s = R.quantize(x)
            R.check_rows(x, codes, s, (dtype, d))
            assert bool((x.float().abs() <= 448 * s.unsqueeze(-1) * (1 + 2.0 ** -22)).all())
            back = R.dequant(codes, s)
            assert bool(((back - x.float()).abs() <= 0.0625 * x.float().abs() + 2.0 ** -9 * s.unsqueeze(-1) * 1.0001).all())     # half an ulp: 3 mantissa bits / the subnormal step 2^-9
            # the rows' maxima survive exactly up to the scale's rounding: code 448 at the arg-max
            nz = s != 1
            assert bool((codes.view(R.FP8).float().abs().amax(-1)[nz] == 448).all())
    # a check that can fail: a code one step off a non-tie is caught
    x = torch.tensor([[1.0, 0.3, -0.7, 0.11] * 16])
    codes, s = R.quantize(x)
    bad = codes.clone()
    bad[0, 1] += 1
    try:
        R.check_rows(x, bad, s)
    except AssertionError:
        pass
    else:
        raise AssertionError("check_rows accepted a wrong code")
