"""The long-row call family (ekv_long_*; include/easykv_hip.h, "long score rows") through ctypes dry runs, on a CPU.

Over the grid of tests/test_dispatch_table.py a long call plans exactly as the plain _typed call of the same (bank, step, dtype), except
where that plan ends in the generic scorer's launch: there it ends in the long-row scorer (info field 10), the launches grow by one — or
two, where the generic scorer would have folded the output itself —, the workspace by the scorer's scratch, and the width refusal of the
plain family is gone.  The Python layers refuse what has no long form (quantised rows, batches) before anything is loaded or launched,
and the build compiles the new object from the open manifest list."""
import ctypes

import numpy as np
import pytest

from tests.test_dispatch_table import _case, _structs, named_cases, random_cases


@pytest.fixture(scope="module")
def lib():
    from easykv_amd import _build, _lib
    import os
    if not os.path.exists(_build.LIB):
        _build.build_lib()
    return _lib.load()


def _plain(lib, c, dtype=0):
    bank, st = _structs(c)
    b, s = ctypes.byref(bank), ctypes.byref(st)
    info = (ctypes.c_int32 * 12)(*([-7] * 12))
    return lib.ekv_step_check_typed(b, s, dtype), lib.ekv_step_info_typed(b, s, dtype, info, 12), list(info), lib.ekv_workspace_bytes_typed(b, s, dtype)


def _long(lib, c, dtype=0):
    bank, st = _structs(c)
    b, s = ctypes.byref(bank), ctypes.byref(st)
    info = (ctypes.c_int32 * 12)(*([-7] * 12))
    return lib.ekv_long_step_check(b, s, dtype), lib.ekv_long_step_info(b, s, dtype, info, 12), list(info), lib.ekv_long_workspace_bytes(b, s, dtype)


def test_long_calls_plan_as_the_plain_calls_except_where_the_generic_scorer_would_run(lib):
    cs = named_cases() + random_cases()
    n_long = n_lifted = n_two = 0
    for dtype in (0, 1):
        for c in cs:
            prc, pirc, pinfo, pws = _plain(lib, c, dtype)
            lrc, lirc, linfo, lws = _long(lib, c, dtype)
            assert pirc == lirc, c
            if pirc != 0:      # (an argument error of the info call itself)
                assert prc == lrc, c
                continue
            assert pinfo[10:] == [0, 0], c      # (a plain call zeroes what lies beyond its ten fields)
            if linfo[10] == 0:
                assert (lrc, linfo[:10], lws) == (prc, pinfo[:10], pws), (c, prc, lrc, pinfo, linfo, pws, lws)
                assert linfo[11] == 0, c
                continue
            n_long += 1
            assert linfo[10] == 1 and lrc == 0, c
            W = c["n_slots"] - c["score_off"]
            assert linfo[11] == (W + 1023) // 1024, (c, linfo)
            assert linfo[:8] == pinfo[:8], (c, pinfo, linfo)
            if prc == 0:
                assert linfo[9] == pinfo[9], c
                # one launch more (sweep + select for the generic scorer's one); two where the generic scorer would have folded the
                # output itself: neither a scorer-only phase (8) nor an attention kernel that folds its own output
                add = 1 if (c["phases"] & 8) or pinfo[7] else 2
                n_two += add == 2
                assert linfo[8] == pinfo[8] + add, (c, pinfo, linfo)
                assert lws >= pws, c
            else:      # what only the width refusal of the plain family stood against
                n_lifted += 1
                assert prc == -2 and pinfo[8] == 0, (c, prc)
    assert n_long > 100 and n_lifted > 0 and n_two > 0, (n_long, n_lifted, n_two)


def test_the_pinned_width_refusal_is_lifted_by_the_long_call_only(lib):
    c = _case(cap=60032, n_slots=60000, roco_k1=30000, n_split=-1)
    bank, st = _structs(c)
    b, s = ctypes.byref(bank), ctypes.byref(st)
    assert lib.ekv_step_check(b, s) == -2 and lib.ekv_step_check_typed(b, s, 0) == -2
    info = (ctypes.c_int32 * 12)()
    assert lib.ekv_long_step_check(b, s, 0) == 0 and lib.ekv_long_step_info(b, s, 0, info, 12) == 0
    assert info[10] == 1 and info[11] == (60000 + 1023) // 1024
    # the scorer's scratch: three working rows and one key row of t_pad words per (layer, head), behind the plain layout
    t_pad = (60000 + 63) // 64 * 64
    grow = lib.ekv_long_workspace_bytes(b, s, 0) - lib.ekv_workspace_bytes_typed(b, s, 0)
    assert grow in (c["n_layers"] * c["h"] * t_pad * 4, c["n_layers"] * c["h"] * 4 * t_pad * 4), grow
    # a short info array is filled as far as it goes
    short = (ctypes.c_int32 * 11)(*([-7] * 11))
    assert lib.ekv_long_step_info(b, s, 0, short, 11) == 0 and short[10] == 1
    # ... and 130 000 slots, past 16-bit indices
    c = _case(cap=131136, n_slots=131073, roco_k1=65000, n_split=-1)
    bank, st = _structs(c)
    assert lib.ekv_long_step_check(ctypes.byref(bank), ctypes.byref(st), 1) == 0


def test_argument_errors_stay_argument_errors(lib):
    bad = [_case(n_evict=-1), _case(n_slots=4000), _case(policy=9), _case(roco_k1=0), _case(layer_begin=5), _case(score_off=-1),
           _case(cap=60032, n_slots=60000, roco_k1=70000, n_split=-1), _case(cap=60032, n_slots=60000, roco_k1=30000, n_split=-1, phases=2 | 8)]
    for c in bad:
        assert _plain(lib, c)[0] == -1 and _long(lib, c)[0] == -1, c
    c = _case()
    assert _long(lib, c, dtype=2)[:2] == (-1, -1) and _long(lib, c, dtype=-1)[:2] == (-1, -1)
    bank, st = _structs(c)
    info = (ctypes.c_int32 * 12)()
    assert lib.ekv_long_step_check(None, ctypes.byref(st), 0) == -1 and lib.ekv_long_step_check(ctypes.byref(bank), None, 0) == -1
    assert lib.ekv_long_step_info(ctypes.byref(bank), ctypes.byref(st), 0, None, 12) == -1
    assert lib.ekv_long_step_info(ctypes.byref(bank), ctypes.byref(st), 0, info, 0) == -1
    assert lib.ekv_long_workspace_bytes(None, None, 0) == 0
    # an unsupported head_dim is what the attention kernels refuse: unsupported in both families
    c = _case(head_dim=48)
    assert _plain(lib, c)[0] == -2 and _long(lib, c)[0] == -2


def test_quantised_rows_and_batches_have_no_long_form():
    from easykv_amd import _lib
    from easykv_amd.engine import KVBank, KVBankBatch, ROW_FORMATS
    for kind in ROW_FORMATS:      # (refused before the library is loaded or a device is touched)
        with pytest.raises(_lib.EkvError, match="long_rows=True.*16-bit rows"):
            KVBank(1, 4, 4, 128, 256, device="cuda", kv_quant=kind, long_rows=True)
    with pytest.raises(_lib.EkvError, match="long_rows=True.*single sequences"):
        KVBankBatch(2, 1, 4, 4, 128, 256, device="cuda", long_rows=True)
    bank = object.__new__(KVBank)      # (a long_rows bank as quantize() finds it: the refusal precedes every other look at the bank)
    bank.long_rows = True
    for kind in ROW_FORMATS:
        with pytest.raises(_lib.EkvError, match="long_rows=True"):
            bank.quantize(kind)
    # the long family has exactly the four uniform 16-bit calls: no quantised and no batched name
    assert sorted(_lib.LONG_CALLS.values()) == ["ekv_long_step_attend", "ekv_long_step_check", "ekv_long_step_info", "ekv_long_workspace_bytes"]
    assert [n for n in _lib.EXPORTS if "long" in n] == [_lib.LONG_CALLS[w] for w in _lib.STEP_CALLS]


def test_driver_refuses_long_rows_with_quantised_rows_and_in_batches():
    import torch
    from easykv_amd import api
    from tests.native_fake_model import NativeFakeModel
    model = NativeFakeModel(torch.zeros(1, 4, 64, 128), torch.zeros(1, 4, 64, 128), torch.zeros(1, 4, 64, 128), device="cpu")
    ids = torch.arange(1, 40).view(1, -1)      # (every refusal below precedes the first launch: generation_config is read once, up front)
    cfg = dict(budget=16, kv_policy="roco", max_new_tokens=2, long_rows=True)
    with pytest.raises(ValueError, match="long_rows.*kv_quant"):
        api.generate(model, ids, dict(cfg, kv_quant="fp8"))
    with pytest.raises(ValueError, match="long_rows.*False or True"):
        api.generate(model, ids, dict(cfg, long_rows="auto"))
    with pytest.raises(ValueError, match="generate_batch.*long_rows"):
        api.generate_batch(model, [ids, ids], cfg)


def test_long_object_is_among_the_later_objects_only():
    from easykv_amd import _build
    every, added, later = dict(_build.objects()), dict(_build.added_objects()), dict(_build.later_objects())
    assert "ekv_score_long" in later and "ekv_score_long" not in every and "ekv_score_long" not in added
    assert later["ekv_score_long"][-1].endswith("ekv_score_long.inc")
    assert ("EKV_SCORE_LONG", ("1024",)) in _build.later_instances()
    assert len(later) == len(_build.later_objects()) == len(_build.later_instances())
    # no new translation unit of the library's own: the recorded object list stands
    assert not [n for n in every if "long" in n]
