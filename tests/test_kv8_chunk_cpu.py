"""Chunk steps on FP8 rows ("kv8 chunks", include/easykv_hip.h) on a CPU: the dry runs of the ekv_kv8_chunk_* calls.  Dummy non-null
pointers throughout: nothing is dereferenced, nothing is launched."""
import ctypes
import itertools

import pytest

from tests.test_dispatch_table import _case, _chunk, _structs

F16, BF16 = 0, 1
POLICIES = dict(full=0, h2o_head=1, roco=2, tova=3)


def _lib():
    from tests.test_kv8_cpu import _lib as load
    return load()


def _answers(fns, bank, st, dtype, kv8):
    check, info_fn, ws = fns
    b, s, k = ctypes.byref(bank), ctypes.byref(st), ctypes.byref(kv8)
    info = (ctypes.c_int32 * 10)(*([-7] * 10))
    return [check(b, s, dtype, k), info_fn(b, s, dtype, k, info, 10)] + list(info) + [ws(b, s, dtype, k)]


def _step(D, rep, n, policy, t_prev=200):
    scored = policy != "full"
    kw = dict(policy=POLICIES[policy], accumulate=int(scored))
    if n == 1:
        return _case(head_dim=D, hq=2 * rep, h=2, n_slots=t_prev + 1, cap=320, n_evict=int(scored), roco_k1=150, **kw)
    return _chunk(2, 2 * rep, 2, n, t_prev, d=D, **(kw if scored else dict(kw, n_evict=0)))


@pytest.mark.parametrize("D,rep,n,policy,dtype", list(itertools.product((64, 128), (1, 4), (1, 8, 40), POLICIES, (F16, BF16))))
def test_chunk_family_plans_the_grid(D, rep, n, policy, dtype):
    L, lib = _lib()
    kv8 = L.Kv8(256, 256, 256, 256)
    new = (lib.ekv_kv8_chunk_step_check, lib.ekv_kv8_chunk_step_info, lib.ekv_kv8_chunk_workspace_bytes)
    old = (lib.ekv_kv8_step_check, lib.ekv_kv8_step_info, lib.ekv_kv8_workspace_bytes)
    bank, st = _structs(_step(D, rep, n, policy))
    got = _answers(new, bank, st, dtype, kv8)
    assert got[0] == 0 and got[1] == 0 and got[2 + 8] > 0 and got[-1] > 0, got      # EKV_OK, n_launches > 0
    if n == 1:
        assert got == _answers(old, bank, st, dtype, kv8)      # field for field the decode call's
    else:
        assert lib.ekv_kv8_step_check(ctypes.byref(bank), ctypes.byref(st), dtype, ctypes.byref(kv8)) == -2      # the decode family still refuses
        two_pass, wide, n_qblocks, qb_rows = got[2 + 2], got[2 + 3], got[2 + 4], got[2 + 5]
        assert two_pass == 0 and wide == 0 and qb_rows * rep <= 32 and n_qblocks == -(-n // qb_rows), got


@pytest.mark.parametrize("kw", [dict(d=32), dict(d=96), dict(rope_on_read=1), dict(hq=128, h=2), dict(phases=16, phys_extent=256)],
                         ids=["head_dim 32", "head_dim 96", "RoPE-on-read", "rep 64", "slot-indexed rows"])
def test_chunk_family_refusals(kw):
    L, lib = _lib()
    kv8 = L.Kv8(256, 256, 256, 256)
    new = (lib.ekv_kv8_chunk_step_check, lib.ekv_kv8_chunk_step_info, lib.ekv_kv8_chunk_workspace_bytes)
    bank, st = _structs(_chunk(2, kw.pop("hq", 4), kw.pop("h", 2), 8, 200, **kw))
    for dt in (F16, BF16):
        got = _answers(new, bank, st, dt, kv8)
        assert got[0] == -2 and got[2 + 1] == 0 and got[2 + 8] == 0 and got[-1] == 0, got      # EKV_E_UNSUPPORTED: not fused, zero launches, zero bytes
    assert lib.ekv_kv8_chunk_step_check(ctypes.byref(bank), ctypes.byref(st), 2, ctypes.byref(kv8)) == -1
    assert lib.ekv_kv8_chunk_step_check(ctypes.byref(bank), ctypes.byref(st), F16, ctypes.byref(L.Kv8(256, None, 256, 256))) == -1
