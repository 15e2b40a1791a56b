"""Batched decode steps (include/easykv_hip.h, ekv_seq) on a CPU: the four calls exist, and their dry runs plan a table as the
uniform multi-layer step of its envelope and refuse everything a batch does not take before a launch.  Dummy non-null pointers
throughout: nothing is dereferenced, nothing is launched."""
import ctypes
import itertools
import os
import re

from tests.test_dispatch_table import _case, _structs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("ekv_batch_step_check", "ekv_batch_step_info", "ekv_batch_workspace_bytes", "ekv_batch_step_attend")
F16, BF16 = 0, 1
TABLE_BYTES = 0      # the table travels in the kernel arguments: a batch needs exactly the workspace of its envelope's step


def _lib():
    from easykv_amd import _build, _lib as L
    if not os.path.exists(_build.LIB):
        _build.build_lib()
    return L, L.load()


def _table(L, entries):
    tb = (L.Seq * len(entries))()
    for i, e in enumerate(entries):
        for k, v in e.items():
            setattr(tb[i], k, v)
    return tb


def _uniform(L, st, layers):
    return _table(L, [dict(layer=l, n_slots=st.n_slots, score_off=st.score_off, n_evict=st.n_evict, win_lo=st.win_lo, win_tail=st.win_tail,
                           roco_k1=st.roco_k1, range_start=st.range_start, phys_extent=st.phys_extent) for l in layers])


def _step_answers(lib, bank, st, dtype):
    b, s = ctypes.byref(bank), ctypes.byref(st)
    info = (ctypes.c_int32 * 9)(*([-7] * 9))
    return [lib.ekv_step_check_typed(b, s, dtype), lib.ekv_step_info_typed(b, s, dtype, info, 9)] + list(info) + [lib.ekv_workspace_bytes_typed(b, s, dtype)]


def _batch_answers(lib, bank, st, dtype, tb, n=None):
    b, s = ctypes.byref(bank), ctypes.byref(st)
    n = len(tb) if n is None else n
    info = (ctypes.c_int32 * 9)(*([-7] * 9))
    return [lib.ekv_batch_step_check(b, s, dtype, tb, n), lib.ekv_batch_step_info(b, s, dtype, tb, n, info, 9)] + list(info) + \
           [lib.ekv_batch_workspace_bytes(b, s, dtype, tb, n) - TABLE_BYTES]


def test_batch_calls_are_exported_and_declared():
    L, lib = _lib()
    header = open(os.path.join(ROOT, "include", "easykv_hip.h")).read()
    declared = set(re.findall(r"\b(ekv_[a-z_]+)\s*\(", header))
    raw = ctypes.CDLL(L.LIB)
    for name in CALLS:
        assert name in declared and name in L.EXPORTS and hasattr(raw, name) and hasattr(lib, name), name
    assert lib.ekv_abi_version() == 8
    assert "typedef struct ekv_seq {" in header and "#define EKV_MAX_SEQS 64" in header
    assert ctypes.sizeof(L.Seq) == 9 * 4 and L.MAX_SEQS == 64
    # argument checks come before any device access
    assert lib.ekv_batch_step_check(None, None, F16, None, 1) == -1
    assert lib.ekv_batch_step_info(None, None, F16, None, 1, None, 0) == -1
    assert lib.ekv_batch_workspace_bytes(None, None, F16, None, 1) == 0
    assert lib.ekv_batch_step_attend(None, None, F16, None, 1, None, None, None, None, None, None, 0, None) == -1


def _policy_kw(policy, T):
    """A valid decode step of `policy` at length T (one victim wherever T leaves a candidate)."""
    ev = 1 if T >= 3 and policy != 0 else 0
    kw = dict(policy=policy, n_evict=ev, roco_k1=max(ev, T - T // 3), win_lo=0, win_tail=0, range_start=-1)
    if policy == 1:
        kw["win_tail"] = T // 4
    if policy == 4:
        kw["range_start"] = T // 2 if ev else -1
    return kw


def test_batch_plans_as_the_step_of_its_envelope():
    L, lib = _lib()
    n_uniform = n_ragged = n_one_launch = n_split = 0
    for d, (hq, h), n_seq, T, policy in itertools.product((32, 64, 96, 128), ((32, 32), (32, 8), (8, 2), (24, 8)), (1, 2, 8, 33),
                                                          (5, 300, 2049, 5002), (0, 1, 2, 3, 4)):
        cap = (T + 64 + 63) // 64 * 64
        c = _case(head_dim=d, hq=hq, h=h, n_layers=40, cap=cap, layer_begin=0, layer_count=n_seq, n_slots=T, **_policy_kw(policy, T))
        bank, st = _structs(c)
        for dt in (F16, BF16):
            ref = _step_answers(lib, bank, st, dt)
            assert ref[0] == 0, (c, ref)
            # a uniform table, its entries in a permuted, non-contiguous layer order: the multi-layer step, field for field
            layers = [(7 * i + 3) % 40 for i in range(n_seq)]
            got = _batch_answers(lib, bank, st, dt, _uniform(L, st, layers))
            assert got == ref, (c, dt, got, ref)
            n_uniform += 1
            n_one_launch += got[3] == 1
            n_split += got[2] > 1
            # what the step says about the per-sequence fields is ignored in favour of the table
            st2 = type(st).from_buffer_copy(st)
            st2.layer_begin, st2.layer_count, st2.n_slots, st2.n_evict, st2.roco_k1, st2.score_off = 39, 7, 1, 0, 0, 3
            assert _batch_answers(lib, bank, st2, dt, _uniform(L, st, layers)) == ref, (c, dt)
        # a ragged table: the plan of its envelope (longest entry, widest extent, any victim)
        if n_seq > 1:
            lens = [max(1, T * (i + 1) // n_seq - (i % 3)) for i in range(n_seq)]
            lens[n_seq // 2], lens[0] = T, min(lens[0], 2)
            entries = []
            for i, t in enumerate(lens):
                kw = _policy_kw(policy, t)
                if i % 2 == 0 and t != T:
                    kw.update(n_evict=0, range_start=-1)
                off = min(i, t - 1) if policy in (1, 2, 3) and t > 40 else 0
                if policy == 2:
                    kw["roco_k1"] = max(kw["n_evict"], (t - off) // 2)
                if policy == 1:
                    kw["win_tail"] = (t - off) // 4
                entries.append(dict(layer=(11 * i + 5) % 40, n_slots=t, score_off=off, phys_extent=min(cap, t + i), n_evict=kw["n_evict"],
                                    win_lo=0, win_tail=kw["win_tail"], roco_k1=kw["roco_k1"], range_start=kw["range_start"]))
            env = type(st).from_buffer_copy(st)
            env.n_slots, env.phys_extent = T, max(e["phys_extent"] for e in entries)
            env.n_evict = max(e["n_evict"] for e in entries)
            env.score_off, env.win_lo, env.win_tail, env.roco_k1, env.range_start = min(e["score_off"] for e in entries), 0, 0, env.n_evict, 0
            for dt in (F16, BF16):
                ref = _step_answers(lib, bank, env, dt)
                got = _batch_answers(lib, bank, st, dt, _table(L, entries))
                assert ref[0] == 0 and got == ref, (c, dt, entries, got, ref)
                n_ragged += 1
    assert n_uniform == 2 * 4 * 4 * 4 * 4 * 5 and n_ragged == 2 * 4 * 4 * 3 * 4 * 5 and n_one_launch > 100 and n_split > 100, (n_uniform, n_ragged, n_one_launch, n_split)


def test_batch_refusals_come_before_any_launch():
    L, lib = _lib()
    bank, st = _structs(_case(n_layers=32))
    tb = _uniform(L, st, range(8))
    assert _batch_answers(lib, bank, st, F16, tb)[0] == 0

    def refused(code, st=st, bank=bank, tb=tb, n=None, dt=F16):
        got = _batch_answers(lib, bank, st, dt, tb, n)
        assert got[0] == code, (code, got)
        if got[1] == 0:      # the info call answered: not one launch, no launches
            assert got[3] == 0 and got[10] == 0, got
        else:                # it refused its own arguments (bank, dtype): the same code, the array untouched
            assert got[1] in (-1, -2) and got[2:11] == [-7] * 9, got
        assert got[11] == 0, got      # a refused table needs no workspace
        b, s = ctypes.byref(bank), ctypes.byref(st)
        # the real call answers the same before it looks at a pointer
        assert lib.ekv_batch_step_attend(b, s, dt, tb, len(tb) if n is None else n, None, None, None, None, None, None, 0, None) == code

    # EKV_E_UNSUPPORTED: chunk steps, RoPE-on-read, the slot-indexed layout, phased and deferred forms, the head-averaged tova row
    for kw in (dict(q_len=8, n_slots=2056, n_evict=8, roco_k1=1800, count_add2=16), dict(rope_on_read=1), dict(phases=16, phys_extent=2112),
               dict(phases=1 | 4), dict(phases=8), dict(phases=1), dict(defer_layers=32, n_split=4, phases=8), dict(policy=3, tova_head_mean=1)):
        b2, s2 = _structs(_case(n_layers=32, **kw))
        refused(-2, st=s2, bank=b2)
    # ... and shapes only the generic scorer serves: GQA factors > 8, rows beyond the fast scorer's 6144 slots, cap % 4 != 0
    for kw in (dict(hq=48, h=4), dict(n_slots=7000, cap=7040, roco_k1=5000), dict(n_slots=2049, cap=2114)):
        b2, s2 = _structs(_case(n_layers=32, **kw))
        assert lib.ekv_step_check(ctypes.byref(b2), ctypes.byref(s2)) == 0, kw
        refused(-2, st=s2, bank=b2, tb=_uniform(L, s2, range(8)))
    # EKV_E_ARG: the table
    refused(-1, n=0)
    refused(-1, tb=_uniform(L, st, list(range(32)) * 3), n=65)
    refused(-1, tb=_uniform(L, st, [0, 1, 32]))
    refused(-1, tb=_uniform(L, st, [0, 1, -1]))
    refused(-1, tb=_uniform(L, st, [0, 5, 2, 5]))
    assert lib.ekv_batch_step_check(ctypes.byref(bank), ctypes.byref(st), F16, None, 4) == -1
    assert lib.ekv_batch_step_check(None, ctypes.byref(st), F16, tb, 8) == -1
    assert lib.ekv_batch_step_check(ctypes.byref(bank), None, F16, tb, 8) == -1
    for dt in (2, -1):
        refused(-1, dt=dt)
    # ... and entries the single-sequence step of that geometry refuses
    for field, bad in (("n_slots", 0), ("n_slots", 2113), ("roco_k1", 0), ("roco_k1", 2050), ("score_off", 2049), ("score_off", -1),
                       ("n_evict", -1), ("n_evict", 2049)):
        t2 = _uniform(L, st, range(8))
        setattr(t2[5], field, bad)
        refused(-1, tb=t2)
    b2, s2 = _structs(_case(n_layers=32, policy=4, range_start=4))
    t2 = _uniform(L, s2, range(8))
    assert _batch_answers(lib, b2, s2, F16, t2)[0] == 0
    t2[3].range_start = 2049
    refused(-1, st=s2, bank=b2, tb=t2)
    b2, s2 = _structs(_case(n_layers=32, policy=1, win_tail=200))
    t2 = _uniform(L, s2, range(8))
    assert _batch_answers(lib, b2, s2, F16, t2)[0] == 0
    t2[0].win_tail = 2049
    refused(-1, st=s2, bank=b2, tb=t2)
    # a short entry keeps its own bounds: a window that fits the envelope but not the entry is the entry's error
    t2 = _uniform(L, st, range(8))
    t2[2].n_slots, t2[2].roco_k1 = 100, 1434
    refused(-1, tb=t2)
    t2[2].roco_k1 = 60
    assert _batch_answers(lib, bank, st, F16, t2)[0] == 0
    # bad head_dim: the bank's own refusal
    b2, s2 = _structs(_case(n_layers=32, head_dim=48))
    refused(-2, st=s2, bank=b2)
