"""Batched decode steps on MXFP6 K/V rows (include/easykv_hip.h, "kv6 batches") on a CPU: the four calls exist, their dry runs plan a
table exactly as the 16-bit batched call plans it (a uniform table: as the kv6 multi-layer step it spells out) and refuse what either
family refuses before a launch, the build links the two new objects (easykv_amd._build.added_objects()) beside the recorded lists, the planner's kv6 + batch stages run
clean as a stand-alone program under AddressSanitizer + UBSan (tests/plan_kv6_main.cpp) with the library's answers, and the seeded
inputs of the ragged GPU cases (tests/test_hip_batch_kv6.py, cases (b) and (c)) leave the oracle's decisions well defined.  Dummy
non-null pointers throughout: nothing is dereferenced, nothing is launched."""
import ctypes
import itertools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import batch_kv6_cases as cases
from tests import kv6_ref as R
from tests.test_batch_cpu import _batch_answers, _lib, _policy_kw, _table, _uniform
from tests.test_dispatch_table import KEYS, SWITCHES, _case, _structs
from tests.test_dispatch_table import cases as dispatch_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("ekv_kv6_batch_step_check", "ekv_kv6_batch_step_info", "ekv_kv6_batch_workspace_bytes", "ekv_kv6_batch_step_attend")
OBJECTS = ["ekv_attn_decode_d128_plain_batch_kv6", "ekv_attn_decode_d128_plain_batch_kv6_bf16"]
SEQ_KEYS = ("layer", "n_slots", "score_off", "n_evict", "win_lo", "win_tail", "roco_k1", "range_start", "phys_extent")
F16, BF16 = 0, 1
GQA = ((32, 32), (32, 8), (8, 2), (24, 8))      # the head shapes tests/test_batch_kv8_cpu.py sweeps: GQA x 1, x 4, x 4, x 3 (padded build)


def _kv6_batch_answers(lib, bank, st, dtype, kv6, tb, n=None):
    b, s, k = ctypes.byref(bank), ctypes.byref(st), (ctypes.byref(kv6) if kv6 is not None else None)
    n = len(tb) if n is None else n
    info = (ctypes.c_int32 * 9)(*([-7] * 9))
    return [lib.ekv_kv6_batch_step_check(b, s, dtype, k, tb, n), lib.ekv_kv6_batch_step_info(b, s, dtype, k, tb, n, info, 9)] + list(info) + \
           [lib.ekv_kv6_batch_workspace_bytes(b, s, dtype, k, tb, n)]


def _kv6_step_answers(lib, bank, st, dtype, kv6):
    b, s, k = ctypes.byref(bank), ctypes.byref(st), ctypes.byref(kv6)
    info = (ctypes.c_int32 * 9)(*([-7] * 9))
    return [lib.ekv_kv6_step_check(b, s, dtype, k), lib.ekv_kv6_step_info(b, s, dtype, k, info, 9)] + list(info) + [lib.ekv_kv6_workspace_bytes(b, s, dtype, k)]


def _ragged_entries(n_seq, T, policy, cap):
    """The ragged table of tests/test_batch_cpu.py / tests/test_batch_kv8_cpu.py for this envelope."""
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
    return entries


def _sweep():
    """(case, uniform entries, ragged entries or None) over the tables tests/test_batch_kv8_cpu.py sweeps, at head_dim 128, GQA <= 4."""
    for (hq, h), n_seq, T, policy in itertools.product(GQA, (1, 2, 8, 33), (5, 300, 2049, 5002), (0, 1, 2, 3, 4)):
        cap = (T + 64 + 63) // 64 * 64
        c = _case(head_dim=128, hq=hq, h=h, n_layers=40, cap=cap, layer_begin=0, layer_count=n_seq, n_slots=T, **_policy_kw(policy, T))
        uniform = [dict(layer=(7 * i + 3) % 40, **{k: c[k] for k in SEQ_KEYS[1:]}) for i in range(n_seq)]
        yield c, uniform, (_ragged_entries(n_seq, T, policy, cap) if n_seq > 1 else None)


# ---- 1. exports and declarations ----------------------------------------------------------------------------------------------------
def test_kv6_batch_calls_are_exported_and_declared():
    L, lib = _lib()
    header = open(os.path.join(ROOT, "include", "easykv_hip.h")).read()
    declared = set(re.findall(r"\b(ekv_[a-z0-9_]+)\s*\(", header))
    raw = ctypes.CDLL(L.LIB)
    for name in CALLS:
        assert name in declared and name in L.EXPORTS and hasattr(raw, name) and hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name      # typed by load()
    assert lib.ekv_abi_version() == 8
    assert lib.ekv_kv6_batch_workspace_bytes.restype is ctypes.c_size_t and lib.ekv_kv6_batch_step_check.restype is ctypes.c_int
    assert "There is no batch form" not in header and '"kv6 batches"' in header
    # argument checks come before any device access
    assert lib.ekv_kv6_batch_step_check(None, None, F16, None, None, 1) == -1
    assert lib.ekv_kv6_batch_step_info(None, None, F16, None, None, 1, None, 0) == -1
    assert lib.ekv_kv6_batch_workspace_bytes(None, None, F16, None, None, 1) == 0
    assert lib.ekv_kv6_batch_step_attend(None, None, F16, None, None, 1, None, None, None, None, None, None, 0, None) == -1


# ---- 2. plan identity ---------------------------------------------------------------------------------------------------------------
def test_kv6_batch_plans_as_the_16_bit_batch_and_as_the_kv6_multi_layer_step():
    """Return code, the nine info fields, fused_order 0 and the workspace bytes are ekv_batch_*'s of the same table; a uniform table
    also equals ekv_kv6_step_* of the multi-layer step it spells out."""
    L, lib = _lib()
    kv6 = L.Kv6(256, 256, 256, 256)
    n_uniform = n_ragged = n_one_launch = n_split = 0
    for c, uniform, ragged in _sweep():
        bank, st = _structs(c)
        for ti, entries in enumerate((uniform, ragged)):
            if entries is None:
                continue
            tb = _table(L, entries)
            for dt in (F16, BF16):
                ref = _batch_answers(lib, bank, st, dt, tb)
                got = _kv6_batch_answers(lib, bank, st, dt, kv6, tb)
                assert ref[0] == 0 and got == ref, (c, dt, ti, got, ref)
                info = (ctypes.c_int32 * 10)(*([-7] * 10))
                assert lib.ekv_kv6_batch_step_info(ctypes.byref(bank), ctypes.byref(st), dt, ctypes.byref(kv6), tb, len(tb), info, 10) == 0
                assert list(info)[:9] == got[2:11] and info[9] == 0, list(info)      # fused_order 0: the kv6 batch instances keep order F
                if ti == 0:
                    solo = _kv6_step_answers(lib, bank, st, dt, kv6)
                    assert solo == got, (c, dt, solo, got)
                n_uniform += ti == 0
                n_ragged += ti == 1
                n_one_launch += got[3] == 1
                n_split += got[2] > 1
    assert n_uniform == 2 * 4 * 4 * 4 * 5 and n_ragged == 2 * 4 * 3 * 4 * 5 and n_one_launch > 50 and n_split > 50, (n_uniform, n_ragged, n_one_launch, n_split)
    # the 16-bit row pointers are not needed
    bank, st = _structs(_case(n_layers=32))
    tb = _uniform(L, st, range(8))
    ref = _batch_answers(lib, bank, st, F16, tb)
    bank.k = bank.v = None
    assert ref[0] == 0 and _kv6_batch_answers(lib, bank, st, F16, kv6, tb) == ref


# ---- 3. refusals --------------------------------------------------------------------------------------------------------------------
def test_kv6_batch_refusals_come_before_any_launch():
    L, lib = _lib()
    kv6 = L.Kv6(256, 256, 256, 256)
    bank, st = _structs(_case(n_layers=32))
    tb = _uniform(L, st, range(8))
    assert _kv6_batch_answers(lib, bank, st, F16, kv6, tb)[0] == 0

    def refused(code, st=st, bank=bank, tb=tb, n=None, dt=F16, kv6=kv6):
        got = _kv6_batch_answers(lib, bank, st, dt, kv6, tb, n)
        assert got[0] == code, (code, got)
        if got[1] == 0:      # the info call answered: not one launch, no launches
            assert got[3] == 0 and got[10] == 0, got
        else:                # it refused its own arguments: the same code, the array untouched
            assert got[1] in (-1, -2) and got[2:11] == [-7] * 9, got
        assert got[11] == 0, got      # zero bytes
        b, s = ctypes.byref(bank), ctypes.byref(st)
        k = ctypes.byref(kv6) if kv6 is not None else None
        # the real call answers the same before it looks at a pointer
        assert lib.ekv_kv6_batch_step_attend(b, s, dt, k, tb, len(tb) if n is None else n, None, None, None, None, None, None, 0, None) == code

    # EKV_E_UNSUPPORTED: what a kv6 step refuses (head_dim 32 / 64 / 96, GQA factors 5 and 8), each of a table the 16-bit batch takes ...
    for kw in (dict(head_dim=32), dict(head_dim=64), dict(head_dim=96), dict(hq=40, h=8), dict(hq=64, h=8)):
        b2, s2 = _structs(_case(n_layers=32, **kw))
        t2 = _uniform(L, s2, range(8))
        assert _batch_answers(lib, b2, s2, F16, t2)[0] == 0, kw
        refused(-2, st=s2, bank=b2, tb=t2)
    for kw in (dict(hq=24, h=8), dict(hq=32, h=8), dict(hq=16, h=8)):      # GQA x 3 (padded build), x 4, x 2: taken
        b2, s2 = _structs(_case(n_layers=32, **kw))
        assert _kv6_batch_answers(lib, b2, s2, F16, kv6, _uniform(L, s2, range(8)))[0] == 0, kw
    # ... and what either family refuses: RoPE-on-read, chunk steps, every `phases` bit, deferred steps, the head-averaged tova row
    for kw in (dict(rope_on_read=1), dict(q_len=8, n_slots=2056, n_evict=8, roco_k1=1800, count_add2=16), dict(phases=16, phys_extent=2112),
               dict(phases=1 | 4), dict(phases=8), dict(phases=1), dict(phases=4), dict(phases=2), dict(phases=32, phys_extent=2112),
               dict(defer_layers=32, n_split=4, phases=8), dict(policy=3, tova_head_mean=1)):
        b2, s2 = _structs(_case(n_layers=32, **kw))
        refused(-2, st=s2, bank=b2)
    # ... and scored shapes only the generic scorer serves: more than 6144 slots, cap % 4 != 0
    for kw in (dict(n_slots=7000, cap=7040, roco_k1=5000), dict(n_slots=2049, cap=2114)):
        b2, s2 = _structs(_case(n_layers=32, **kw))
        refused(-2, st=s2, bank=b2, tb=_uniform(L, s2, range(8)))
    # EKV_E_ARG: a missing descriptor or plane — before the table is read (a NULL table next to it changes nothing)
    refused(-1, kv6=None)
    for i in range(4):
        planes = [256] * 4
        planes[i] = None
        refused(-1, kv6=L.Kv6(*planes))
        assert lib.ekv_kv6_batch_step_check(ctypes.byref(bank), ctypes.byref(st), F16, ctypes.byref(L.Kv6(*planes)), None, 8) == -1
    # ... a bad element type, and the bad tables of the kv8-batch test
    for dt in (2, -1):
        refused(-1, dt=dt)
    refused(-1, n=0)
    refused(-1, tb=_uniform(L, st, list(range(32)) * 3), n=65)
    refused(-1, tb=_uniform(L, st, [0, 1, 32]))
    refused(-1, tb=_uniform(L, st, [0, 5, 2, 5]))
    assert lib.ekv_kv6_batch_step_check(ctypes.byref(bank), ctypes.byref(st), F16, ctypes.byref(kv6), None, 4) == -1
    assert lib.ekv_kv6_batch_step_check(None, ctypes.byref(st), F16, ctypes.byref(kv6), tb, 8) == -1
    assert lib.ekv_kv6_batch_step_check(ctypes.byref(bank), None, F16, ctypes.byref(kv6), tb, 8) == -1
    for field, bad in (("n_slots", 0), ("n_slots", 2113), ("roco_k1", 0), ("score_off", 2049), ("n_evict", 2049)):
        t2 = _uniform(L, st, range(8))
        setattr(t2[5], field, bad)
        refused(-1, tb=t2)
    # a short entry keeps its own bounds
    t2 = _uniform(L, st, range(8))
    t2[2].n_slots, t2[2].roco_k1 = 100, 1434
    refused(-1, tb=t2)
    t2[2].roco_k1 = 60
    assert _kv6_batch_answers(lib, bank, st, F16, kv6, t2)[0] == 0


# ---- 4. build -----------------------------------------------------------------------------------------------------------------------
def test_batch_kv6_objects_are_built_beside_the_recorded_lists():
    from easykv_amd import _build
    every, added = [n for n, _ in _build.objects()], dict(_build.added_objects())
    assert [n for n in added if "batch_kv6" in n] == OBJECTS and not set(added) & set(every) and not any("kv6" in n for n in every)
    # the other quantised objects are there under the names their own tests hold them to
    for n in ["ekv_kv4", "ekv_attn_decode_d128_plain_kv4", "ekv_attn_decode_d128_plain_batch_kv4"] + \
            [f"ekv_attn_decode_d{d}_plain_batch_kv8{t}" for d in (64, 128) for t in ("", "_bf16")]:
        assert n in every, n
    lines = [(fam, w) for fam, w in _build.added_instances() if "kv6" in w and "batch" in w]
    assert lines == [("EKV_DECODE", ("128", "plain", "f16", "kv6", "batch")), ("EKV_DECODE", ("128", "plain", "bf16", "kv6", "batch"))]
    for n in OBJECTS:
        assert "-DEKV_KV6=1" in added[n] and "-DEKV_BATCH=1" in added[n] and "-DEKV_D=128" in added[n] and added[n][-1].endswith("ekv_attn_decode.inc")
    assert "-DEKV_BF16=1" in added[OBJECTS[1]] and "-DEKV_BF16=1" not in added[OBJECTS[0]]
    _build.build_lib()
    t = os.path.getmtime(_build.ADDED_MANIFEST)
    for n in OBJECTS:
        obj = os.path.join(_build.OBJ, n + ".o")
        assert os.path.exists(obj) and os.path.getmtime(obj) >= t, n
    syms = subprocess.run(["nm", "-D", "--defined-only", _build.LIB], capture_output=True, text=True).stdout
    for elem in ("f16", "bf16"):
        assert f"ekv_launch_decode_fused_d128_plain_{elem}_kv6_batch" in syms and f"ekv_launch_attn_decode_d128_plain_{elem}_kv6_batch" in syms


# ---- 5. the host planner under sanitizers ---------------------------------------------------------------------------------------------
COMPILERS = [c for c in ("g++", "/opt/rocm/llvm/bin/clang++") if shutil.which(c)]
I32_MAX = 2 ** 31 - 1
SPECIAL = (-2 ** 31, -7, -1, 0, 1, I32_MAX, I32_MAX - 1, I32_MAX - 63)


@pytest.fixture(scope="module", params=COMPILERS or [None], ids=lambda c: os.path.basename(c) if c else "none")
def program(request, tmp_path_factory):
    if request.param is None:
        pytest.skip("no host C++ compiler on this machine")
    exe = str(tmp_path_factory.mktemp("plan_kv6") / "plan_kv6_main")
    # (the sanitizer runtimes linked into the program; nothing is loaded into Python)
    static = ["-static-libasan", "-static-libubsan"] if os.path.basename(request.param) == "g++" else []
    cmd = [request.param, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", *static,
           "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", os.path.join(ROOT, "tests", "plan_kv6_main.cpp"),
           os.path.join(ROOT, "easykv_amd", "csrc", "ekv_plan.cpp"), "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    return exe


def _line(c, dtype=0, plane=0, nulls=0, seqs=None, n_seq=None):
    v = [c[k] for k in KEYS] + [dtype, plane, nulls, int(seqs is not None), (len(seqs) if n_seq is None else n_seq) if seqs is not None else 0]
    for e in seqs or []:
        v += [e[k] for k in SEQ_KEYS]
    return " ".join(str(int(x)) for x in v)


def _library(L, lib, c, dtype=0, plane=0, nulls=0, seqs=None, n_seq=None):
    """The same kv6 call through the C ABI of the library: the row the program prints."""
    p = lambda on: 256 if on else None
    bank = L.Bank(p(not nulls & 4), p(not nulls & 8), p(not nulls & 16), p(c["score_sum"]), p(c["score_sq"]), p(c["score_sq"]), c["n_layers"],
                  c["hq"], c["h"], c["head_dim"], c["cap"], p(c["arrive"]), p(c["birth"]), p(c["birth"]))
    st = L.Step()
    for k in KEYS[9:]:
        if k != "count_add2":
            setattr(st, k, c[k])
    st.count_add, st.count_tail_step, st.sm_div = c["count_add2"] / 2, -1.0 if c["q_len"] > 1 else 0.0, 1.0
    b = None if nulls & 1 else ctypes.byref(bank)
    s = None if nulls & 2 else ctypes.byref(st)
    q6 = L.Kv6(*[p(not (nulls & 64 and plane == i)) for i in range(4)])
    q = None if nulls & 32 else ctypes.byref(q6)
    info = (ctypes.c_int32 * 10)(*([-7] * 10))
    if seqs is not None:
        n = len(seqs) if n_seq is None else n_seq
        tb = (L.Seq * max(len(seqs), 1))()
        for i, e in enumerate(seqs):
            for k in SEQ_KEYS:
                setattr(tb[i], k, e[k])
        t = None if nulls & 128 else tb
        rc = [lib.ekv_kv6_batch_step_check(b, s, dtype, q, t, n), lib.ekv_kv6_batch_step_info(b, s, dtype, q, t, n, info, 10), lib.ekv_kv6_batch_workspace_bytes(b, s, dtype, q, t, n)]
    else:
        rc = [lib.ekv_kv6_step_check(b, s, dtype, q), lib.ekv_kv6_step_info(b, s, dtype, q, info, 10), lib.ekv_kv6_workspace_bytes(b, s, dtype, q)]
    return rc[:2] + list(info) + [rc[2]]


def _u64(rows):
    return np.array([[int(x) & (2 ** 64 - 1) for x in row] for row in rows], dtype=np.uint64)


def _same(L, lib, exe, calls):
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    lines = [_line(*a, **kw) for a, kw in calls]
    r = subprocess.run([exe], input="\n".join(lines) + "\n", env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-4000:])      # a sanitizer report ends the program with a non-zero status
    got = _u64(ln.split() for ln in r.stdout.splitlines())
    assert got.shape == (len(calls), 13), got.shape
    want = _u64(_library(L, lib, *a, **kw) for a, kw in calls)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert len(bad) == 0, [(calls[i], want[i].tolist(), got[i].tolist()) for i in bad[:3]]


def _arbitrary_calls(n=20000, seed=20261019):
    """Seeded arbitrary kv6 descriptors, 7 in 10 with a table: int32 fields negative / 0 / 1 / typical / near INT32_MAX, null pointers
    and planes, n_seq -1 .. 65 — the sweep of tests/test_plan_host_cpu.py aimed at the kv6 + batch stages."""
    rs = np.random.RandomState(seed)
    typical = dispatch_cases() + [c for c, _, _ in _sweep()]
    calls = []
    for _ in range(n):
        c = dict(typical[rs.randint(len(typical))])
        p_field = (0.01, 0.03, 0.1, 0.3)[rs.randint(4)]
        for k in KEYS:
            if k not in ("arrive", "birth", "score_sum", "score_sq", "count_add2") and rs.rand() < p_field:
                c[k] = SPECIAL[rs.randint(len(SPECIAL))]
        kw = dict(dtype=int(rs.choice([0, 0, 0, 1, 1, 2, -1])), plane=int(rs.randint(4)))
        kw["nulls"] = int(sum(bit for bit in (1, 2, 4, 8, 16, 32, 64, 128) if rs.rand() < 0.02))
        if rs.rand() < 0.7:
            n_seq = int(rs.randint(-1, 66))
            seqs = []
            for i in range(max(n_seq, 0)):
                e = dict(layer=i, n_slots=max(1, c["n_slots"] - int(rs.randint(0, 40))), score_off=c["score_off"], n_evict=c["n_evict"], win_lo=c["win_lo"],
                         win_tail=c["win_tail"], roco_k1=c["roco_k1"], range_start=c["range_start"], phys_extent=c["phys_extent"])
                for k in SEQ_KEYS:
                    if rs.rand() < 0.03:
                        e[k] = SPECIAL[rs.randint(len(SPECIAL))]
                seqs.append(e)
            kw.update(seqs=seqs, n_seq=n_seq)
        calls.append(((c,), kw))
    return calls


def test_host_planner_kv6_batch_tables_under_sanitizers(program):
    """The uniform and ragged tables of the sweep above in both element types, each missing plane, and 20 000 arbitrary descriptors:
    the stand-alone program ends without a sanitizer report and prints the library's answers."""
    L, lib = _lib()
    calls = []
    for c, uniform, ragged in _sweep():
        for dt in (F16, BF16):
            calls.append(((c,), dict(dtype=dt, seqs=uniform)))
            if ragged is not None:
                calls.append(((c,), dict(dtype=dt, seqs=ragged)))
    n_tables = len(calls)
    assert n_tables == 2 * 4 * 4 * 4 * 5 + 2 * 4 * 3 * 4 * 5
    c0 = _case(n_layers=32)
    tb0 = [dict(layer=i, **{k: c0[k] for k in SEQ_KEYS[1:]}) for i in range(8)]
    calls += [((c0,), dict(seqs=tb0, nulls=64, plane=i)) for i in range(4)] + [((c0,), dict(seqs=tb0, nulls=32)), ((c0,), dict(seqs=tb0, nulls=128))]
    calls += [((_case(n_layers=32, head_dim=d),), dict(seqs=tb0)) for d in (32, 64, 96)] + [((_case(n_layers=32, hq=64, h=8),), dict(seqs=tb0))]
    calls += _arbitrary_calls()
    _same(L, lib, program, calls)
    # (the sweep means something: most tables are accepted, and the arbitrary descriptors reach every return code)
    codes = [_library(L, lib, *a, **kw)[0] for a, kw in calls]
    assert all(x == 0 for x in codes[:n_tables]) and {0, -1, -2} <= set(codes[n_tables:]), sorted(set(codes))


# ---- 6. precondition of the ragged GPU cases, on the reference side alone ---------------------------------------------------------------
def _deq(x):
    return R.dequant(*R.quantize(x))


@pytest.mark.parametrize("policy", cases.POLICIES)
@pytest.mark.parametrize("draw", [0, 1], ids=["short_first", "short_last"])
@pytest.mark.parametrize("shape", list(cases.SHAPES))
def test_ragged_case_inputs_leave_the_oracles_decisions_well_defined(shape, draw, policy):
    """The precondition of GPU case (b): the oracle over the case's seeded inputs, prompt rows and appended rows quantised by
    tests/kv6_ref.py, must find at least 90 % of EACH evicting entry's decisions well defined under tests.test_hip_fullsize.Probe.  A
    seed that does not meet it is changed (tests/batch_kv6_cases.py SEEDS), never the cap."""
    from oracle import easykv_oracle as O
    from tests.test_hip_fullsize import Probe
    D, Hq, H, dtype = cases.SHAPES[shape]
    entries, tokens = cases.inputs(shape, draw)
    assert D == 128 and Hq // H <= 4
    assert [e["T"] for e in entries] == (list(cases.RAGGED_T) if draw == 0 else list(reversed(cases.RAGGED_T)))
    assert {2, 17, 96, 300, 2049} <= set(cases.RAGGED_T) and len(cases.RAGGED_T) == 10 and len(tokens) == 2
    assert all(cases.EVICTS[t] for t in (96, 300, 2049)) and not cases.EVICTS[2] and not cases.EVICTS[17]
    if dtype is torch.bfloat16:      # V clamped to +-0.49 (0.4902 once rounded to bf16): every output stays below 0.5
        assert all(float(e["v0"].float().abs().max()) < 0.5 for e in entries if e["T"] > 2) and all(float(v.float().abs().max()) < 0.5 for _, _, v in tokens)
    probe = Probe()
    O.SELECT_HOOK = probe
    try:
        for i, e in enumerate(entries):
            if not e["evict"]:
                continue
            st = O.LayerState(k=_deq(e["k0"]).unsqueeze(0), v=_deq(e["v0"]).unsqueeze(0))
            st.s, st.q, st.c = O.init_state_decoding((H,), e["W"] - 1)
            st.s[:, :e["W"] - 1] += e["warm"]
            st.q[:, :e["W"] - 1] += e["warm"] ** 2
            n_dec = n_stable = 0
            for q, k, v in tokens:
                _, ids = O.layer_step(st, q[i:i + 1].float(), _deq(k[i:i + 1]), _deq(v[i:i + 1]), O.StepPlan(**cases.plan_kw(e, policy)))
                assert ids is not None and st.k.shape[2] == e["T"] - 1
                n_dec += H
                n_stable += int((~probe.last_unstable).sum())
            print(f"[kv6-batch-precondition] {shape} draw {draw} {policy} T={e['T']}: {n_stable} of {n_dec} decisions well defined")
            assert n_stable >= 0.9 * n_dec, (shape, draw, policy, e["T"], n_stable, n_dec)
    finally:
        O.SELECT_HOOK = None


def test_lockstep_inputs_leave_the_oracles_decisions_well_defined():
    """The same precondition for GPU case (c): every sequence of the lockstep run alone through the oracle, on quantised rows."""
    from oracle import easykv_oracle as O
    from tests.test_hip_fullsize import Probe
    Hq, H, D = cases.LOCK_SHAPE
    P, Bud, G0 = cases.LOCK["prompts"], cases.LOCK["budgets"], cases.LOCK["scored"]
    probe = Probe()
    O.SELECT_HOOK = probe
    n_dec = n_stable = 0
    try:
        for s in range(4):
            e, toks = cases.lockstep_inputs(s)
            last = cases.LOCK_RETIRE[1] if s == cases.LOCK_RETIRE[0] else cases.LOCK_STEPS - 1
            st = O.LayerState(k=_deq(e["k0"]).unsqueeze(0), v=_deq(e["v0"]).unsqueeze(0))
            st.s, st.q, st.c = O.init_state_decoding((H,), Bud[s])
            st.s[:, :G0[s]] += e["warm"]
            st.q[:, :G0[s]] += e["warm"] ** 2
            for step in range(last + 1):
                q, k, v = toks[step]
                evict = cases.lockstep_evicts(s, step)
                _, ids = O.layer_step(st, q.float(), _deq(k), _deq(v), O.StepPlan(policy="roco", phase="decode", evict=evict, score_off=P[s], budget=Bud[s]))
                if evict:
                    assert ids is not None
                    n_dec += H
                    n_stable += int((~probe.last_unstable).sum())
    finally:
        O.SELECT_HOOK = None
    assert n_dec == H * ((32 - 10) + (32 - 6) + (16 - 4) + (32 - 30))
    print(f"[kv6-batch-precondition] lockstep: {n_stable} of {n_dec} decisions well defined")
    assert n_stable >= 0.9 * n_dec, (n_stable, n_dec)


# ---- 7. the engine's argument errors that need no GPU ------------------------------------------------------------------------------------
def test_kvbank_kv_quant_errors_come_before_any_device_access():
    from easykv_amd import KVBank, KVBankBatch
    from easykv_amd._lib import EkvError
    for make in (lambda **kw: KVBank(2, 4, 4, 128, 64, **kw), lambda **kw: KVBankBatch(2, 2, 4, 4, 128, 64, **kw)):
        with pytest.raises(ValueError, match=r"must be None or 'fp8' / 'mxfp4', not 'int4'; 'mxfp6' is accepted as well"):
            make(kv_quant="int4")
        with pytest.raises(ValueError, match=r"must be None or 'fp8'"):
            make(kv_quant="MXFP6")
    with pytest.raises(EkvError, match=r"quantize_mxfp6\(\): MXFP6 rows are built for head_dim 128, not 64"):
        KVBank(2, 4, 4, 64, 64, kv_quant="mxfp6")
    with pytest.raises(EkvError, match=r"quantize_mxfp6\(\): MXFP6 rows are built for GQA factors up to 4, not 8"):
        KVBankBatch(2, 2, 16, 2, 128, 64, kv_quant="mxfp6")
    with pytest.raises(EkvError, match="FP8 rows are built for head_dim 64 and 128"):      # (fp8's own refusal is unchanged)
        KVBank(2, 4, 4, 96, 64, kv_quant="fp8")
