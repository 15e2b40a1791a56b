"""The step planner (easykv_amd/csrc/ekv_plan.cpp) as a stand-alone host program under AddressSanitizer + UBSan, on a CPU.

tests/plan_host_main.cpp links ekv_plan.cpp and nothing else of the library; it is built here with the host compiler and
-fsanitize=address,undefined -fno-sanitize-recover=undefined (the runtimes linked in; nothing is loaded into Python) and run as a child process.
  (a) the whole grid of tests/test_dispatch_table.py equals tests/golden/dispatch/dispatch_table.npz, one process per switch setting;
  (b) the uniform and ragged tables of tests/test_batch_cpu.py and the kv8 grid of tests/test_kv8_cpu.py give what the library gives;
  (c) 50 000 seeded arbitrary descriptors (int32 fields negative / 0 / 1 / typical / near INT32_MAX, null pointers, n_seq -1 .. 65) end
      without a sanitizer report and with the library's answers;
  (d) the geometry predicates over their sweep equal tests/golden/dispatch/predicates.npz, recorded from the library before the planner
      and the geometry header were split off (this pins the LDS byte counts, which no GPU test can check safely).
A sanitizer report ends the program with a non-zero status, which fails the test that ran it."""
import ctypes
import itertools
import os
import shutil
import subprocess
import time

import numpy as np
import pytest

from tests.test_batch_cpu import _policy_kw
from tests.test_dispatch_table import ENVS, KEYS, SWITCHES, _case, cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "dispatch")
COMPILERS = [c for c in ("g++", "/opt/rocm/llvm/bin/clang++") if shutil.which(c)]
SEQ_KEYS = ("layer", "n_slots", "score_off", "n_evict", "win_lo", "win_tail", "roco_k1", "range_start", "phys_extent")
I32_MAX = 2 ** 31 - 1
SPECIAL = (-2 ** 31, -7, -1, 0, 1, I32_MAX, I32_MAX - 1, I32_MAX - 63)


@pytest.fixture(scope="module", params=COMPILERS or [None], ids=lambda c: os.path.basename(c) if c else "none")
def program(request, tmp_path_factory):
    if request.param is None:
        pytest.skip("no host C++ compiler on this machine")
    exe = str(tmp_path_factory.mktemp("plan_host") / "plan_host_main")
    # (the sanitizer runtimes linked into the program — clang++'s default: the program then starts whatever else the process environment loads)
    static = ["-static-libasan", "-static-libubsan"] if os.path.basename(request.param) == "g++" else []
    cmd = [request.param, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", *static,
           "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", os.path.join(ROOT, "tests", "plan_host_main.cpp"),
           os.path.join(ROOT, "easykv_amd", "csrc", "ekv_plan.cpp"), "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    return exe


def _run(exe, lines=None, args=(), switches=None):
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env.update(switches or {})
    r = subprocess.run([exe, *args], input="\n".join(lines or []) + "\n", env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-4000:])
    return r.stdout


def _u64(rows):
    """Rows of answers as uint64 (two's complement): a refused step's workspace bytes may be any size_t."""
    return np.array([[int(x) & (2 ** 64 - 1) for x in row] for row in rows], dtype=np.uint64)


def _answers(exe, lines, switches=None):
    out = _u64(ln.split() for ln in _run(exe, lines, switches=switches).splitlines())
    assert out.shape == (len(lines), 16), out.shape
    return out


def _line(c, dtype=0, kv8=0, nulls=0, seqs=None, n_seq=None):
    """A case of tests/test_dispatch_table.py (+ the call's variant) as the program reads it."""
    v = [c[k] for k in KEYS] + [dtype, kv8, nulls, int(seqs is not None), (len(seqs) if n_seq is None else n_seq) if seqs is not None else 0]
    for e in seqs or []:
        v += [e[k] for k in SEQ_KEYS]
    return " ".join(str(int(x)) for x in v)


@pytest.fixture(scope="module")
def lib():
    from easykv_amd import _build, _lib
    if not os.path.exists(_build.LIB):
        _build.build_lib()
    return _lib, _lib.load()


def _library(L, lib, c, dtype=0, kv8=0, nulls=0, seqs=None, n_seq=None):
    """The same call through the C ABI of the library: the row the program prints."""
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
    info = (ctypes.c_int32 * 10)(*([-7] * 10))
    plan = [-7, -7, -7]
    if seqs is not None:
        n = len(seqs) if n_seq is None else n_seq
        tb = (L.Seq * max(len(seqs), 1))()
        for i, e in enumerate(seqs):
            for k in SEQ_KEYS:
                setattr(tb[i], k, e[k])
        t = None if nulls & 128 else tb
        rc = [lib.ekv_batch_step_check(b, s, dtype, t, n), lib.ekv_batch_step_info(b, s, dtype, t, n, info, 10), lib.ekv_batch_workspace_bytes(b, s, dtype, t, n)]
    elif kv8:
        q8 = L.Kv8(256, 256, p(not nulls & 64), 256)
        q = None if nulls & 32 else ctypes.byref(q8)
        rc = [lib.ekv_kv8_step_check(b, s, dtype, q), lib.ekv_kv8_step_info(b, s, dtype, q, info, 10), lib.ekv_kv8_workspace_bytes(b, s, dtype, q)]
    else:
        rc = [lib.ekv_step_check_typed(b, s, dtype), lib.ekv_step_info_typed(b, s, dtype, info, 10), lib.ekv_workspace_bytes_typed(b, s, dtype)]
        if dtype == 0:
            ns, fu = ctypes.c_int32(-7), ctypes.c_int32(-7)
            plan = [lib.ekv_step_plan(b, s, ctypes.byref(ns), ctypes.byref(fu)), ns.value, fu.value]
    return [rc[0]] + plan + [rc[1]] + list(info) + [rc[2]]


def _same(L, lib, exe, calls):
    got = _answers(exe, [_line(*a, **kw) for a, kw in calls])
    want = _u64(_library(L, lib, *a, **kw) for a, kw in calls)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert len(bad) == 0, [(calls[i], want[i].tolist(), got[i].tolist()) for i in bad[:3]]


@pytest.mark.parametrize("name", list(ENVS))
def test_dispatch_grid_equals_the_golden_table(program, name):
    golden = np.load(os.path.join(GOLDEN, "dispatch_table.npz"))
    cs = cases()
    got = _answers(program, [_line(c) for c in cs], switches=ENVS[name])
    got = np.concatenate([got[:, :14], got[:, 15:]], axis=1)      # (the table holds the first 9 info fields)
    want = _u64(golden[name].tolist())
    assert got.shape == want.shape
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert len(bad) == 0, [(int(i), cs[i], want[i].tolist(), got[i].tolist()) for i in bad[:5]]


def _batch_calls():
    """The uniform and the ragged tables of tests/test_batch_cpu.py::test_batch_plans_as_the_step_of_its_envelope."""
    calls = []
    for d, (hq, h), n_seq, T, policy in itertools.product((32, 64, 96, 128), ((32, 32), (32, 8), (8, 2), (24, 8)), (1, 2, 8, 33),
                                                          (5, 300, 2049, 5002), (0, 1, 2, 3, 4)):
        cap = (T + 64 + 63) // 64 * 64
        c = _case(head_dim=d, hq=hq, h=h, n_layers=40, cap=cap, layer_begin=0, layer_count=n_seq, n_slots=T, **_policy_kw(policy, T))
        uniform = [dict(layer=(7 * i + 3) % 40, **{k: c[k] for k in SEQ_KEYS[1:]}) for i in range(n_seq)]
        entries = []
        if n_seq > 1:
            lens = [max(1, T * (i + 1) // n_seq - (i % 3)) for i in range(n_seq)]
            lens[n_seq // 2], lens[0] = T, min(lens[0], 2)
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
        for dt in (0, 1):
            calls.append(((c,), dict(dtype=dt, seqs=uniform)))
            if entries:
                calls.append(((c,), dict(dtype=dt, seqs=entries)))
    return calls


def test_batch_tables_and_kv8_grid_answer_as_the_library(program, lib):
    L, so = lib
    calls = _batch_calls()
    assert len(calls) == 2 * 4 * 4 * 4 * 4 * 5 + 2 * 4 * 4 * 3 * 4 * 5
    calls += [((c,), dict(dtype=dt, kv8=1)) for c in cases() for dt in (0, 1)]
    _same(L, so, program, calls)


def _arbitrary_calls(n=50000, seed=20261018):
    rs = np.random.RandomState(seed)
    typical = cases()
    calls = []
    for _ in range(n):
        c = dict(typical[rs.randint(len(typical))])
        p_field = (0.01, 0.03, 0.1, 0.3)[rs.randint(4)]      # (a few odd fields reach the later stages, many exercise the early ones)
        for k in KEYS:      # every int32 field of bank and step (the four pointer flags stay flags)
            if k not in ("arrive", "birth", "score_sum", "score_sq", "count_add2") and rs.rand() < p_field:
                c[k] = SPECIAL[rs.randint(len(SPECIAL))]
        kw = dict(dtype=int(rs.choice([0, 0, 0, 1, 1, 2, -1])), kv8=int(rs.rand() < 0.25))
        kw["nulls"] = int(sum(bit for bit in (1, 2, 4, 8, 16, 32, 64, 128) if rs.rand() < 0.02))
        if rs.rand() < 0.4:
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


def test_arbitrary_descriptors_end_clean_and_answer_as_the_library(program, lib):
    L, so = lib
    calls = _arbitrary_calls()
    t0 = time.time()
    _same(L, so, program, calls)
    print(f"sweep of {len(calls)} descriptors: {time.time() - t0:.1f} s")


def test_predicates_equal_the_recorded_table(program):
    golden = np.load(os.path.join(GOLDEN, "predicates.npz"))
    got = {}
    for ln in _run(program, args=("--predicates",)).splitlines():
        w = ln.split()
        got[w[0]] = np.array(w[2:], dtype=np.int64)
        assert len(got[w[0]]) == int(w[1])
    assert sorted(got) == sorted(golden.files)
    for name in golden.files:
        assert np.array_equal(got[name], golden[name].astype(np.int64)), name
