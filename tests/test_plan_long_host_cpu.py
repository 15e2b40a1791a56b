"""The long-row call family of the step planner (easykv_amd/csrc/ekv_plan.cpp) as a stand-alone host program under AddressSanitizer +
UBSan, on a CPU.

tests/plan_long_host_main.cpp links ekv_plan.cpp and nothing else of the library; it is built here exactly as tests/test_plan_host_cpu.py
builds its program (host compiler, -fsanitize=address,undefined -fno-sanitize-recover=undefined, the runtimes linked in; nothing is
loaded into Python) and run as a child process.  The grid of tests/test_dispatch_table.py in both element types, and 50 000 seeded
arbitrary descriptors (int32 fields negative / 0 / 1 / typical / near INT32_MAX, null pointers), go through ekv_long_step_check,
ekv_long_step_info and ekv_long_workspace_bytes: the program's answers equal the library's, and a sanitizer report ends the program with
a non-zero status, which fails the test that ran it."""
import ctypes
import os
import shutil
import subprocess
import time

import numpy as np
import pytest

from tests.test_dispatch_table import KEYS, STEP_KEYS, SWITCHES, named_cases, random_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMPILERS = [c for c in ("g++", "/opt/rocm/llvm/bin/clang++") if shutil.which(c)]
I32_MAX = 2 ** 31 - 1
SPECIAL = (-2 ** 31, -7, -1, 0, 1, I32_MAX, I32_MAX - 1, I32_MAX - 63)


@pytest.fixture(scope="module", params=COMPILERS or [None], ids=lambda c: os.path.basename(c) if c else "none")
def program(request, tmp_path_factory):
    if request.param is None:
        pytest.skip("no host C++ compiler on this machine")
    exe = str(tmp_path_factory.mktemp("plan_long_host") / "plan_long_host_main")
    # (the sanitizer runtimes linked into the program — clang++'s default: the program then starts whatever else the process environment loads)
    static = ["-static-libasan", "-static-libubsan"] if os.path.basename(request.param) == "g++" else []
    cmd = [request.param, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", *static,
           "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", os.path.join(ROOT, "tests", "plan_long_host_main.cpp"),
           os.path.join(ROOT, "easykv_amd", "csrc", "ekv_plan.cpp"), "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    return exe


@pytest.fixture(scope="module")
def lib():
    from easykv_amd import _build, _lib
    if not os.path.exists(_build.LIB):
        _build.build_lib()
    return _lib.load()


def _u64(rows):
    return np.array([[int(x) & (2 ** 64 - 1) for x in row] for row in rows], dtype=np.uint64)


def _program(exe, calls):
    lines = [" ".join(str(int(x)) for x in [c[k] for k in KEYS] + [dtype, nulls]) for c, dtype, nulls in calls]
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    r = subprocess.run([exe], input="\n".join(lines) + "\n", env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-4000:])
    out = _u64(ln.split() for ln in r.stdout.splitlines())
    assert out.shape == (len(calls), 15), out.shape
    return out


def _library(lib, c, dtype, nulls):
    """The same call through the C ABI of the library: the row the program prints."""
    from easykv_amd._lib import Bank, Step
    p = lambda on: 256 if on else None      # (dummy non-null pointers: nothing is dereferenced)
    bank = Bank(p(not nulls & 4), p(not nulls & 8), p(not nulls & 16), p(c["score_sum"]), p(c["score_sq"]), p(c["score_sq"]), c["n_layers"],
                c["hq"], c["h"], c["head_dim"], c["cap"], p(c["arrive"]), p(c["birth"]), p(c["birth"]))
    st = Step()
    for k in STEP_KEYS:
        if k != "count_add2":
            setattr(st, k, c[k])
    st.count_add, st.count_tail_step, st.sm_div = c["count_add2"] / 2, -1.0 if c["q_len"] > 1 else 0.0, 1.0
    b = None if nulls & 1 else ctypes.byref(bank)
    s = None if nulls & 2 else ctypes.byref(st)
    info = (ctypes.c_int32 * 12)(*([-7] * 12))
    check = lib.ekv_long_step_check(b, s, dtype)
    irc = lib.ekv_long_step_info(b, s, dtype, None if nulls & 32 else info, 0 if nulls & 64 else 12)
    return [check, irc] + list(info) + [lib.ekv_long_workspace_bytes(b, s, dtype)]


def _same(lib, exe, calls):
    got = _program(exe, calls)
    want = _u64(_library(lib, *call) for call in calls)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert len(bad) == 0, [(calls[i], want[i].tolist(), got[i].tolist()) for i in bad[:3]]
    return got


def test_long_grid_answers_as_the_library(program, lib):
    calls = [(c, dtype, 0) for c in named_cases() + random_cases() for dtype in (0, 1)]
    got = _same(lib, program, calls)
    assert (got[:, 12] == 1).sum() > 100      # (steps that end in the long-row scorer are part of the grid)


def _arbitrary_calls(n=50000, seed=20261020):
    rs = np.random.RandomState(seed)
    typical = named_cases() + random_cases()
    calls = []
    for _ in range(n):
        c = dict(typical[rs.randint(len(typical))])
        p_field = (0.01, 0.03, 0.1, 0.3)[rs.randint(4)]      # (a few odd fields reach the later stages, many exercise the early ones)
        for k in KEYS:      # every int32 field of bank and step (the four pointer flags stay flags)
            if k not in ("arrive", "birth", "score_sum", "score_sq", "count_add2") and rs.rand() < p_field:
                c[k] = SPECIAL[rs.randint(len(SPECIAL))]
        if rs.rand() < 0.15:      # wide rows, where the two families part: up to and beyond 16-bit indices
            c["n_slots"] = int(rs.choice([38391, 38393, 40000, 65535, 65536, 65537, 131073]))
            c["cap"] = (c["n_slots"] + 63) // 64 * 64 + 64 * int(rs.randint(0, 3))
            c["n_split"] = int(rs.choice([-1, 0, 8]))
        dtype = int(rs.choice([0, 0, 0, 1, 1, 2, -1]))
        nulls = int(sum(bit for bit in (1, 2, 4, 8, 16, 32, 64) if rs.rand() < 0.02))
        calls.append((c, dtype, nulls))
    return calls


def test_arbitrary_descriptors_end_clean_and_answer_as_the_library(program, lib):
    calls = _arbitrary_calls()
    t0 = time.time()
    _same(lib, program, calls)
    print(f"sweep of {len(calls)} descriptors: {time.time() - t0:.1f} s")
