"""The planned resident rows of the one-launch decode step (include/easykv_hip.h, "resident rows"), on a CPU: dry runs, no GPU.

1. tests/plan_resident_main.cpp, built as its own program with -fsanitize=address,undefined (the sanitizer runtimes are linked into the
   program; nothing is loaded into Python), sweeps heads x extents x budgets through the byte rule and through the plan of a
   slot-indexed decode step, and checks there what the rule promises; this file checks the program's lines again with its own
   arithmetic: a multiple of 32, resident bytes within the budget, 32 more rows would exceed the budget or the rounded extent,
   budget 0 -> 0, everything fits -> the rounded extent, the planned value is the rule's, the ten ekv_step_info fields do not depend
   on the budget.
2. The library answers the same through its exports (ekv_set_resident_bytes, ekv_step_resident_rows, EKV_RESIDENT_MB and
   EKV_RESIDENT_ROWS in the environment, read once: child processes), only the instances that have resident rows plan any, and
   ekv_step_info answers every case exactly as the library did before the resident rows existed (PARENT_INFO: recorded from it)."""
import json
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMPILERS = [c for c in ("g++", "/opt/rocm/llvm/bin/clang++") if shutil.which(c)]
KNOBS = ("EKV_RESIDENT_MB", "EKV_RESIDENT_ROWS", "EKV_FUSED_ORDER", "EKV_FUSED_ORDER_RULE", "EKV_FUSED_NW")
MB = 1 << 20
HEADS, EXTENTS, BUDGETS = (32, 512, 544, 1024, 1600), (1, 31, 32, 328, 2049, 2304, 6144), (0, 1 * MB, 64 * MB, 220 * MB, 1 << 40)


def _bytes(heads, cap, score_rows, rows, row_bytes=256):
    """K + V of `rows` rows of every head, plus what a head re-reads every step anyway: the score rows, the slot map, the birth row."""
    return heads * (2 * rows * row_bytes + 4 * cap * (score_rows + 2))


def _rule(heads, ext, cap, score_rows, budget):
    ext32 = (ext + 31) // 32 * 32
    rows = ext32
    while rows > 0 and _bytes(heads, cap, score_rows, rows) > budget:
        rows -= 32
    return rows if _bytes(heads, cap, score_rows, rows) <= budget else 0


@pytest.fixture(scope="module", params=COMPILERS or [None], ids=lambda c: os.path.basename(c) if c else "none")
def program_lines(request, tmp_path_factory):
    if request.param is None:
        pytest.skip("no host C++ compiler on this machine")
    exe = str(tmp_path_factory.mktemp("plan_resident") / "plan_resident_main")
    static = ["-static-libasan", "-static-libubsan"] if os.path.basename(request.param) == "g++" else []
    cmd = [request.param, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", *static,
           "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", os.path.join(ROOT, "tests", "plan_resident_main.cpp"),
           os.path.join(ROOT, "easykv_amd", "csrc", "ekv_plan.cpp"), "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    env = {k: v for k, v in os.environ.items() if k not in KNOBS}
    r = subprocess.run([exe], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])      # a failed check or a sanitizer report: non-zero status
    lines = r.stdout.splitlines()
    assert lines[-1].startswith("OK "), lines[-1]
    return lines


def test_rule_under_sanitizers(program_lines):
    rule = [tuple(int(x) for x in ln.split()[1:]) for ln in program_lines if ln.startswith("F ")]
    assert len(rule) == len(HEADS) * len(EXTENTS) * 2 * len(BUDGETS)
    assert {(h, e, b) for h, e, _, _, b, _ in rule} == {(h, e, b) for h in HEADS for e in EXTENTS for b in BUDGETS}
    for heads, ext, cap, score_rows, budget, rows in rule:
        ext32 = (ext + 31) // 32 * 32
        what = (heads, ext, cap, score_rows, budget, rows)
        assert rows % 32 == 0 and 0 <= rows <= ext32, what
        assert rows == 0 or _bytes(heads, cap, score_rows, rows) <= budget, what
        assert rows == ext32 or _bytes(heads, cap, score_rows, rows + 32) > budget, what
        assert budget != 0 or rows == 0, what
        assert _bytes(heads, cap, score_rows, ext32) > budget or rows == ext32, what
        assert rows == _rule(heads, ext, cap, score_rows, budget), what
    # the flagship launch: 1024 heads x 2049 rows under 220 MiB keeps 352 rows of every head (K + V: 184.5 MB of 1.07 GB)
    assert (1024, 2049, 2112, 3, 220 * MB, 352) in rule


def test_planned_value_under_sanitizers(program_lines):
    plans = [tuple(int(x) for x in ln.split()[1:]) for ln in program_lines if ln.startswith("P ")]
    assert len(plans) == len(HEADS) * len(EXTENTS) * len(BUDGETS)
    info0, n_fused, n_resident = {}, 0, 0
    for heads, ext, budget, rows, fused, *info in plans:
        assert len(info) == 10
        cap = (ext + 63 + 63) // 64 * 64
        if budget == 0:
            info0[heads, ext] = info
        assert info == info0[heads, ext], (heads, ext, budget)      # (the program walks the budgets from 0 up)
        assert rows == (_rule(heads, ext, cap, 3, budget) if fused else 0), (heads, ext, budget, rows, fused)
        assert fused == (info[1] == 1 and info[8] == 1), (heads, ext, info)
        n_fused += fused
        n_resident += rows > 0
    assert n_fused >= len(BUDGETS) * 20 and n_resident >= 40, (n_fused, n_resident)
    got = {(h, e, b): r for h, e, b, r, *_ in plans}
    assert got[1024, 2049, 220 * MB] == 352 and got[1024, 2049, 1 << 40] == 2080 and got[544, 328, 64 * MB] == 192 and got[544, 328, 220 * MB] == 352 and got[32, 31, MB] == 32


# ---- the library's exports -----------------------------------------------------------------------------------------------------------
# ekv_step_info of the cases below as the library answered before the resident rows existed: return code, then the ten fields
PARENT_INFO = {"bench": [0, 1, 1, 0, 0, 1, 1, 2, 0, 1, 1], "layers18": [0, 1, 1, 0, 0, 1, 1, 2, 0, 1, 1], "h2o": [0, 1, 1, 0, 0, 1, 1, 2, 0, 1, 1],
               "tova": [0, 1, 1, 0, 0, 1, 1, 2, 0, 1, 1], "ordered_rows": [0, 1, 1, 0, 0, 1, 1, 2, 0, 1, 0],
               "eight_waves": [0, 1, 1, 0, 0, 1, 1, 2, 0, 1, 0], "few_heads": [0, 1, 1, 0, 0, 1, 1, 2, 0, 1, 0], "gqa": [0, 1, 1, 0, 0, 1, 1, 2, 0, 1, 0],
               "d64": [0, 1, 1, 0, 0, 1, 1, 2, 0, 1, 0], "long_rows": [0, 1, 1, 0, 0, 1, 1, 2, 0, 1, 0], "rope": [0, 1, 1, 0, 0, 1, 1, 2, 0, 1, 0],
               "split": [0, 6, 0, 0, 0, 1, 1, 2, 0, 2, 0], "chunk": [0, 1, 1, 0, 0, 1, 8, 2, 1, 1, 0]}
# (heads, extent, cap, score rows) of the cases whose instance has resident rows; every other case plans 0
RESIDENT = {"bench": (1024, 2112, 2112, 3), "layers18": (576, 2112, 2112, 3), "h2o": (1024, 2112, 2112, 1), "tova": (1024, 2112, 2112, 1),
            "eight_waves": (512, 2112, 2112, 3), "few_heads": (128, 2112, 2112, 3), "long_rows": (1024, 3008, 3008, 3)}

CHILD = r"""
import ctypes, json, sys
from tests.test_dispatch_table import _case, _structs
from easykv_amd import _lib
lib = _lib.load()
slot = dict(phases=16, phys_extent=2112, n_split=1)
cases = dict(
    bench=dict(n_layers=32, **slot), layers18=dict(n_layers=18, **slot), h2o=dict(n_layers=32, policy=1, win_tail=100, **slot),
    tova=dict(n_layers=32, policy=3, **slot),
    ordered_rows=dict(n_layers=32, phys_extent=2112, n_split=1), eight_waves=dict(n_layers=16, **slot), few_heads=dict(n_layers=4, **slot),
    gqa=dict(n_layers=32, hq=32, h=16, **slot), d64=dict(n_layers=32, head_dim=64, **slot),
    long_rows=dict(n_layers=32, phases=16, n_split=1, n_slots=3000, cap=3008, phys_extent=3008, roco_k1=2100),
    rope=dict(n_layers=32, rope_on_read=1, n_split=1), split=dict(n_layers=1), chunk=dict(n_layers=32, q_len=8, n_evict=8, n_slots=2056, roco_k1=1000))
out = {}
for budget in json.loads(sys.argv[1]):
    if budget is not None:
        assert lib.ekv_set_resident_bytes(budget) == 0
    for name, kw in cases.items():
        bank, st = _structs(_case(**kw))
        info = (ctypes.c_int32 * 10)()
        rc = lib.ekv_step_info(ctypes.byref(bank), ctypes.byref(st), info, 10)
        rows = [lib.ekv_step_resident_rows(ctypes.byref(bank), ctypes.byref(st), dt) for dt in (0, 1)]
        out.setdefault(str(budget), {})[name] = [[rc] + list(info), rows]
out["errors"] = [lib.ekv_step_resident_rows(None, None, 0), lib.ekv_step_resident_rows(ctypes.byref(bank), ctypes.byref(st), 7)]
print(json.dumps(out))
"""


def _ask(budgets, **knobs):
    from easykv_amd import _build
    if not os.path.exists(_build.LIB):
        _build.build_lib()
    env = {k: v for k, v in os.environ.items() if k not in KNOBS}
    env.update({k: str(v) for k, v in knobs.items()})
    r = subprocess.run([sys.executable, "-c", CHILD, json.dumps(budgets)], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.splitlines()[-1])


def _check(got, budget, forced=None):
    for name, (info, rows) in got.items():
        assert info == PARENT_INFO[name], (name, budget, info)
        if name in RESIDENT:
            heads, ext, cap, score_rows = RESIDENT[name]
            want = _rule(heads, ext, cap, score_rows, budget) if forced is None else min(forced // 32 * 32, (ext + 31) // 32 * 32)
        else:
            want = 0
        assert rows == [want, want], (name, budget, rows, want)      # (fp16 and bf16 plan alike)


def test_library_plans_the_rule_and_step_info_is_the_parents():
    budgets = [0, MB, 64 * MB, 220 * MB, 1 << 40]
    got = _ask(budgets)
    assert got.pop("errors") == [-1, -1]
    for b in budgets:
        _check(got[str(b)], b)
    assert got[str(220 * MB)]["bench"][1] == [352, 352] and got[str(1 << 40)]["few_heads"][1] == [2112, 2112]


def test_environment_knobs():
    # EKV_RESIDENT_MB is the budget until the setter sets one; a negative value returns to it
    got = _ask([None, 64 * MB, -1], EKV_RESIDENT_MB=220)
    got.pop("errors")
    _check(got["None"], 220 * MB)
    _check(got[str(64 * MB)], 64 * MB)
    _check(got["-1"], 220 * MB)
    _check(_ask([None], EKV_RESIDENT_MB=0)["None"], 0)
    # EKV_RESIDENT_ROWS replaces the byte rule (capped at the rounded extent) under any budget but 0: a caller that switched the
    # resident rows off keeps them off
    for forced in (0, 96, 100, 100000):
        got = _ask([None, 1, 0], EKV_RESIDENT_ROWS=forced, EKV_RESIDENT_MB=64)
        _check(got["None"], None, forced)
        _check(got["1"], None, forced)
        _check(got["0"], 0)
