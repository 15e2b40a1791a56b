"""Waves per workgroup and phase-order word the one-launch decode step is planned with, on a CPU: dry runs, no GPU.

tests/plan_rounds_main.cpp, built as its own program with -fsanitize=address,undefined (the sanitizer runtimes are linked into the
program; nothing is loaded into Python), plans a decode step of 32 .. 2000 heads (1 .. 50 layers of 32 or 40 heads) for every step kind and checks what holds under any
setting (the low bits of the word are the ekv_step_info field, bits 24-31 are zero, rule source 3 only on 8 waves, the threshold
packing).  The planner reads its knobs once per process, so the program runs once per setting and this file checks its lines:

  * a launch of 256 .. 512 heads runs 8-wave workgroups in order F in every mode; with the two-round launch off (EKV_FUSED_ROUNDS = 0)
    every other launch runs 4-wave ones.  ROUNDS_DEFAULT is the compile-time default, on because the two-round launch was measured
    faster;
  * with the two-round launch on (EKV_FUSED_ROUNDS = 1), launches of 1024 heads or more run on 8 waves exactly where the step runs the instance
    that has both orders and fits two per CU — head_dim 128, one query head per KV head, 16-bit rows, plain keys, slot-indexed rows, a
    scored policy, at most 2304 rows — with rule source 3 and the measured threshold, and every other kind of step keeps 4 waves;
  * EKV_FUSED_NW = 4 | 8 overrides the wave count, EKV_FUSED_ORDER the mode and EKV_FUSED_ORDER_RULE the rule."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMPILERS = [c for c in ("g++", "/opt/rocm/llvm/bin/clang++") if shutil.which(c)]
KNOBS = ("EKV_RESIDENT_MB", "EKV_RESIDENT_ROWS", "EKV_FUSED_ORDER", "EKV_FUSED_ORDER_RULE", "EKV_FUSED_NW", "EKV_FUSED_ROUNDS")
ROUNDS_DEFAULT = 1                                                 # EKV_FUSED_ROUNDS_DEFAULT of ekv_plan.cpp
BOTH_ORDERS = ("roco", "h2o", "tova", "heads40", "cols12")      # kinds that run the 8-wave instance with both phase orders
FOUR_WAVE_ORDERS = ("roco", "h2o", "tova", "heads40", "cap")           # ... the 4-wave one (at most 2304 rows)
OTHER = ("gqa", "d64", "rope", "ordered", "kv8", "batch", "sink")
MIN_HEADS = 1024                                                   # EKV_FUSED_ROUNDS_MIN_HEADS: two full rounds on 256 CUs
THRESHOLD = 0                                                      # EKV_FUSED_ROUNDS_THRESHOLD of ekv_plan.cpp: every workgroup in order K
ROUND_RULE = (3 << 4) | (1 << 6) | ((THRESHOLD // 8 >> 4) << 8) | ((THRESHOLD // 8 & 15) << 12)      # source 3, invert, the threshold
SLOT_RULE = (0 << 4) | (1 << 6) | (2 << 8) | (2 << 12)                                     # the 4-wave rule: hardware slots 2 and 3


@pytest.fixture(scope="module", params=COMPILERS or [None], ids=lambda c: os.path.basename(c) if c else "none")
def program(request, tmp_path_factory):
    if request.param is None:
        pytest.skip("no host C++ compiler on this machine")
    exe = str(tmp_path_factory.mktemp("plan_rounds") / "plan_rounds_main")
    static = ["-static-libasan", "-static-libubsan"] if os.path.basename(request.param) == "g++" else []
    cmd = [request.param, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", *static,
           "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", os.path.join(ROOT, "tests", "plan_rounds_main.cpp"),
           os.path.join(ROOT, "easykv_amd", "csrc", "ekv_plan.cpp"), "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]

    def run(**knobs):
        """{(kind, heads): (waves, rule word without the resident rows, info field)} of the planned one-launch steps"""
        env = {k: v for k, v in os.environ.items() if k not in KNOBS}
        env.update({k: str(v) for k, v in knobs.items()})
        r = subprocess.run([exe], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
        assert r.returncode == 0, (knobs, r.returncode, r.stdout[-2000:], r.stderr[-4000:])      # a failed check or a sanitizer report
        lines = r.stdout.splitlines()
        assert lines[-1].startswith("OK "), lines[-1]
        got = {}
        for ln in lines:
            if ln.startswith("W "):
                kind, heads, rc, one, nw, word, info9 = ln.split()[1:]
                if kind in ("unscored", "wide"):      # (refused on slot-indexed rows / wider than the one-launch step: nothing planned)
                    assert (int(rc), int(one)) == (-2, 0), ln
                    continue
                assert (int(rc), int(one)) == (0, 1), ln
                got[kind, int(heads)] = (int(nw), int(word) & 0xFFFF, int(info9))
        assert {k for k, _ in got} == set(BOTH_ORDERS) | set(OTHER) | {"cap"}
        return got
    return run


def _expect(got, rounds, mode, force_nw=0, rule8=ROUND_RULE, rule_given=False):
    for (kind, heads), (nw, word, info9) in got.items():
        what = (kind, heads, nw, hex(word))
        one_round = 256 <= heads <= 512
        two_rounds = rounds and kind in BOTH_ORDERS and kind != "cols12" and heads >= MIN_HEADS      # (the 5-column build: at most 2304 rows)
        assert nw == (force_nw or (8 if one_round or two_rounds else 4)), what
        assert info9 == word & 3, what
        if kind in OTHER or mode == 0:
            want = 0
        elif nw == 8:
            if one_round or kind == "cap":
                want = 0                                     # one round of one or two workgroups per CU, and the soft-capped 8-wave instances: order F in every mode
            elif mode == 2:
                want = 2
            else:
                want = (1 | rule8) if heads > 512 or rule_given else 0
        else:
            want = 0 if kind not in FOUR_WAVE_ORDERS else (2 if mode == 2 else ((1 | SLOT_RULE) if heads >= 512 else 0))
        assert word == want, what + (hex(want),)


def test_default_wave_counts_and_orders(program):
    _expect(program(), ROUNDS_DEFAULT, 1)
    for mode in (0, 1, 2):
        _expect(program(EKV_FUSED_ORDER=mode), ROUNDS_DEFAULT, mode)


def test_two_round_launch(program):
    got = program(EKV_FUSED_ROUNDS=1)
    _expect(got, 1, 1)
    assert got["roco", 1024] == (8, 1 | ROUND_RULE, 1) and got["roco", 512] == (8, 0, 0) and got["roco", 224] == (4, 0, 0)
    assert got["roco", 576] == (4, 1 | SLOT_RULE, 1) and got["roco", 1600] == (8, 1 | ROUND_RULE, 1)
    assert got["cols12", 1024] == (4, 0, 0) and got["kv8", 1024] == (4, 0, 0) and got["gqa", 1024] == (4, 0, 0)
    for mode in (0, 2):
        _expect(program(EKV_FUSED_ROUNDS=1, EKV_FUSED_ORDER=mode), 1, mode)
    _expect(program(EKV_FUSED_ROUNDS=0), 0, 1)


def test_wave_count_override(program):
    for rounds in (0, 1):
        _expect(program(EKV_FUSED_NW=4, EKV_FUSED_ROUNDS=rounds), rounds, 1, force_nw=4)
        for mode in (0, 1, 2):
            _expect(program(EKV_FUSED_NW=8, EKV_FUSED_ROUNDS=rounds, EKV_FUSED_ORDER=mode), rounds, mode, force_nw=8)
    got = program(EKV_FUSED_NW=8)
    assert got["roco", 1024] == (8, 1 | ROUND_RULE, 1) and got["roco", 32] == (8, 0, 0) and got["roco", 256] == (8, 0, 0)


def test_rule_override(program):
    # threshold 128 workgroups (mask nibble 1, bound nibble 0, units of 8), order K at or past it
    rule = (3 << 4) | (1 << 6) | (1 << 8) | (0 << 12)
    got = program(EKV_FUSED_NW=8, EKV_FUSED_ORDER_RULE="3,1,0,1")
    _expect(got, 0, 1, force_nw=8, rule8=rule, rule_given=True)
    assert got["roco", 32] == (8, 1 | rule, 1) and got["roco", 512] == (8, 0, 0)
    # a 4-wave launch ignores a rule that names source 3 (only the 8-wave instances read it) and keeps its slot rule
    got = program(EKV_FUSED_NW=4, EKV_FUSED_ORDER_RULE="3,1,0,1")
    assert got["roco", 1024] == (4, 1 | SLOT_RULE, 1) and got["roco", 576] == (4, 1 | SLOT_RULE, 1) and got["roco", 224] == (4, 0, 0)
