"""Batched decode steps on 16-bit-key / MXFP4-value rows (include/easykv_hip.h, "kv164 batches") on a CPU: the four calls exist, their
dry runs plan a table exactly as the 16-bit batched call plans it (a uniform table: as the kv164 multi-layer step it spells out) and
refuse what either family refuses before a launch, the planner's kv164 stages run clean as a stand-alone program under AddressSanitizer
+ UBSan (tests/plan_kv164_main.cpp) with the library's answers, and the seeded inputs of the ragged GPU cases
(tests/test_hip_batch_kv164.py) leave the oracle's decisions well defined on unquantised keys.  Dummy non-null pointers throughout:
nothing is dereferenced, nothing is launched."""
import ctypes
import itertools
import os
import re
import subprocess

import pytest
import torch

from tests import batch_kv6_cases as cases      # (the ragged tables and seeds of the kv6 batch cases, reused as tests/kv164_cases.py reuses the step cases)
from tests import kv164_cases as K
from tests.test_batch_cpu import _batch_answers, _lib, _policy_kw, _table, _uniform
from tests.test_batch_kv6_cpu import COMPILERS, SEQ_KEYS, _arbitrary_calls, _line, _ragged_entries, _u64
from tests.test_dispatch_table import SWITCHES, _case, _structs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("ekv_kv164_batch_step_check", "ekv_kv164_batch_step_info", "ekv_kv164_batch_workspace_bytes", "ekv_kv164_batch_step_attend")
F16, BF16 = 0, 1
GQA = ((32, 32), (32, 8), (24, 8), (64, 8))      # GQA x 1, x 4, x 3 (padded build), x 8


def _kv164_batch_answers(lib, bank, st, dtype, kv164, tb, n=None):
    b, s, k = ctypes.byref(bank), ctypes.byref(st), (ctypes.byref(kv164) if kv164 is not None else None)
    n = len(tb) if n is None else n
    info = (ctypes.c_int32 * 9)(*([-7] * 9))
    return [lib.ekv_kv164_batch_step_check(b, s, dtype, k, tb, n), lib.ekv_kv164_batch_step_info(b, s, dtype, k, tb, n, info, 9)] + list(info) + \
           [lib.ekv_kv164_batch_workspace_bytes(b, s, dtype, k, tb, n)]


def _kv164_step_answers(lib, bank, st, dtype, kv164):
    b, s, k = ctypes.byref(bank), ctypes.byref(st), ctypes.byref(kv164)
    info = (ctypes.c_int32 * 9)(*([-7] * 9))
    return [lib.ekv_kv164_step_check(b, s, dtype, k), lib.ekv_kv164_step_info(b, s, dtype, k, info, 9)] + list(info) + [lib.ekv_kv164_workspace_bytes(b, s, dtype, k)]


def _sweep():
    """(case, uniform entries, ragged entries or None): the tables of tests/test_batch_kv6_cpu.py at head_dim 128, over GQA x 1 .. x 8."""
    for (hq, h), n_seq, T, policy in itertools.product(GQA, (1, 2, 8, 33), (5, 300, 2049, 5002), (0, 1, 2, 3, 4)):
        cap = (T + 64 + 63) // 64 * 64
        c = _case(head_dim=128, hq=hq, h=h, n_layers=40, cap=cap, layer_begin=0, layer_count=n_seq, n_slots=T, **_policy_kw(policy, T))
        uniform = [dict(layer=(7 * i + 3) % 40, **{k: c[k] for k in SEQ_KEYS[1:]}) for i in range(n_seq)]
        yield c, uniform, (_ragged_entries(n_seq, T, policy, cap) if n_seq > 1 else None)


def test_kv164_batch_calls_are_exported_and_declared():
    L, lib = _lib()
    header = open(os.path.join(ROOT, "include", "easykv_hip.h")).read()
    declared = set(re.findall(r"\b(ekv_[a-z0-9_]+)\s*\(", header))
    raw = ctypes.CDLL(L.LIB)
    for name in CALLS:
        assert name in declared and name in L.EXPORTS and hasattr(raw, name) and hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name      # typed by load()
    assert lib.ekv_abi_version() == 8
    assert lib.ekv_kv164_batch_workspace_bytes.restype is ctypes.c_size_t and lib.ekv_kv164_batch_step_check.restype is ctypes.c_int
    assert '"kv164 batches"' in header
    assert lib.ekv_kv164_batch_step_check(None, None, F16, None, None, 1) == -1
    assert lib.ekv_kv164_batch_step_info(None, None, F16, None, None, 1, None, 0) == -1
    assert lib.ekv_kv164_batch_workspace_bytes(None, None, F16, None, None, 1) == 0
    assert lib.ekv_kv164_batch_step_attend(None, None, F16, None, None, 1, None, None, None, None, None, None, 0, None) == -1


def test_kv164_batch_plans_as_the_16_bit_batch_and_as_the_kv164_multi_layer_step():
    """Return code, the nine info fields, fused_order 0 and the workspace bytes are ekv_batch_*'s of the same table; a uniform table
    also equals ekv_kv164_step_* of the multi-layer step it spells out."""
    L, lib = _lib()
    kv164 = L.Kv164(256, 256)
    n_uniform = n_ragged = n_one_launch = n_split = n_refused = 0
    for c, uniform, ragged in _sweep():
        bank, st = _structs(c)
        for ti, entries in enumerate((uniform, ragged)):
            if entries is None:
                continue
            tb = _table(L, entries)
            for dt in (F16, BF16):
                ref = _batch_answers(lib, bank, st, dt, tb)
                got = _kv164_batch_answers(lib, bank, st, dt, kv164, tb)
                assert got == ref, (c, dt, ti, got, ref)
                if ref[0] != 0:      # (the 16-bit batch's own refusal — GQA x 8 past the one-CU score rows: the same code, nothing planned)
                    assert ref[0] == -2 and c["hq"] // c["h"] == 8, (c, ref)
                    n_refused += 1
                    continue
                info = (ctypes.c_int32 * 10)(*([-7] * 10))
                assert lib.ekv_kv164_batch_step_info(ctypes.byref(bank), ctypes.byref(st), dt, ctypes.byref(kv164), tb, len(tb), info, 10) == 0
                assert list(info)[:9] == got[2:11] and info[9] == 0, list(info)      # fused_order 0
                if ti == 0:
                    solo = _kv164_step_answers(lib, bank, st, dt, kv164)
                    assert solo == got, (c, dt, solo, got)
                n_uniform += ti == 0
                n_ragged += ti == 1
                n_one_launch += got[3] == 1
                n_split += got[2] > 1
    assert n_uniform + n_ragged + n_refused == 2 * 4 * 4 * 4 * 5 + 2 * 4 * 3 * 4 * 5 and n_refused < 0.1 * n_uniform, (n_uniform, n_ragged, n_refused)
    assert n_one_launch > 50 and n_split > 50, (n_one_launch, n_split)
    # the 16-bit V rows are not needed; the K rows are read, so a table on a bank without them is an argument error
    bank, st = _structs(_case(n_layers=32))
    tb = _uniform(L, st, range(8))
    ref = _batch_answers(lib, bank, st, F16, tb)
    bank.v = None
    assert ref[0] == 0 and _kv164_batch_answers(lib, bank, st, F16, kv164, tb) == ref
    bank.k = None
    got = _kv164_batch_answers(lib, bank, st, F16, kv164, tb)
    assert got[:2] == [-1, -1] and got[2:11] == [-7] * 9 and got[11] == 0, got


def test_kv164_batch_refusals_come_before_any_launch():
    L, lib = _lib()
    kv164 = L.Kv164(256, 256)
    bank, st = _structs(_case(n_layers=32))
    tb = _uniform(L, st, range(8))
    assert _kv164_batch_answers(lib, bank, st, F16, kv164, tb)[0] == 0

    def refused(code, st=st, bank=bank, tb=tb, n=None, dt=F16, kv164=kv164):
        got = _kv164_batch_answers(lib, bank, st, dt, kv164, tb, n)
        assert got[0] == code, (code, got)
        if got[1] == 0:      # the info call answered: not one launch, no launches
            assert got[3] == 0 and got[10] == 0, got
        else:                # it refused its own arguments: the same code, the array untouched
            assert got[1] in (-1, -2) and got[2:11] == [-7] * 9, got
        assert got[11] == 0, got      # zero bytes
        b, s = ctypes.byref(bank), ctypes.byref(st)
        k = ctypes.byref(kv164) if kv164 is not None else None
        assert lib.ekv_kv164_batch_step_attend(b, s, dt, k, tb, len(tb) if n is None else n, None, None, None, None, None, None, 0, None) == code

    # EKV_E_UNSUPPORTED: head_dim 32 / 64 / 96, each of a table the 16-bit batch takes ...
    for kw in (dict(head_dim=32), dict(head_dim=64), dict(head_dim=96)):
        b2, s2 = _structs(_case(n_layers=32, **kw))
        t2 = _uniform(L, s2, range(8))
        assert _batch_answers(lib, b2, s2, F16, t2)[0] == 0, kw
        refused(-2, st=s2, bank=b2, tb=t2)
    for kw in (dict(hq=24, h=8), dict(hq=32, h=8), dict(hq=16, h=8), dict(hq=40, h=8), dict(hq=64, h=8)):      # every GQA factor the 16-bit batch takes
        b2, s2 = _structs(_case(n_layers=32, **kw))
        assert _kv164_batch_answers(lib, b2, s2, F16, kv164, _uniform(L, s2, range(8)))[0] == 0, kw
    # ... and what either family refuses: RoPE-on-read, chunk steps, every `phases` bit, deferred steps, the head-averaged tova row
    for kw in (dict(rope_on_read=1), dict(q_len=8, n_slots=2056, n_evict=8, roco_k1=1800, count_add2=16), dict(phases=16, phys_extent=2112),
               dict(phases=1 | 4), dict(phases=8), dict(phases=1), dict(phases=4), dict(phases=2), dict(phases=32, phys_extent=2112),
               dict(defer_layers=32, n_split=4, phases=8), dict(policy=3, tova_head_mean=1)):
        b2, s2 = _structs(_case(n_layers=32, **kw))
        refused(-2, st=s2, bank=b2)
    # EKV_E_ARG: a missing descriptor or plane, whichever — before the table is read
    refused(-1, kv164=None)
    for i in range(2):
        planes = [256] * 2
        planes[i] = None
        refused(-1, kv164=L.Kv164(*planes))
        assert lib.ekv_kv164_batch_step_check(ctypes.byref(bank), ctypes.byref(st), F16, ctypes.byref(L.Kv164(*planes)), None, 8) == -1
    for dt in (2, -1):
        refused(-1, dt=dt)
    refused(-1, n=0)
    refused(-1, tb=_uniform(L, st, [0, 1, 32]))
    refused(-1, tb=_uniform(L, st, [0, 5, 2, 5]))
    for field, bad in (("n_slots", 0), ("n_slots", 2113), ("roco_k1", 0), ("score_off", 2049), ("n_evict", 2049)):
        t2 = _uniform(L, st, range(8))
        setattr(t2[5], field, bad)
        refused(-1, tb=t2)


# ---- the host planner under sanitizers -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=COMPILERS or [None], ids=lambda c: os.path.basename(c) if c else "none")
def program(request, tmp_path_factory):
    if request.param is None:
        pytest.skip("no host C++ compiler on this machine")
    exe = str(tmp_path_factory.mktemp("plan_kv164") / "plan_kv164_main")
    # (the sanitizer runtimes linked into the program; nothing is loaded into Python)
    static = ["-static-libasan", "-static-libubsan"] if os.path.basename(request.param) == "g++" else []
    cmd = [request.param, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", *static,
           "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", os.path.join(ROOT, "tests", "plan_kv164_main.cpp"),
           os.path.join(ROOT, "easykv_amd", "csrc", "ekv_plan.cpp"), "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    return exe


def _library(L, lib, c, dtype=0, plane=0, nulls=0, seqs=None, n_seq=None):
    """The same kv164 call through the C ABI of the library: the row the program prints."""
    from tests.test_dispatch_table import KEYS
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
    q164 = L.Kv164(*[p(not (nulls & 64 and plane == i)) for i in range(2)])
    q = None if nulls & 32 else ctypes.byref(q164)
    info = (ctypes.c_int32 * 10)(*([-7] * 10))
    if seqs is not None:
        n = len(seqs) if n_seq is None else n_seq
        tb = (L.Seq * max(len(seqs), 1))()
        for i, e in enumerate(seqs):
            for k in SEQ_KEYS:
                setattr(tb[i], k, e[k])
        t = None if nulls & 128 else tb
        rc = [lib.ekv_kv164_batch_step_check(b, s, dtype, q, t, n), lib.ekv_kv164_batch_step_info(b, s, dtype, q, t, n, info, 10), lib.ekv_kv164_batch_workspace_bytes(b, s, dtype, q, t, n)]
    else:
        rc = [lib.ekv_kv164_step_check(b, s, dtype, q), lib.ekv_kv164_step_info(b, s, dtype, q, info, 10), lib.ekv_kv164_workspace_bytes(b, s, dtype, q)]
    return rc[:2] + list(info) + [rc[2]]


def test_host_planner_kv164_stages_under_sanitizers(program):
    """Uniform and ragged tables of the sweep in both element types, each missing plane, refused head_dims, and 8 000 arbitrary
    descriptors with and without a table: the stand-alone program ends without a sanitizer report and prints the library's answers."""
    import numpy as np
    L, lib = _lib()
    calls = []
    for c, uniform, ragged in _sweep():
        for dt in (F16, BF16):
            calls.append(((c,), dict(dtype=dt, seqs=uniform)))
            if ragged is not None:
                calls.append(((c,), dict(dtype=dt, seqs=ragged)))
    n_tables = len(calls)
    c0 = _case(n_layers=32)
    tb0 = [dict(layer=i, **{k: c0[k] for k in SEQ_KEYS[1:]}) for i in range(8)]
    calls += [((c0,), dict(seqs=tb0, nulls=64, plane=i)) for i in range(4)] + [((c0,), dict(nulls=64, plane=i)) for i in range(4)]      # (planes 2, 3: none)
    calls += [((c0,), dict(seqs=tb0, nulls=32)), ((c0,), dict(seqs=tb0, nulls=128)), ((c0,), dict(nulls=4 | 8)), ((c0,), dict(nulls=4)), ((c0,), dict(nulls=8)),
              ((c0,), dict(seqs=tb0, nulls=4)), ((c0,), dict(seqs=tb0, nulls=8))]
    calls += [((_case(n_layers=32, head_dim=d),), dict(seqs=tb0)) for d in (32, 64, 96)] + [((_case(n_layers=32, hq=64, h=8),), dict(seqs=tb0))]
    calls += _arbitrary_calls(n=8000, seed=202610164)
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    lines = [_line(*a, **kw) for a, kw in calls]
    r = subprocess.run([program], input="\n".join(lines) + "\n", env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-4000:])      # a sanitizer report ends the program with a non-zero status
    got = _u64(ln.split() for ln in r.stdout.splitlines())
    assert got.shape == (len(calls), 13), got.shape
    want = _u64(_library(L, lib, *a, **kw) for a, kw in calls)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert len(bad) == 0, [(calls[i], want[i].tolist(), got[i].tolist()) for i in bad[:3]]
    codes = [int(np.int64(w[0])) for w in want]
    assert sum(x == 0 for x in codes[:n_tables]) > 0.9 * n_tables and {0, -1, -2} <= set(codes[n_tables:]), sorted(set(codes))


# ---- precondition of the ragged GPU cases, on the reference side alone -----------------------------------------------------------------
@pytest.mark.parametrize("policy", cases.POLICIES)
@pytest.mark.parametrize("draw", [0, 1], ids=["short_first", "short_last"])
@pytest.mark.parametrize("shape", list(cases.SHAPES))
def test_ragged_case_inputs_leave_the_oracles_decisions_well_defined(shape, draw, policy):
    """The oracle over the ragged cases' seeded inputs (tests/batch_kv6_cases.py), K unquantised and V quantised by tests/kv4_ref.py (V cannot
    touch a decision), finds at least 90 % of EACH evicting entry's decisions well defined under
    tests.test_hip_fullsize.Probe: the cap tests/test_hip_batch_kv164.py asserts on the GPU."""
    from oracle import easykv_oracle as O
    from tests.test_hip_fullsize import Probe
    D, Hq, H, dtype = cases.SHAPES[shape]
    entries, tokens = cases.inputs(shape, draw)
    assert {2, 17, 96, 300, 2049} <= {e["T"] for e in entries}
    probe = Probe()
    O.SELECT_HOOK = probe
    try:
        for i, e in enumerate(entries):
            if not e["evict"]:
                continue
            kd, vd = K.dequant_ref(e["k0"], e["v0"])
            st = O.LayerState(k=kd.unsqueeze(0), v=vd.unsqueeze(0))
            st.s, st.q, st.c = O.init_state_decoding((H,), e["W"] - 1)
            st.s[:, :e["W"] - 1] += e["warm"]
            st.q[:, :e["W"] - 1] += e["warm"] ** 2
            n_dec = n_stable = 0
            for q, k, v in tokens:
                kn, vn = K.dequant_ref(k[i:i + 1], v[i:i + 1])
                _, ids = O.layer_step(st, q[i:i + 1].float(), kn, vn, O.StepPlan(**cases.plan_kw(e, policy)))
                assert ids is not None and st.k.shape[2] == e["T"] - 1
                n_dec += H
                n_stable += int((~probe.last_unstable).sum())
            print(f"[kv164-batch-precondition] {shape} draw {draw} {policy} T={e['T']}: {n_stable} of {n_dec} decisions well defined")
            assert n_stable >= 0.9 * n_dec, (shape, draw, policy, e["T"], n_stable, n_dec)
    finally:
        O.SELECT_HOOK = None
