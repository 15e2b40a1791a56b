"""Batched decode steps on FP8 K/V rows (include/easykv_hip.h, "kv8 batches") on a CPU: the four calls exist, their dry runs plan
a table exactly as the 16-bit batched call plans it and refuse what either family refuses before a launch, and the seeded inputs of
the ragged GPU case (tests/test_hip_batch_kv8.py, case (b)) leave the oracle's decisions well defined.  Dummy non-null pointers
throughout: nothing is dereferenced, nothing is launched."""
import ctypes
import itertools
import os
import re

import pytest
import torch

from tests import batch_kv8_cases as cases
from tests import kv8_ref as R
from tests.test_batch_cpu import _batch_answers, _lib, _policy_kw, _table, _uniform
from tests.test_dispatch_table import _case, _structs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("ekv_kv8_batch_step_check", "ekv_kv8_batch_step_info", "ekv_kv8_batch_workspace_bytes", "ekv_kv8_batch_step_attend")
F16, BF16 = 0, 1


def _kv8_batch_answers(lib, bank, st, dtype, kv8, tb, n=None):
    b, s, k = ctypes.byref(bank), ctypes.byref(st), (ctypes.byref(kv8) if kv8 is not None else None)
    n = len(tb) if n is None else n
    info = (ctypes.c_int32 * 9)(*([-7] * 9))
    return [lib.ekv_kv8_batch_step_check(b, s, dtype, k, tb, n), lib.ekv_kv8_batch_step_info(b, s, dtype, k, tb, n, info, 9)] + list(info) + \
           [lib.ekv_kv8_batch_workspace_bytes(b, s, dtype, k, tb, n)]


def test_kv8_batch_calls_are_exported_and_declared():
    L, lib = _lib()
    header = open(os.path.join(ROOT, "include", "easykv_hip.h")).read()
    declared = set(re.findall(r"\b(ekv_[a-z0-9_]+)\s*\(", header))
    raw = ctypes.CDLL(L.LIB)
    for name in CALLS:
        assert name in declared and name in L.EXPORTS and hasattr(raw, name) and hasattr(lib, name), name
    assert lib.ekv_abi_version() == 8
    # argument checks come before any device access
    assert lib.ekv_kv8_batch_step_check(None, None, F16, None, None, 1) == -1
    assert lib.ekv_kv8_batch_step_info(None, None, F16, None, None, 1, None, 0) == -1
    assert lib.ekv_kv8_batch_workspace_bytes(None, None, F16, None, None, 1) == 0
    assert lib.ekv_kv8_batch_step_attend(None, None, F16, None, None, 1, None, None, None, None, None, None, 0, None) == -1


def test_combination_instances_are_built_and_linked():
    """The four kv8 + batch lines of the manifest: parsed, named as the object tags say, and after a build present (tests/test_instances_cpu.py
    holds easykv_amd._build.objects(), everything that is linked, to the recorded set)."""
    from easykv_amd import _build
    want = [f"ekv_attn_decode_d{d}_plain_batch_kv8{t}" for d in (64, 128) for t in ("", "_bf16")]
    every = [n for n, _ in _build.objects()]
    got = [n for n in every if "batch_kv8" in n]
    assert got == want and len(set(every)) == len(every), got
    assert len(every) == len(_build.sources()) + len(_build.instances())      # one object per source + one per manifest line
    assert sum(1 for fam, w in _build.instances() if "kv8" in w and "batch" in w) == 4
    _build.build_lib()
    t = os.path.getmtime(_build.MANIFEST)
    for n in got:
        obj = os.path.join(_build.OBJ, n + ".o")
        assert os.path.exists(obj) and os.path.getmtime(obj) >= t, n


def test_kv8_batch_plans_as_the_16_bit_batch_of_the_same_table():
    """The uniform and the ragged tables of tests/test_batch_cpu.py at head_dim 64 / 128: return code, every info field and the
    workspace bytes of the kv8 batch call are those of the 16-bit batched call."""
    L, lib = _lib()
    kv8 = L.Kv8(256, 256, 256, 256)
    n_uniform = n_ragged = n_one_launch = n_split = 0
    for d, (hq, h), n_seq, T, policy in itertools.product((64, 128), ((32, 32), (32, 8), (8, 2), (24, 8)), (1, 2, 8, 33), (5, 300, 2049, 5002),
                                                          (0, 1, 2, 3, 4)):
        cap = (T + 64 + 63) // 64 * 64
        c = _case(head_dim=d, hq=hq, h=h, n_layers=40, cap=cap, layer_begin=0, layer_count=n_seq, n_slots=T, **_policy_kw(policy, T))
        bank, st = _structs(c)
        layers = [(7 * i + 3) % 40 for i in range(n_seq)]
        tables = [_uniform(L, st, layers)]
        if n_seq > 1:      # the ragged table of tests/test_batch_cpu.py
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
            tables.append(_table(L, entries))
        for ti, tb in enumerate(tables):
            for dt in (F16, BF16):
                ref = _batch_answers(lib, bank, st, dt, tb)
                got = _kv8_batch_answers(lib, bank, st, dt, kv8, tb)
                assert ref[0] == 0 and got == ref, (c, dt, ti, got, ref)
                n_uniform += ti == 0
                n_ragged += ti == 1
                n_one_launch += got[3] == 1
                n_split += got[2] > 1
    assert n_uniform == 2 * 2 * 4 * 4 * 4 * 5 and n_ragged == 2 * 2 * 4 * 3 * 4 * 5 and n_one_launch > 100 and n_split > 100, (n_uniform, n_ragged, n_one_launch, n_split)
    # the 16-bit row pointers are not needed
    bank, st = _structs(_case(n_layers=32))
    tb = _uniform(L, st, range(8))
    ref = _batch_answers(lib, bank, st, F16, tb)
    bank.k = bank.v = None
    assert ref[0] == 0 and _kv8_batch_answers(lib, bank, st, F16, kv8, tb) == ref


def test_kv8_batch_refusals_come_before_any_launch():
    L, lib = _lib()
    kv8 = L.Kv8(256, 256, 256, 256)
    bank, st = _structs(_case(n_layers=32))
    tb = _uniform(L, st, range(8))
    assert _kv8_batch_answers(lib, bank, st, F16, kv8, tb)[0] == 0

    def refused(code, st=st, bank=bank, tb=tb, n=None, dt=F16, kv8=kv8):
        got = _kv8_batch_answers(lib, bank, st, dt, kv8, tb, n)
        assert got[0] == code, (code, got)
        if got[1] == 0:      # the info call answered: not one launch, no launches
            assert got[3] == 0 and got[10] == 0, got
        else:                # it refused its own arguments: the same code, the array untouched
            assert got[1] in (-1, -2) and got[2:11] == [-7] * 9, got
        assert got[11] == 0, got      # zero bytes
        b, s = ctypes.byref(bank), ctypes.byref(st)
        k = ctypes.byref(kv8) if kv8 is not None else None
        # the real call answers the same before it looks at a pointer
        assert lib.ekv_kv8_batch_step_attend(b, s, dt, k, tb, len(tb) if n is None else n, None, None, None, None, None, None, 0, None) == code

    # EKV_E_UNSUPPORTED: what a kv8 step refuses (head_dim 32 / 96) ...
    for d in (32, 96):
        b2, s2 = _structs(_case(n_layers=32, head_dim=d))
        t2 = _uniform(L, s2, range(8))
        assert _batch_answers(lib, b2, s2, F16, t2)[0] == 0, d      # (the 16-bit batch takes it)
        refused(-2, st=s2, bank=b2, tb=t2)
    # ... and what either family refuses: RoPE-on-read, chunk steps, every `phases` bit, deferred steps, the head-averaged tova row
    for kw in (dict(rope_on_read=1), dict(q_len=8, n_slots=2056, n_evict=8, roco_k1=1800, count_add2=16), dict(phases=16, phys_extent=2112),
               dict(phases=1 | 4), dict(phases=8), dict(phases=1), dict(phases=4), dict(phases=2), dict(phases=32, phys_extent=2112),
               dict(defer_layers=32, n_split=4, phases=8), dict(policy=3, tova_head_mean=1)):
        b2, s2 = _structs(_case(n_layers=32, **kw))
        refused(-2, st=s2, bank=b2)
    # ... and scored shapes only the generic scorer serves: GQA factors > 8, more than 6144 slots, cap % 4 != 0
    for kw in (dict(hq=48, h=4), dict(n_slots=7000, cap=7040, roco_k1=5000), dict(n_slots=2049, cap=2114)):
        b2, s2 = _structs(_case(n_layers=32, **kw))
        refused(-2, st=s2, bank=b2, tb=_uniform(L, s2, range(8)))
    # EKV_E_ARG: a missing descriptor or plane
    refused(-1, kv8=None)
    for i in range(4):
        planes = [256] * 4
        planes[i] = None
        refused(-1, kv8=L.Kv8(*planes))
    # ... a bad element type, and a bad table
    for dt in (2, -1):
        refused(-1, dt=dt)
    refused(-1, n=0)
    refused(-1, tb=_uniform(L, st, list(range(32)) * 3), n=65)
    refused(-1, tb=_uniform(L, st, [0, 1, 32]))
    refused(-1, tb=_uniform(L, st, [0, 5, 2, 5]))
    assert lib.ekv_kv8_batch_step_check(ctypes.byref(bank), ctypes.byref(st), F16, ctypes.byref(kv8), None, 4) == -1
    assert lib.ekv_kv8_batch_step_check(None, ctypes.byref(st), F16, ctypes.byref(kv8), tb, 8) == -1
    assert lib.ekv_kv8_batch_step_check(ctypes.byref(bank), None, F16, ctypes.byref(kv8), tb, 8) == -1
    for field, bad in (("n_slots", 0), ("n_slots", 2113), ("roco_k1", 0), ("score_off", 2049), ("n_evict", 2049)):
        t2 = _uniform(L, st, range(8))
        setattr(t2[5], field, bad)
        refused(-1, tb=t2)
    # a short entry keeps its own bounds
    t2 = _uniform(L, st, range(8))
    t2[2].n_slots, t2[2].roco_k1 = 100, 1434
    refused(-1, tb=t2)
    t2[2].roco_k1 = 60
    assert _kv8_batch_answers(lib, bank, st, F16, kv8, t2)[0] == 0


@pytest.mark.parametrize("policy", cases.POLICIES)
@pytest.mark.parametrize("draw", [0, 1], ids=["short_first", "short_last"])
@pytest.mark.parametrize("shape", list(cases.SHAPES))
def test_ragged_case_inputs_leave_the_oracles_decisions_well_defined(shape, draw, policy):
    """The precondition of GPU case (b), on the reference side alone: the oracle over the case's seeded inputs, prompt rows and
    appended rows quantised by tests/kv8_ref.py, must find at least 90 % of EACH evicting entry's decisions well defined under
    tests.test_hip_fullsize.Probe.  A seed that does not meet it is changed (tests/batch_kv8_cases.py SEEDS), never the cap."""
    from oracle import easykv_oracle as O
    from tests.test_hip_fullsize import Probe
    D, Hq, H, dtype = cases.SHAPES[shape]
    entries, tokens = cases.inputs(shape, draw)
    assert [e["T"] for e in entries] == (list(cases.RAGGED_T) if draw == 0 else list(reversed(cases.RAGGED_T)))
    probe = Probe()
    O.SELECT_HOOK = probe
    try:
        for i, e in enumerate(entries):
            if not e["evict"]:
                continue
            st = O.LayerState(k=R.dequant(*R.quantize(e["k0"])).unsqueeze(0), v=R.dequant(*R.quantize(e["v0"])).unsqueeze(0))
            st.s, st.q, st.c = O.init_state_decoding((H,), e["W"] - 1)
            st.s[:, :e["W"] - 1] += e["warm"]
            st.q[:, :e["W"] - 1] += e["warm"] ** 2
            n_dec = n_stable = 0
            for q, k, v in tokens:
                kq, vq = R.dequant(*R.quantize(k[i:i + 1])), R.dequant(*R.quantize(v[i:i + 1]))
                _, ids = O.layer_step(st, q[i:i + 1].float(), kq, vq, O.StepPlan(**cases.plan_kw(e, policy)))
                assert ids is not None and st.k.shape[2] == e["T"] - 1
                n_dec += H
                n_stable += int((~probe.last_unstable).sum())
            print(f"[kv8-batch-precondition] {shape} draw {draw} {policy} T={e['T']}: {n_stable} of {n_dec} decisions well defined")
            assert n_stable >= 0.9 * n_dec, (shape, draw, policy, e["T"], n_stable, n_dec)
    finally:
        O.SELECT_HOOK = None
