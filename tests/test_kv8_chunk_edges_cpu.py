"""The cases of tests/kv8_chunk_edge_cases.py on a CPU: every case plans as its table row says (the dry run of the ekv_kv8_chunk_* calls:
dummy non-null pointers, nothing is launched), reaches the edges it is in the table for (the planner's rows_per_split and the kernel's
t0 / t1 / append rule, restated there), and — an evicting case — has a head whose victims the GPU test can compare exactly."""
import ctypes

import pytest

from tests import kv8_chunk_edge_cases as E
from tests.test_dispatch_table import _case, _structs

DTYPE = {E.F16: 0, E.BF: 1}


def _info(case, **kw):
    from tests.test_kv8_cpu import _lib
    L, lib = _lib()
    bank, st = _structs(_case(**E.step_fields(case, **kw)))
    kv8 = L.Kv8(256, 256, 256, 256)
    b, s, k = ctypes.byref(bank), ctypes.byref(st), ctypes.byref(kv8)
    info = (ctypes.c_int32 * 10)(*([-7] * 10))
    assert lib.ekv_kv8_chunk_step_check(b, s, DTYPE[case.dtype], k) == 0, case.name      # EKV_OK
    assert lib.ekv_kv8_chunk_step_info(b, s, DTYPE[case.dtype], k, info, 10) == 0, case.name
    keys = ("n_split", "fused", "two_pass", "wide", "n_qblocks", "qb_rows", "n_col_parts", "fold_in_kernel", "n_launches", "fused_order")
    return dict(zip(keys, (int(x) for x in info)))


def test_the_table_is_what_the_issue_lists():
    names = [c.name for c in E.CASES]
    assert len(set(names)) == len(names)
    assert all(c.dtype is E.F16 for c in E.CASES if not c.name.endswith("-bf16"))
    assert {c.name[:-5] for c in E.CASES if c.dtype is E.BF} == {"straddle", "empty-pairs", "rep5"}
    assert all(E.BY_NAME[n + "-bf16"]._replace(name=n, dtype=E.F16, seed=0) == E.BY_NAME[n]._replace(seed=0) for n in ("straddle", "empty-pairs", "rep5"))
    assert all(c.policy in ("roco", "h2o_head") for c in E.CASES if c.name != "dense-prefix") and E.BY_NAME["dense-prefix"].policy == "full"
    assert {c.T0 + c.n for c in E.CASES if c.name.startswith("boundaries")} == {95, 96, 97, 127, 128, 129}
    assert all(c.n == 2 * (32 // c.rep) + 1 for c in E.CASES if c.name in ("rep3", "rep5", "rep7"))
    assert set(E.NON_EVICTING + E.VIEWS + E.TWO_STEPS) <= set(names)


FORMS = [(c, True) for c in E.CASES] + [(E.BY_NAME[n], False) for n in E.NON_EVICTING]


@pytest.mark.parametrize("case,evict", FORMS, ids=[c.name + ("" if e else "-accumulate-only") for c, e in FORMS])
def test_case_plans_as_claimed_and_reaches_its_edges(case, evict):
    info = _info(case, evict=evict)
    assert info["two_pass"] == 0 and info["wide"] == 0 and info["n_launches"] > 0, info
    assert (info["n_split"], info["n_qblocks"], info["qb_rows"]) == case.expect, info
    assert info["qb_rows"] * case.rep <= 32 and info["n_qblocks"] == -(-case.n // info["qb_rows"])
    got = E.edges(case, info["n_split"], info["qb_rows"])
    assert set(case.reaches) <= got, (case.name, sorted(set(case.reaches) - got))
    assert ("fused_tail" in got) == bool(info["fused"]) and (not info["fused"] or info["n_launches"] == 1), info
    # what the table's comments say in numbers
    rps, wgs = E.geometry(case, info["n_split"], info["qb_rows"])
    if case.name.startswith("straddle") or case.name == "empty-pairs":
        assert rps == (128 if case.D == 128 else 64)
    if case.name.startswith("empty-pairs"):
        assert [w["nb"] for w in wgs if w["split"] == 0] == [32, 32, 32, 4]
        w = next(w for w in wgs if w["split"] == 1 and w["i0"] == 0)
        assert w["t1"] == 52 and w["t0"] == 64
    if case.name == "dense-prefix":
        assert sum(w["t0"] >= w["t1"] for w in wgs) == 8 and [w["nb"] for w in wgs if w["split"] == 0] == [16] * 9 + [6]
    if case.name.startswith("rep") and case.rep in (3, 5, 7):
        assert sorted({w["NR"] for w in wgs}) == [case.rep, {3: 30, 5: 30, 7: 28}[case.rep]]


@pytest.mark.parametrize("name", E.VIEWS)
def test_the_deferred_form_plans_the_same_geometry(name):
    """The deferred runs (L = 3, one layer per call, phases 1 | 4 then 8): the per-layer call and the flush are accepted, and the
    per-layer call has the immediate call's split, blocks and rows per block."""
    case = E.with_layers(E.BY_NAME[name], 3)
    now = _info(case)
    fields = dict(E.step_fields(case, n_split=now["n_split"]), defer_layers=3)
    from tests.test_kv8_cpu import _lib
    L, lib = _lib()
    kv8 = L.Kv8(256, 256, 256, 256)
    for phases, lb, lc in ((1 | 4, 1, 1), (8, 0, 3)):
        bank, st = _structs(_case(**dict(fields, phases=phases, layer_begin=lb, layer_count=lc, defer_index=lb)))
        info = (ctypes.c_int32 * 10)()
        assert lib.ekv_kv8_chunk_step_check(ctypes.byref(bank), ctypes.byref(st), 0, ctypes.byref(kv8)) == 0, (name, phases)
        assert lib.ekv_kv8_chunk_step_info(ctypes.byref(bank), ctypes.byref(st), 0, ctypes.byref(kv8), info, 10) == 0
        assert (info[0], info[4], info[5]) == case.expect and info[1] == 0 and info[8] > 0, (name, phases, list(info))


EVICTING = [c for c in E.CASES if c.policy != "full"] + [E.with_layers(E.BY_NAME[n], 3)._replace(name=n + "-3-layers") for n in E.VIEWS]


@pytest.mark.parametrize("case", EVICTING, ids=lambda c: c.name)
def test_an_evicting_case_has_a_head_to_compare_exactly(case):
    """The condition the GPU test needs (not a measurement): on the rule's restatement of the bank, at least one head of every stepping
    layer is both stable under the probe and left uncut by roco's feasible set.  Seeds are picked here until it holds.  (The 3-layer
    forms are what the deferred runs of the GPU test draw.)"""
    for l, (_, ids_ref, exact) in enumerate(E.restate(case, E.draw(case))):
        assert ids_ref is not None and tuple(ids_ref.shape) == (case.H, case.n)
        assert exact, (case.name, l, "no stable and uncut head: pick another seed in tests/kv8_chunk_edge_cases.py")
