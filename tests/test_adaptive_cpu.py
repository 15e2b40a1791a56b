"""Adaptive head budgets without a GPU (include/easykv_hip.h, "adaptive head budgets"): the exports, dry runs of the call
family (ekv_ada_*) through the C ABI over fake banks (nothing is dereferenced, nothing is launched), the planner driven over an adaptive
grid by a stand-alone program under AddressSanitizer + UBSan (tests/plan_ada_main.cpp; the sanitizer runtimes are linked into the program,
which runs as a child process), the new manifest lines, the engine's routing, and the reference's own rule (tests/adaptive_ref.py).

What the plans must say: an adaptive step plans as the pooled call of the same step — for radius 0, as the plain call asked for
"attention, then the scorer" (phases = 1 | 2) — field for field, except that the scorer launch counts three kernels (n_launches is two
higher) and the workspace holds 4 + 1 bytes more per (layer, head, padded column); every refusal leaves zero launches and zero bytes."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest
import torch

from tests import adaptive_ref as A
from tests.test_dispatch_table import _case, _chunk, _structs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMPILERS = [c for c in ("g++", "/opt/rocm/llvm/bin/clang++") if shutil.which(c)]
INFO = ("n_split", "one_launch", "two_pass", "wide", "n_qblocks", "qb_rows", "n_col_parts", "fold_in_kernel", "n_launches", "fused_order")
F16, BF16 = 0, 1
OK, ARG, UNSUPPORTED = 0, -1, -2
CALLS = ("ekv_ada_step_check", "ekv_ada_step_info", "ekv_ada_workspace_bytes", "ekv_ada_step_attend")
U64 = 2 ** 64 - 1


@pytest.fixture(scope="module")
def lib():
    from easykv_amd import _build, _lib
    if not os.path.exists(_build.LIB):
        _build.build_lib()
    return _lib.load()


def _answers(check, info_fn, ws, bank, st, dtype, *desc):
    b, s = ctypes.byref(bank), ctypes.byref(st)
    info = (ctypes.c_int32 * 10)(*([-7] * 10))
    return [check(b, s, dtype, *desc), info_fn(b, s, dtype, *desc, info, 10)] + list(info) + [ws(b, s, dtype, *desc)]


def _plain(lib, bank, st, dtype):
    return _answers(lib.ekv_step_check_typed, lib.ekv_step_info_typed, lib.ekv_workspace_bytes_typed, bank, st, dtype)


def _pool(lib, bank, st, dtype, radius, op):
    from easykv_amd import _lib as L
    return _answers(lib.ekv_pool_step_check, lib.ekv_pool_step_info, lib.ekv_pool_workspace_bytes, bank, st, dtype, ctypes.byref(L.Pool(radius, op)))


def _ada(lib, bank, st, dtype, lo, hi, radius=3, op=0, null=0):
    from easykv_amd import _lib as L
    desc = None if null == 1 else ctypes.byref(L.Ada(radius, op, lo, hi, None if null == 2 else 256))
    return _answers(lib.ekv_ada_step_check, lib.ekv_ada_step_info, lib.ekv_ada_workspace_bytes, bank, st, dtype, desc)


def _refused(got, code=UNSUPPORTED):
    d = dict(zip(INFO, got[2:12]))
    return got[0] == code and got[12] == 0 and (got[1] != 0 or (d["n_launches"] == 0 and d["one_launch"] == 0))


def _align(x, a):
    return (x + a - 1) // a * a


def _extra_bytes(layers, h, T):
    t_pad = _align(T, 64)
    return _align(layers * h * t_pad * 4, 256) + _align(layers * h * t_pad, 256)


def _as_twin(got, twin, extra, launches=2):
    """The adaptive answers are the twin's with `launches` more kernels and `extra` more bytes."""
    want = list(twin)
    want[2 + INFO.index("n_launches")] += launches
    want[12] += extra
    return got == want


def test_ada_calls_are_exported_and_declared(lib):
    from easykv_amd import _lib as L
    header = open(os.path.join(ROOT, "include", "easykv_hip.h")).read()
    declared = set(re.findall(r"\b(ekv_[a-z0-9_]+)\s*\(", header))
    raw = ctypes.CDLL(L.LIB)
    for name in CALLS:
        assert name in declared and name in L.EXPORTS and hasattr(raw, name), name
    assert lib.ekv_abi_version() == 8
    assert re.search(r"typedef struct ekv_ada \{\s*int32_t radius;\s*int32_t op;\s*int32_t evict_min;\s*int32_t evict_max;\s*int32_t \*n_evict_out;\s*\} ekv_ada;", header)
    for text in ("Adaptive head budgets", "FORCED", "PROTECTED", "FREE", "(key, head, j)", "0 <= evict_min <= n_evict <= evict_max <= C"):
        assert text in header, text
    assert lib.ekv_ada_step_check(None, None, F16, None) == ARG
    assert lib.ekv_ada_workspace_bytes(None, None, F16, None) == 0
    # every existing struct is untouched: the budgets are an argument of the four calls
    assert ctypes.sizeof(L.Step) == 31 * 4 and ctypes.sizeof(L.Pool) == 8 and ctypes.sizeof(L.Ada) == 24


def test_manifest_holds_the_adaptive_lines():
    from easykv_amd import _build
    later = dict(_build.later_objects())
    names = [f"ekv_score_select_ada_nt{nt}{e}" for nt in (512, 1024) for e in ("", "_bf16")]
    for name in names:
        assert name in later and "-DEKV_ADA=1" in later[name] and "-DEKV_POOL=1" not in later[name] and later[name][-1].endswith("ekv_score_select.inc"), name
    assert later["ekv_score_allot"][-1].endswith("ekv_score_allot.inc") and "-DEKV_ALLOT_NT=1024" in later["ekv_score_allot"]
    everything = _build.objects() + _build.added_objects() + _build.later_objects()
    assert sorted(n for n, a in everything if "-DEKV_ADA=1" in a) == sorted(names)
    assert not [n for n, _ in _build.objects() + _build.added_objects() if "ada" in n or "allot" in n]
    assert not [n for n in names + ["ekv_score_allot"] if "pool" in n]
    assert {"EKV_SCORE_SELECT_ADA", "EKV_SCORE_ALLOT"} <= set(_build.FAMILIES)


def test_adaptive_plans_and_refusals_by_name(lib):
    # a one-shot observation step of a 7B-shaped model: 32 queries over 4096 keys, half of them evicted; 32 layers at once and one layer
    for layers in (32, 1):
        c = _chunk(layers, 32, 32, 32, 4064, policy=1, n_evict=2048, win_lo=4, win_tail=32)
        bank, st = _structs(c)
        C = 4096 - 4 - 32
        for lo, hi in ((2048, 2048), (1000, 3000), (0, C)):
            got = _ada(lib, bank, st, F16, lo, hi)
            assert got[0] == OK and _as_twin(got, _pool(lib, bank, st, F16, 3, 0), _extra_bytes(layers, 32, 4096)), (layers, lo, hi, got)
        # radius 0: the plain call asked for attention, then the scorer
        got = _ada(lib, bank, st, F16, 1000, 3000, radius=0)
        st.phases = 3
        assert got[0] == OK and _as_twin(got, _plain(lib, bank, st, F16), _extra_bytes(layers, 32, 4096)), (layers, got)
    # a decode step: never the one-launch kernel
    bank, st = _structs(_case(n_layers=32, policy=1, win_tail=600))
    assert _plain(lib, bank, st, F16)[3] == 1
    got = _ada(lib, bank, st, F16, 1, 1)
    assert got[0] == OK and got[3] == 0 and got[10] >= 4, got
    # the refusals, each a step the plain call takes
    base = dict(policy=1, n_evict=1000, win_lo=4, win_tail=32)
    refusals = [_chunk(2, 8, 8, 32, 2000, **dict(base, policy=2)), _chunk(2, 8, 8, 32, 2000, **dict(base, policy=4, range_start=4)),
                _chunk(2, 8, 8, 32, 2000, rope_on_read=1, **base), _chunk(2, 8, 8, 32, 2000, **dict(base, policy=3, tova_head_mean=1))]
    for c in refusals:
        bank, st = _structs(c)
        assert _plain(lib, bank, st, F16)[0] == OK, c
        assert _refused(_ada(lib, bank, st, F16, 500, 1500)), c
    bank, st = _structs(_case(n_layers=32, phases=16, phys_extent=2112, policy=1, win_tail=0))
    assert _refused(_ada(lib, bank, st, F16, 1, 1)), "slot rows"
    bank, st = _structs(_chunk(1, 1, 1, 8, 38392, d=64, **dict(base, n_evict=20000, win_tail=8)))
    assert _refused(_ada(lib, bank, st, F16, 20000, 20000)), "past the generic scorer's width"
    bank, st = _structs(_chunk(1, 1, 1, 8, 38360, d=64, **dict(base, n_evict=20000, win_tail=8)))
    assert _ada(lib, bank, st, F16, 20000, 20000)[0] == OK
    # more than 64 KV heads: the pooled call takes the step, the adaptive one does not
    for h, want in ((64, OK), (65, UNSUPPORTED)):
        bank, st = _structs(_chunk(1, h, h, 32, 2000, **base))
        assert _pool(lib, bank, st, F16, 3, 0)[0] == OK
        got = _ada(lib, bank, st, F16, 500, 1500)
        assert got[0] == want and (want == OK or _refused(got)), (h, got)
    # argument errors
    bank, st = _structs(_chunk(2, 8, 8, 32, 2000, **base))
    C = 2032 - 4 - 32
    assert _ada(lib, bank, st, F16, 500, 1500)[0] == OK and _ada(lib, bank, st, F16, 0, C)[0] == OK and _ada(lib, bank, st, F16, 1000, 1000, radius=0)[0] == OK
    for kw in (dict(null=1), dict(null=2), dict(radius=-1), dict(op=2), dict(op=-1)):
        assert _refused(_ada(lib, bank, st, F16, 500, 1500, **kw), ARG), kw
    for lo, hi in ((-1, 1500), (1001, 1500), (500, 999), (500, C + 1)):
        assert _refused(_ada(lib, bank, st, F16, lo, hi), ARG), (lo, hi)
    bank, st = _structs(_chunk(2, 8, 8, 32, 2000, **dict(base, n_evict=0)))
    assert _refused(_ada(lib, bank, st, F16, 0, 0), ARG), "an adaptive step evicts"
    bank, st = _structs(_chunk(2, 8, 8, 32, 2000, **base))
    assert lib.ekv_ada_step_check(ctypes.byref(bank), ctypes.byref(st), 2, None) == ARG


# ---- the planner as a stand-alone program under the sanitizers ---------------------------------------------------------------------------
@pytest.fixture(scope="module", params=COMPILERS or [None], ids=lambda c: os.path.basename(c) if c else "none")
def program(request, tmp_path_factory):
    if request.param is None:
        pytest.skip("no host C++ compiler on this machine")
    exe = str(tmp_path_factory.mktemp("plan_ada") / "plan_ada_main")
    static = ["-static-libasan", "-static-libubsan"] if os.path.basename(request.param) == "g++" else []
    cmd = [request.param, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", *static,
           "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", os.path.join(ROOT, "tests", "plan_ada_main.cpp"),
           os.path.join(ROOT, "easykv_amd", "csrc", "ekv_plan.cpp"), "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    return exe


def test_ada_planner_grid_ends_clean_and_answers_as_the_library(program, lib):
    from easykv_amd import _lib as L
    r = subprocess.run([program], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-4000:])      # (a sanitizer report ends the program with a non-zero status)
    lines = r.stdout.splitlines()
    assert len(lines) > 3000
    n = dict(as_twin=0, degenerate=0, radius0=0, refused=0, arg=0, heads=0, deferred=0, attention_only=0, big=0)
    bad = []
    for i, ln in enumerate(lines):
        left, right = ln.split("=>")
        ada, twin = right.split("|")
        (d, hq, h, layers, cap_rows, q_len, T, policy, n_evict, win_lo, win_tail, rope, n_split, two_pass, dtype, head_mean, phases, defer_layers,
         radius, op, lo, hi, null) = (int(x) for x in left.split())
        got, ref = [int(x) for x in ada.split()], [int(x) for x in twin.split()]
        assert len(got) == 13 and len(ref) == 12
        ref = [ref[0], 0] + ref[1:]      # (in the layout of `got`: check, info rc, ten fields, bytes)
        if dtype in (F16, BF16) and i % 3 == 0:      # the library gives the same answers
            bank = L.Bank(256, 256, 256, 256, 256, 256, layers, hq, h, d, cap_rows, 256, 256, 256)
            st = L.Step()
            st.layer_count, st.q_len, st.n_slots, st.policy, st.n_evict, st.win_lo, st.win_tail = layers, q_len, T, policy, n_evict, win_lo, win_tail
            st.roco_k1 = max(T - q_len - 4, n_evict)
            st.range_start, st.rope_on_read, st.n_split, st.two_pass, st.roco_tail, st.causal, st.sm_div = (4 if policy == 4 else -1), rope, n_split, two_pass, 10, 1, 8.0
            st.tova_head_mean, st.phases, st.accumulate = head_mean, phases, int(policy != 0)
            st.count_add, st.count_tail_step = float(q_len), -1.0
            if defer_layers:
                st.defer_layers = defer_layers
                if phases == 5:
                    st.layer_begin = st.defer_index = 1
                    st.layer_count = 1
            want = _ada(lib, bank, st, dtype, lo, hi, radius, op, null)
            if [x & U64 for x in want] != [x & U64 for x in got]:
                bad.append((ln, want))
        C = T - win_lo - win_tail
        if null or radius < 0 or op not in (0, 1) or dtype not in (F16, BF16) or not (0 <= lo <= n_evict <= hi <= C and n_evict >= 1):
            assert _refused(got, ARG), ln
            n["arg"] += 1
        elif policy not in (1, 3) or rope or head_mean or phases == 16 or h > 64 or ref[0] != OK:
            assert _refused(got, got[0]) and got[0] in (UNSUPPORTED, ARG), ln
            n["refused"] += 1
            n["heads"] += h > 64 and ref[0] == OK
        else:
            extra = _extra_bytes(defer_layers or layers, h, T)
            assert got[0] == OK and _as_twin(got, ref, extra, 0 if phases == 5 else 2), ln
            n["as_twin"] += 1
            n["degenerate"] += lo == hi
            n["radius0"] += radius == 0
            n["deferred"] += phases == 8
            n["attention_only"] += phases == 5
            n["big"] += T >= 12000
    assert not bad, bad[:3]
    assert all(v > 0 for v in n.values()), n
    print(f"[adaptive] planner grid: {n}")


def test_engine_routes_adaptive_steps_to_their_family():
    from easykv_amd import engine
    from easykv_amd._lib import EkvError

    class Lib:
        def __getattr__(self, name):
            return name
    bank = engine.KVBank.__new__(engine.KVBank)
    bank.lib, bank._pool_fams, bank._ada_fams, bank._fmt = Lib(), {}, {}, None
    bank.logit_cap = bank.sinks = bank.windows = None
    bank.long_rows, bank.kv_quant = False, None
    bank.n_layers, bank.n_kv_heads, bank.device = 2, 4, "cpu"
    bank._ada_out = None
    bank._check_fn, bank._info_fn, bank._ws_fn, bank._attend_fn, bank._desc_ref = "c", "i", "w", "a", ()
    assert engine.StepPlan().head_adaptive is None and bank._family(engine.StepPlan()) == ("c", "i", "w", "a", ())
    fam = bank._family(engine.StepPlan(pool=7, pool_op="avg", head_adaptive=(10, 30)))
    assert fam[:4] == CALLS and len(fam[4]) == 1
    desc = bank._ada_fams[(3, 1, 10, 30)][5]
    assert (desc.radius, desc.op, desc.evict_min, desc.evict_max) == (3, 1, 10, 30) and desc.n_evict_out == bank._ada_out.data_ptr()
    assert tuple(bank._ada_out.shape) == (2, 4) and bank._ada_out.dtype == torch.int32
    fam1 = bank._family(engine.StepPlan(pool=1, head_adaptive=(10, 30)))      # kernel size 1: radius 0, the unpooled rows rank
    assert fam1[:4] == CALLS and bank._ada_fams[(0, 0, 10, 30)][5].radius == 0
    bank._ada_row(engine.StepPlan(pool=7, pool_op="avg", head_adaptive=(10, 30)), 1)
    assert desc.n_evict_out == bank._ada_out.data_ptr() + 16
    # evict_ids: [layers][H][evict_max] whatever the caller wants back; any other tensor is refused
    plan = engine.StepPlan(pool=7, pool_op="avg", head_adaptive=(10, 30))
    for given in (None, False):
        ids = bank._ada_ids(plan, 2, given)
        assert tuple(ids.shape) == (2, 4, 30) and ids.dtype == torch.int32 and bool((ids == -1).all())
    mine = torch.zeros(2, 4, 30, dtype=torch.int32)
    assert bank._ada_ids(plan, 2, mine) is mine
    for bad in (torch.zeros(2, 4, 20, dtype=torch.int32), torch.zeros(2, 4, 30, dtype=torch.int64), torch.zeros(2, 4, 60, dtype=torch.int32)[:, :, ::2]):
        with pytest.raises(ValueError, match="evict_max"):
            bank._ada_ids(plan, 2, bad)
    # raggedness is per layer
    bank.head_slots = None
    assert not bank._ragged(0, 2)
    bank.head_slots = [None, [5, 6, 7, 8]]
    assert not bank._ragged(0, 1) and bank._ragged(1, 1) and bank._ragged(0, 2)
    with pytest.raises(EkvError, match="different numbers of rows"):
        bank._refuse_ragged(0, 2)
    for bad in ((1,), (1, 2, 3), (1.0, 2), "12", 5, (True, 2)):
        with pytest.raises(ValueError, match="head_adaptive"):
            bank._family(engine.StepPlan(head_adaptive=bad))
    for bad in (0, 2, -3, "7"):
        with pytest.raises(ValueError, match="kernel size"):
            bank._family(engine.StepPlan(pool=bad, head_adaptive=(1, 2)))
    for attr, value, match in (("logit_cap", 30.0, "logit_cap"), ("sinks", torch.zeros(1, 1), "sinks"), ("windows", (0,), "windows"),
                               ("long_rows", True, "long_rows"), ("_fmt", engine.ROW_FORMATS["fp8"], "kv_quant")):
        b2 = engine.KVBank.__new__(engine.KVBank)
        b2.__dict__.update(bank.__dict__)
        setattr(b2, attr, value)
        if attr == "_fmt":
            b2.kv_quant = "fp8"
        with pytest.raises(EkvError, match=match):
            b2._family(engine.StepPlan(head_adaptive=(1, 2)))


def test_reference_rule_on_hand_made_rows():
    """tests/adaptive_ref.py's `allot` on rows small enough to check by hand, ties included."""
    # two heads, six candidates each (sink 1, obs 1), n_evict 3, evict_min 1, evict_max 5
    rank = torch.tensor([[9., 0., 1., 2., 3., 4., 5., 9.], [9., 0., 0., 5., 5., 5., 5., 9.]])
    # forced: head 0 {1}, head 1 {1}; protected: head 0 {6}, head 1 {6}; four more victims among the free {1,2,3,4 | 0,5,5,5}: 0 (h1), 1, 2, 3 (h0)
    k, victims = A.allot(rank, 3, 1, 5, 1, 1)
    assert k == [4, 2] and victims[0].tolist() == [1, 2, 3, 4] and victims[1].tolist() == [1, 2]
    # a tie at the threshold goes to the lower head, then to the lower index
    rank = torch.tensor([[9., 1., 1., 1., 1., 9.], [9., 1., 1., 1., 1., 9.]])
    k, victims = A.allot(rank, 2, 0, 4, 1, 1)
    assert k == [4, 0] and victims[0].tolist() == [1, 2, 3, 4]
    k, victims = A.allot(rank, 2, 1, 3, 1, 1)
    assert k == [3, 1] and victims[0].tolist() == [1, 2, 3] and victims[1].tolist() == [1]
    # degenerate bounds: every head evicts n_evict; NaN ranks largest
    rank = torch.tensor([[9., 3., float("nan"), 1., 2., 9.], [9., 4., 3., 2., 1., 9.]])
    k, victims = A.allot(rank, 2, 2, 2, 1, 1)
    assert k == [2, 2] and victims[0].tolist() == [3, 4] and victims[1].tolist() == [3, 4]
    k, victims = A.allot(rank, 3, 0, 4, 1, 1)
    assert sum(k) == 6 and 2 not in victims[0].tolist()[:3] and k == [3, 3]
    for args in ((3, 1, 5), (2, 0, 4)):
        r = torch.rand(3, 40, generator=torch.Generator().manual_seed(5))
        kk, vv = A.allot(r, args[0] * 4, args[1] * 4, args[2] * 4, 2, 4)
        assert A.valid(vv, r, args[0] * 4, args[1] * 4, args[2] * 4, 2, 4) and sum(kk) == 3 * args[0] * 4


# ---- the driver over stub caches (the fixtures of tests/test_oneshot_cpu.py) -------------------------------------------------------------------
from tests.test_oneshot_cpu import OneShotBank, StubCache, _ids, _model, _run, api      # noqa: E402,F401  (`api` is a fixture)


@pytest.fixture
def no_library(monkeypatch):
    """The shared library must not be touched: a refusal of the driver comes before the first bank, and so before the library is loaded."""
    from easykv_amd import _lib

    def load():
        raise AssertionError("_lib.load() was called")
    monkeypatch.setattr(_lib, "load", load)


@pytest.mark.parametrize("mode,policy,pool", [("encoding", "h2o_head", 7), ("auto", "tova", 3), ("encoding", "h2o_head", 1)])
def test_the_key_puts_the_bounds_into_the_observation_plan_and_sizes_the_decode_bank_by_the_ceiling(api, mode, policy, pool):
    n, B, obs, m = 200, 80, 16, 5
    base = dict(kv_policy=policy, budget=B, max_new_tokens=m, prefill="one_shot", obs_window=obs, score_pool=pool)
    for extra, lo, hi in ((dict(), 60, 168), (dict(head_budget_floor=0.5, head_budget_ceil=1.5), 90, 150), (dict(head_budget_floor=1.0, head_budget_ceil=1.0), 120, 120),
                          (dict(head_budget_floor=0, head_budget_ceil=10), 0, 180)):
        OneShotBank.handed.clear()
        res, cache, line = _run(api, _model(), n, dict(base, head_budgets="adaptive", **extra), mode)
        assert (lo, hi) == A.budget_bounds(n, B, obs, 4, extra.get("head_budget_floor", 0.2), extra.get("head_budget_ceil", 2.0))[1:]
        pre = [f for f in cache.log if f[2]["phase"] == "prefill"]
        assert [f[0] for f in pre] == [n - obs, obs] and pre[0][2]["head_adaptive"] is None
        b = pre[1][2]
        assert (b["head_adaptive"], b["n_evict"], b["pool"], b["sink"], b["recent"], b["tova_head_mean"]) == ((lo, hi), n - B, pool, 4, obs, False)
        # the decode bank holds the longest head the bounds allow (+ what a head grows by), from the ceiling and not from a sync
        grow = m if mode == "encoding" else 1
        assert OneShotBank.handed == [(n + 8, (n - lo + grow + 3) // 4 * 4 + 8, B)]
        dec = [f for f in cache.log if f[2]["phase"] == "decode"]
        assert len(dec) == m and all(f[2]["head_adaptive"] is None and f[2]["pool"] == 1 for f in dec)
        assert res == " ".join(str((n + i) % 16) for i in range(m))
        assert line == (f"KV cache budget ratio: {B / n * 100:.2f}%({B}/{n})" if mode == "encoding" else f"KV Cache Budget ratio {B / (n + m) * 100:.2f}%[{B}/({n}+{m})]")


def test_without_the_key_every_plan_is_the_one_it_was(api):
    n, m = 200, 4
    for mode, policy, pool in (("encoding", "h2o_head", 7), ("auto", "tova", 3), ("encoding", "roco", 1), ("auto", "roco", 1)):
        base = dict(kv_policy=policy, budget=80, max_new_tokens=m, prefill="one_shot", obs_window=16, score_pool=pool)
        ref = _run(api, _model(), n, base, mode)
        handed = list(OneShotBank.handed)
        assert all(f[2]["head_adaptive"] is None for f in ref[1].log)
        for key in (None, "uniform"):
            OneShotBank.handed.clear()
            got = _run(api, _model(), n, dict(base, head_budgets=key, head_budget_floor=0.5), mode)      # (floor / ceiling are read only with the key)
            assert got[0] == ref[0] and got[2] == ref[2] and got[1].log == ref[1].log and OneShotBank.handed == handed[-1:]
    # the strided prefill, with and without an explicit 'uniform'
    strided = dict(kv_policy="roco", budget=80, max_new_tokens=m)
    for mode in ("encoding", "auto"):
        assert _run(api, _model(), n, dict(strided, head_budgets="uniform"), mode)[1].log == _run(api, _model(), n, strided, mode)[1].log
    # a budget that holds the prompt: the key changes nothing
    big = dict(kv_policy="h2o_head", budget=1.0, max_new_tokens=m, prefill="one_shot")
    assert _run(api, _model(), n, dict(big, head_budgets="adaptive"), "encoding")[1].log == _run(api, _model(), n, big, "encoding")[1].log


def test_the_drivers_refusals_fire_before_the_library_is_loaded(api, no_library):
    from types import SimpleNamespace
    gen = dict(kv_policy="h2o_head", budget=80, max_new_tokens=4, prefill="one_shot", head_budgets="adaptive")
    model, ids = _model(), _ids(200)
    cases = [(dict(prefill=None), "encoding", "needs generation_config\\['prefill'\\] = 'one_shot'"), (dict(head_budgets="pyramid"), "encoding", "'uniform' or 'adaptive'"),
             (dict(head_budget_floor=1.5), "encoding", "head_budget_floor"), (dict(head_budget_floor=-0.1), "encoding", "head_budget_floor"),
             (dict(head_budget_ceil=0.5), "encoding", "head_budget_ceil"), (dict(head_budget_ceil="2"), "encoding", "head_budget_ceil"),
             (dict(), "decoding", "serves the modes"), (dict(), "ppl", "serves the modes"), (dict(streaming=True), "encoding", "streaming"),
             (dict(kv_policy="roco", score_pool=1), "encoding", "serves kv_policy 'h2o_head' and 'tova'"), (dict(kv_policy="roco"), "encoding", "no single row to pool"),
             (dict(kv_policy="recency"), "encoding", "scored policy"), (dict(kv_policy="tova", score_pool=1), "encoding", "head-averaged row, the same for every head"),
             (dict(long_rows=True, score_pool=1), "encoding", "long_rows"), (dict(attention_sinks=torch.zeros(2, 4), score_pool=1), "encoding", "attention sinks"),
             (dict(hipgraph=True), "encoding", "hipgraph"), (dict(kv_quant="fp8"), "encoding", "kv_quant"), (dict(score_pool=4), "encoding", "odd integer")]
    for extra, mode, match in cases:
        with pytest.raises(ValueError, match=match):
            api.generate(model, ids, dict(gen, **extra), kv_mode=mode, stride=4)
    with pytest.raises(ValueError, match="generate_batch"):
        api.generate_batch(model, [ids, ids], gen, kv_mode="encoding", stride=4)
    with pytest.raises(ValueError, match="GQA factors up to 8"):
        api.generate(_model(hq=32, h=2), ids, gen, kv_mode="encoding", stride=4)
    with pytest.raises(ValueError, match="at most 64 KV heads"):
        api.generate(_model(hq=65, h=65), ids, gen, kv_mode="encoding", stride=4)
    sharded = _model()
    sharded.layer_shard = SimpleNamespace(rank=0, world=2, begin=0, count=1)
    with pytest.raises(ValueError, match="layer-sharded"):
        api.generate(sharded, ids, gen, kv_mode="encoding", stride=4)
    assert StubCache.made == 0
    # per prompt, before any bank exists: a ceiling past the 6144 slots per head the decode steps take
    with pytest.raises(ValueError, match="6144"):
        api.generate(_model(length=16400), _ids(16000), dict(gen, budget=7000, head_budget_ceil=1.0), kv_mode="encoding", stride=4)
    assert StubCache.made == 0
