"""One-shot prompt compression and pooled selection without a GPU: the exports, dry runs of the pooled call family (ekv_pool_*) through
the C ABI over fake banks (nothing is dereferenced, nothing is launched), the planner driven over a pooled grid by a stand-alone program
under AddressSanitizer + UBSan (tests/plan_pool_main.cpp; the sanitizer runtimes are linked into the program, which runs as a child
process), the new manifest lines, the engine's routing, and the driver over stub caches in the manner of tests/test_driver_cpu.py.

What the plans must say: a pooled step plans as the plain call of the same step with every in-kernel scorer tail off —
for a chunk step that is the plain call asked for "attention, then the scorer" (phases = 1 | 2): the same tiling, scheme, launches and
workspace, never one launch; every refusal leaves zero launches and zero bytes."""
import contextlib
import ctypes
import dataclasses
import io
import os
import re
import shutil
import subprocess

import pytest
import torch

from tests.test_dispatch_table import _case, _chunk, _structs
from tests.test_driver_cpu import StubBank, StubCache, _ids

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMPILERS = [c for c in ("g++", "/opt/rocm/llvm/bin/clang++") if shutil.which(c)]
INFO = ("n_split", "one_launch", "two_pass", "wide", "n_qblocks", "qb_rows", "n_col_parts", "fold_in_kernel", "n_launches", "fused_order")
F16, BF16 = 0, 1
OK, ARG, UNSUPPORTED = 0, -1, -2
CALLS = ("ekv_pool_step_check", "ekv_pool_step_info", "ekv_pool_workspace_bytes", "ekv_pool_step_attend")
U64 = 2 ** 64 - 1


@pytest.fixture(scope="module")
def lib():
    from easykv_amd import _build, _lib
    if not os.path.exists(_build.LIB):
        _build.build_lib()
    return _lib.load()


def _plain(lib, bank, st, dtype):
    b, s = ctypes.byref(bank), ctypes.byref(st)
    info = (ctypes.c_int32 * 10)(*([-7] * 10))
    return [lib.ekv_step_check_typed(b, s, dtype), lib.ekv_step_info_typed(b, s, dtype, info, 10)] + list(info) + [lib.ekv_workspace_bytes_typed(b, s, dtype)]


def _pool(lib, bank, st, dtype, radius=3, op=0, null=False):
    from easykv_amd import _lib as L
    b, s = ctypes.byref(bank), ctypes.byref(st)
    p = None if null else ctypes.byref(L.Pool(radius, op))
    info = (ctypes.c_int32 * 10)(*([-7] * 10))
    return [lib.ekv_pool_step_check(b, s, dtype, p), lib.ekv_pool_step_info(b, s, dtype, p, info, 10)] + list(info) + [lib.ekv_pool_workspace_bytes(b, s, dtype, p)]


def _refused(got, code=UNSUPPORTED):
    """The pooled call's answer is `code`, with zero launches and zero bytes."""
    d = dict(zip(INFO, got[2:12]))
    return got[0] == code and got[12] == 0 and (got[1] != 0 or (d["n_launches"] == 0 and d["one_launch"] == 0))


def test_pool_calls_are_exported_and_declared(lib):
    from easykv_amd import _lib as L
    header = open(os.path.join(ROOT, "include", "easykv_hip.h")).read()
    declared = set(re.findall(r"\b(ekv_[a-z0-9_]+)\s*\(", header))
    raw = ctypes.CDLL(L.LIB)
    for name in CALLS:
        assert name in declared and name in L.EXPORTS and hasattr(raw, name), name
    assert lib.ekv_abi_version() == 8
    assert re.search(r"typedef struct ekv_pool \{\s*int32_t radius;\s*int32_t op;\s*\} ekv_pool;", header)
    assert "#define EKV_POOL_MAX 0" in header and "#define EKV_POOL_AVG 1" in header and (L.POOL_OPS["max"], L.POOL_OPS["avg"]) == (0, 1)
    for text in ("max_pool1d(s[R], 2r+1, stride=1, padding=r)", "avg_pool1d(s[R], 2r+1, stride=1, padding=r)", "count_include_pad=True",
                 "lowest logical index", "One-shot prefill"):
        assert text in header, text
    # argument checks come before any device access
    assert lib.ekv_pool_step_check(None, None, F16, None) == ARG
    assert lib.ekv_pool_workspace_bytes(None, None, F16, None) == 0
    # ekv_step is untouched (tests/test_host_cpu.py pins it): the pooling is an argument of the four calls
    assert ctypes.sizeof(L.Step) == 31 * 4 and ctypes.sizeof(L.Pool) == 8


def test_manifest_holds_the_pooled_scorer_lines():
    from easykv_amd import _build
    later = dict(_build.later_objects())
    names = [f"ekv_score_select_pool_nt{nt}{e}" for nt in (512, 1024) for e in ("", "_bf16")]
    for name in names:
        assert name in later and "-DEKV_POOL=1" in later[name] and later[name][-1].endswith("ekv_score_select.inc"), name
    assert "-DEKV_SS_NT=1024" in later["ekv_score_select_pool_nt1024_bf16"] and "-DEKV_BF16=1" in later["ekv_score_select_pool_nt1024_bf16"]
    everything = _build.objects() + _build.added_objects() + _build.later_objects()
    assert sorted(n for n, a in everything if "-DEKV_POOL=1" in a) == sorted(names)
    assert not [n for n, _ in _build.objects() + _build.added_objects() if "pool" in n]
    fams = [f for f, _ in _build.later_instances() if "POOL" in f]
    assert fams == ["EKV_SCORE_SELECT_POOL"] * 4 and "EKV_SCORE_SELECT_POOL" in _build.FAMILIES


def test_pooled_plans_and_refusals_by_name(lib):
    # a one-shot observation step of a 7B-shaped model: 32 queries over 4096 keys, half of them evicted; 32 layers at once and one layer
    for layers in (32, 1):
        c = _chunk(layers, 32, 32, 32, 4064, policy=1, n_evict=2048, win_lo=4, win_tail=32)
        bank, st = _structs(c)
        got, plain0 = _pool(lib, bank, st, F16), _plain(lib, bank, st, F16)
        st.phases = 3
        ref = _plain(lib, bank, st, F16)
        assert got[0] == OK and plain0[0] == OK and got == ref, (layers, got, ref)
        d = dict(zip(INFO, got[2:12]))
        assert d["one_launch"] == 0 and d["n_launches"] >= 2 and got[12] > 0, d
    # steps whose plain call is ONE launch (logits in LDS; the logits-resident kernel; the 16x16 kernel's scorer tail) or ends in the wide
    # column-sum pass's tail: the pooled call is the attention launches + the generic scorer
    for c, what in ((_chunk(32, 32, 32, 8, 2056, policy=1), "lds"), (_chunk(32, 32, 8, 16, 1232, policy=1), "resident"),
                    (_chunk(32, 32, 32, 96, 5002, policy=1), "wide tail"), (_chunk(2, 16, 2, 4, 200, d=64, n_split=1, policy=3), "16x16 tail")):
        bank, st = _structs(c)
        plain0, got = _plain(lib, bank, st, F16), _pool(lib, bank, st, F16, 1, 1)
        st.phases = 3
        ref = _plain(lib, bank, st, F16)
        pd, gd = dict(zip(INFO, plain0[2:12])), dict(zip(INFO, got[2:12]))
        assert plain0[0] == OK and got[0] == OK and got == ref, (what, got, ref)
        assert gd["one_launch"] == 0 and (pd["one_launch"] == 1 or pd["n_launches"] <= gd["n_launches"]), (what, pd, gd)
    # a decode step: never the one-launch kernel
    bank, st = _structs(_case(n_layers=32, policy=1, win_tail=600))
    assert _plain(lib, bank, st, F16)[3] == 1
    got = _pool(lib, bank, st, F16)
    assert got[0] == OK and got[3] == 0 and got[10] >= 2, got
    # the refusals, each a step the plain call takes: roco, recency / random, no policy, RoPE-on-read, the head-mean TOVA row,
    # slot-indexed score rows; past the generic scorer's width (also refused by the plain call)
    base = dict(policy=1, n_evict=1000, win_lo=4, win_tail=32)
    refusals = [_chunk(2, 8, 8, 32, 2000, **dict(base, policy=2)), _chunk(2, 8, 8, 32, 2000, **dict(base, policy=4, range_start=4)),
                _chunk(2, 8, 8, 32, 2000, **dict(base, policy=0, n_evict=0, accumulate=0)), _chunk(2, 8, 8, 32, 2000, rope_on_read=1, **base),
                _chunk(2, 8, 8, 32, 2000, **dict(base, policy=3, tova_head_mean=1))]
    for c in refusals:
        bank, st = _structs(c)
        assert _plain(lib, bank, st, F16)[0] == OK, c
        assert _refused(_pool(lib, bank, st, F16)), c
    bank, st = _structs(_case(n_layers=32, phases=16, phys_extent=2112, policy=1, win_tail=0))
    assert _refused(_pool(lib, bank, st, F16)), "slot rows"
    bank, st = _structs(_chunk(1, 1, 1, 8, 38392, d=64, **dict(base, n_evict=20000, win_tail=8)))
    assert _refused(_pool(lib, bank, st, F16)) and _plain(lib, bank, st, F16)[0] == UNSUPPORTED
    bank, st = _structs(_chunk(1, 1, 1, 8, 38360, d=64, **dict(base, n_evict=20000, win_tail=8)))
    assert _pool(lib, bank, st, F16)[0] == OK
    # argument errors: a NULL struct, radius 0 (kernel size 1 is the plain call's business), an unknown op, an unknown element type
    bank, st = _structs(_chunk(2, 8, 8, 32, 2000, **base))
    assert _pool(lib, bank, st, F16)[0] == OK
    for kw in (dict(null=True), dict(radius=0), dict(radius=-1), dict(op=2), dict(op=-1)):
        assert _refused(_pool(lib, bank, st, F16, **kw), ARG), kw
    assert lib.ekv_pool_step_check(ctypes.byref(bank), ctypes.byref(st), 2, None) == ARG


# ---- the planner as a stand-alone program under the sanitizers ---------------------------------------------------------------------------
@pytest.fixture(scope="module", params=COMPILERS or [None], ids=lambda c: os.path.basename(c) if c else "none")
def program(request, tmp_path_factory):
    if request.param is None:
        pytest.skip("no host C++ compiler on this machine")
    exe = str(tmp_path_factory.mktemp("plan_pool") / "plan_pool_main")
    static = ["-static-libasan", "-static-libubsan"] if os.path.basename(request.param) == "g++" else []
    cmd = [request.param, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", *static,
           "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", os.path.join(ROOT, "tests", "plan_pool_main.cpp"),
           os.path.join(ROOT, "easykv_amd", "csrc", "ekv_plan.cpp"), "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    return exe


def test_pool_planner_grid_ends_clean_and_answers_as_the_library(program, lib):
    from easykv_amd import _lib as L
    r = subprocess.run([program], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-4000:])      # (a sanitizer report ends the program with a non-zero status)
    lines = r.stdout.splitlines()
    assert len(lines) > 5000
    n = dict(chunk_same=0, decode_ok=0, refused=0, arg=0, wide=0, two_pass=0, one_pass=0, big=0, deferred=0, plain_one_launch=0)
    bad = []
    for ln in lines:
        left, right = ln.split("=>")
        pooled, plain = right.split("|")
        (d, hq, h, layers, cap_rows, q_len, T, policy, n_evict, win_lo, win_tail, roco_k1, rope, n_split, two_pass, dtype, head_mean, phases,
         radius, op, null) = (int(x) for x in left.split())
        got, ref = [int(x) for x in pooled.split()], [int(x) for x in plain.split()]
        assert len(got) == 13 and len(ref) == 12
        deferred = phases in (5, 8)
        if dtype in (F16, BF16):      # the library gives the same answers (the program's plain call runs with phases = 1 | 2 where the pooled has 0)
            bank = L.Bank(256, 256, 256, 256, 256, 256, layers, hq, h, d, cap_rows, 256, 256, 256)
            st = L.Step()
            st.layer_count, st.q_len, st.n_slots, st.policy, st.n_evict, st.win_lo, st.win_tail, st.roco_k1 = layers, q_len, T, policy, n_evict, win_lo, win_tail, roco_k1
            st.range_start, st.rope_on_read, st.n_split, st.two_pass, st.roco_tail, st.causal, st.sm_div = (4 if policy == 4 else -1), rope, n_split, two_pass, 10, 1, 8.0
            st.tova_head_mean, st.phases, st.accumulate = head_mean, phases, int(policy != 0)
            st.count_add, st.count_tail_step = float(q_len), -1.0
            if deferred:
                st.defer_layers = 4
                if phases == 5:
                    st.layer_begin = st.defer_index = 1
                    st.layer_count = 1
            want = _pool(lib, bank, st, dtype, radius, op, bool(null))
            if phases == 0:
                st.phases = 3
            want_plain = _plain(lib, bank, st, dtype)
            if [x & U64 for x in want] != [x & U64 for x in got] or [x & U64 for x in want_plain[:1] + want_plain[2:]] != [x & U64 for x in ref]:
                bad.append((ln, want, want_plain))
        info, rep = dict(zip(INFO, got[2:12])), hq // h
        if null or radius < 1 or op not in (0, 1) or dtype not in (F16, BF16):
            assert _refused(got, ARG), ln
            n["arg"] += 1
        elif policy not in (1, 3) or rope or head_mean or phases == 16:
            assert _refused(got, got[0]) and got[0] in (UNSUPPORTED, ARG), ln
            n["refused"] += 1
        elif got[0] != OK:      # what the plain call refuses as well: a row past the scorer's width, a GQA factor past a query block
            assert _refused(got, got[0]) and ref[0] == got[0], ln
            n["refused"] += 1
        elif deferred:
            # attention + fold of one layer: the plain call's answers; the flush: the plain call's tiling and workspace (its launches may
            # end in the column-sum pass's tail, the pooled flush ends in the generic scorer)
            same = slice(2, 12) if phases == 5 else slice(2, 10)
            assert ref[0] == OK and got[same] == ref[same.start - 1:same.stop - 1] and got[12] == ref[11] and info["one_launch"] == 0, ln
            assert phases == 5 or info["n_launches"] >= 1, ln
            n["deferred"] += 1
        elif q_len == 1:
            assert info["one_launch"] == 0 and info["n_launches"] >= 2 and got[12] > 0, ln
            n["decode_ok"] += 1
        else:
            assert ref[0] == OK and got[2:12] == ref[1:11] and got[12] == ref[11] > 0, ln
            assert info["one_launch"] == 0 and info["n_launches"] >= 2, ln
            n["chunk_same"] += 1
            n["wide"] += info["wide"]
            n["two_pass"] += info["two_pass"]
            n["one_pass"] += not info["two_pass"]
            n["big"] += T > 12000
    assert not bad, (len(bad), bad[:2])
    print(f"pool planner grid: {len(lines)} calls, {n}")
    assert min(v for k, v in n.items() if k != "plain_one_launch") > 20, n


# ---- the engine's routing (no library call is made: the bank is a shell) ------------------------------------------------------------
def test_engine_routes_by_the_step_and_refuses_by_the_bank():
    from easykv_amd import _lib, engine
    from easykv_amd._lib import EkvError
    plan = engine.StepPlan()
    assert (plan.n_evict, plan.pool, plan.pool_op) == (None, 1, "max")

    class Lib:
        def __getattr__(self, name):
            return name
    bank = engine.KVBank.__new__(engine.KVBank)
    bank.lib, bank._pool_fams, bank._fmt = Lib(), {}, None
    bank._check_fn, bank._info_fn, bank._ws_fn, bank._attend_fn, bank._desc_ref = "c", "i", "w", "a", ()
    assert bank._family(engine.StepPlan()) == ("c", "i", "w", "a", ())
    assert bank._family(None) == ("c", "i", "w", "a", ())
    fam = bank._family(engine.StepPlan(pool=7, pool_op="avg"))
    assert fam[:4] == CALLS and len(fam[4]) == 1
    desc = bank._pool_fams[(3, 1)][5]
    assert (desc.radius, desc.op) == (3, 1) and bank._family(engine.StepPlan(pool=7, pool_op="avg")) is not None and len(bank._pool_fams) == 1
    for bad in (0, 2, 4, -3, 3.0, "7"):
        with pytest.raises(ValueError, match="kernel size"):
            bank._family(engine.StepPlan(pool=bad))
    with pytest.raises(ValueError, match="pool_op"):
        bank._family(engine.StepPlan(pool=3, pool_op="min"))
    for attr, value, match in (("logit_cap", 30.0, "logit_cap"), ("sinks", torch.zeros(1, 1), "sinks"), ("windows", (0,), "windows"),
                               ("long_rows", True, "long_rows"), ("_fmt", engine.ROW_FORMATS["fp8"], "kv_quant")):
        b2 = engine.KVBank.__new__(engine.KVBank)
        b2.__dict__.update(bank.__dict__)
        setattr(b2, attr, value)
        if attr == "_fmt":
            b2.kv_quant = "fp8"
        with pytest.raises(EkvError, match=match):
            b2._family(engine.StepPlan(pool=3))
        assert b2._family(engine.StepPlan()) == ("c", "i", "w", "a", ())      # (the unpooled step is the bank's own business)
    # make_step: n_evict overrides the stride, and with it roco's feasible set
    bank.n_slots, bank.extent, bank.head_dim, bank.sm_scale = [968], [968], 128, None
    st = bank.make_step(engine.StepPlan(policy="roco", phase="prefill", evict=True, budget=1000, recent=32, sink=4, stride=32, n_evict=936), 32, 0, 1)
    assert (st.n_evict, st.win_lo, st.win_tail, st.roco_k1, st.count_add, st.count_tail_step) == (936, 4, 32, 964, 32.0, -1.0)
    st = bank.make_step(engine.StepPlan(policy="roco", phase="prefill", evict=True, budget=1000, recent=100, sink=4, stride=32), 32, 0, 1)
    assert (st.n_evict, st.roco_k1) == (32, 896)


# ---- the driver over stub caches ---------------------------------------------------------------------------------------------------------
class OneShotBank(StubBank):
    handed = []

    def hand_over(self, cap):
        new = OneShotBank(self.n_layers, self.n_q_heads, self.n_kv_heads, self.head_dim, cap, self.dtype)
        new.n_slots = list(self.n_slots)
        type(self).handed.append((self.cap, cap, self.n_slots[0]))
        return new


class OneShotCache(StubCache):
    def __init__(self, *a, long_rows=False, **kw):
        super().__init__(*a, **kw)
        self.bank = OneShotBank(self.layer_count, self.bank.n_q_heads, self.bank.n_kv_heads, self.bank.head_dim, self.bank.cap, self.bank.dtype)

    def attend(self, layer_idx, q, k, v):
        self.n_attend += 1
        if self.n_attend == self.layer_count:
            n, p = q.shape[2], self.plan
            k_ev = 0 if not p.evict else (1 if p.phase == "decode" else (p.stride if p.n_evict is None else p.n_evict))
            self.bank.n_slots = [self.bank.n_slots[0] + n - k_ev] * self.layer_count
            self.log.append((n, self.positions.view(-1).tolist(), dataclasses.asdict(p)))
        return torch.zeros_like(q)


@pytest.fixture
def api(monkeypatch):
    from easykv_amd import api
    monkeypatch.setattr(api, "BudgetedKVCache", OneShotCache)
    StubCache.made = 0
    OneShotBank.handed = []
    return api


def _model(hq=4, h=4, d=32, length=256):
    from oracle.fake_model import make_streams
    from tests.native_fake_model import NativeFakeModel
    return NativeFakeModel(*make_streams(2, hq, h, d, length, seed=1), device="cpu")


def _run(api, model, n, cfg, mode, stride=4):
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        res, cache = api.generate(model, _ids(n), cfg, kv_mode=mode, stride=stride, return_cache=True)
    return res, cache, buf.getvalue().strip()


@pytest.mark.parametrize("mode,policy,pool", [("encoding", "h2o_head", 7), ("encoding", "roco", 1), ("auto", "tova", 3), ("auto", "roco", 1)])
def test_one_shot_is_two_forwards_and_a_hand_over(api, mode, policy, pool):
    n, B, obs, m = 200, 80, 16, 5
    cfg = dict(kv_policy=policy, budget=B, max_new_tokens=m, prefill="one_shot", obs_window=obs, score_pool=pool, score_pool_op="avg")
    res, cache, line = _run(api, _model(), n, cfg, mode)
    pre = [f for f in cache.log if f[2]["phase"] == "prefill"]
    assert [f[0] for f in pre] == [n - obs, obs] and pre[0][1] == list(range(n - obs)) and pre[1][1] == list(range(n - obs, n))
    a, b = pre[0][2], pre[1][2]
    assert (a["policy"], a["accumulate"], a["evict"], a["pool"]) == ("full", False, False, 1)
    assert (b["policy"], b["accumulate"], b["evict"], b["n_evict"], b["sink"], b["recent"], b["stride"], b["budget"]) == (policy, True, True, n - B, 4, obs, obs, n)
    assert (b["pool"], b["pool_op"], b["tova_head_mean"]) == (pool, "avg", False)      # (the head-averaged row is tova's alone)
    # the cap of both banks: the whole prompt, then what the same mode's strided prefill would have sized
    _, idx, _ = api.geometry(mode, n, B, 4)
    want_cap = (idx + 4 + m if mode == "encoding" else idx + 4 + 1) + 8
    assert OneShotBank.handed == [(n + 8, want_cap, B)] and cache.bank.cap == want_cap
    dec = [f for f in cache.log if f[2]["phase"] == "decode"]
    assert len(dec) == m and [f[1] for f in dec] == [[n + i] for i in range(m)]
    if mode == "encoding":
        assert all(f[2]["policy"] == "full" and not f[2]["evict"] for f in dec)
        assert line == f"KV cache budget ratio: {B / n * 100:.2f}%({B}/{n})" and cache.get_seq_length() == B + m
    else:
        assert all((f[2]["policy"], f[2]["evict"], f[2]["budget"], f[2]["score_off"], f[2]["pool"]) == (policy, True, B, 0, 1) for f in dec)
        assert line == f"KV Cache Budget ratio {B / (n + m) * 100:.2f}%[{B}/({n}+{m})]" and cache.get_seq_length() == B
    assert res == " ".join(str((n + i) % 16) for i in range(m))


def test_the_default_path_is_unchanged_and_a_budget_that_holds_the_prompt_ignores_the_key(api):
    n, m = 200, 4
    base = dict(kv_policy="roco", budget=80, max_new_tokens=m)
    for mode in ("encoding", "auto"):
        ref = _run(api, _model(), n, base, mode)
        got = _run(api, _model(), n, dict(base, prefill=None), mode)
        assert got[0] == ref[0] and got[2] == ref[2] and got[1].log == ref[1].log and not OneShotBank.handed
        assert all(f[2]["n_evict"] is None and f[2]["pool"] == 1 for f in ref[1].log)
        # B >= n: the key changes nothing
        big = dict(base, budget=n if mode == "auto" else 1.0)
        assert _run(api, _model(), n, dict(big, prefill="one_shot", score_pool=1), mode)[1].log == _run(api, _model(), n, big, mode)[1].log
    assert not OneShotBank.handed


def test_one_shot_refusals_come_before_any_cache(api):
    from types import SimpleNamespace
    gen = dict(kv_policy="h2o_head", budget=80, max_new_tokens=4, prefill="one_shot")
    model, ids = _model(), _ids(200)
    cases = [(dict(), "decoding", "serves the modes"), (dict(), "ppl", "serves the modes"), (dict(streaming=True), "encoding", "streaming"),
             (dict(kv_policy="recency"), "encoding", "scored policy"), (dict(kv_policy="random"), "encoding", "scored policy"),
             (dict(kv_policy="roco"), "encoding", "no single row to pool"), (dict(kv_policy="tova"), "encoding", "head-averaged"),
             (dict(prefill="snap"), "encoding", "must be None or 'one_shot'"), (dict(score_pool=4), "encoding", "odd integer"),
             (dict(score_pool=0), "encoding", "odd integer"), (dict(score_pool_op="min"), "encoding", "'max' or 'avg'"),
             (dict(obs_window=0), "encoding", "integer >= 1"), (dict(obs_window=5000), "encoding", "largest\\s+that works is 4096"),
             (dict(long_rows=True), "encoding", "no pooled sink, window, capped or"),
             (dict(attention_sinks=torch.zeros(2, 4)), "encoding", "attention sinks")]
    for extra, mode, match in cases:
        with pytest.raises(ValueError, match=match):
            api.generate(model, ids, dict(gen, **extra), kv_mode=mode, stride=4)
    gqa = _model(hq=16, h=2)      # GQA factor 8: 512 observation queries at most
    with pytest.raises(ValueError, match="largest\\s+that works is 512"):
        api.generate(gqa, ids, dict(gen, obs_window=513), kv_mode="encoding", stride=4)
    capped = _model(d=128)
    capped.config.attn_logit_softcapping = 30.0
    with pytest.raises(ValueError, match="attn_logit_softcapping"):
        api.generate(capped, ids, gen, kv_mode="encoding", stride=4)
    assert StubCache.made == 0
    # per prompt, before the first forward: an observation window the budget cannot hold
    with pytest.raises(ValueError, match="largest that works is 76"):
        api.generate(model, ids, dict(gen, obs_window=100), kv_mode="encoding", stride=4)
    # score_pool = 1 makes no new call: roco, and the models the pooled family refuses, are served
    for extra in (dict(kv_policy="roco"), dict(kv_policy="tova"), dict(long_rows=True)):
        _, cache, _ = _run(api, model, 200, dict(gen, score_pool=1, **extra), "encoding")
        assert cache.log[1][2]["tova_head_mean"] == (extra.get("kv_policy") == "tova")      # (encoding mode's head-averaged TOVA row, unpooled)


def test_generate_batch_takes_the_key(monkeypatch, api):
    from tests.batch_fake_model import BatchFakeModel
    from tests.test_driver_cpu import StubBankBatch, StubCacheBatch
    from oracle.fake_model import make_streams
    monkeypatch.setattr(api, "KVBankBatch", StubBankBatch)
    monkeypatch.setattr(api, "BudgetedKVCacheBatch", StubCacheBatch)
    model = BatchFakeModel(*make_streams(2, 4, 4, 32, 256, seed=1), device="cpu")
    cfg = dict(kv_policy="tova", budget=80, max_new_tokens=4, prefill="one_shot", obs_window=16, score_pool=3)
    lengths = (150, 200, 90)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        res, cache = api.generate_batch(model, [_ids(n) for n in lengths], cfg, kv_mode="auto", stride=4, return_cache=True)
    assert [h[2] for h in OneShotBank.handed] == [80, 80, 80] and [h[0] for h in OneShotBank.handed] == [n + 8 for n in lengths]
    lines = buf.getvalue().strip().split("\n")
    for i, n in enumerate(lengths):
        sres, scache, sline = _run(api, _model(), n, cfg, "auto")
        assert res[i] == sres and lines[i] == sline
        assert cache.logs[i] == [f for f in scache.log if f[2]["phase"] == "decode"]
