"""Deferred decode steps over KV heads of different lengths, without a GPU (include/easykv_hip.h, "heads"): the exports, the
manifest lines, dry runs of the call family (ekv_heads_*) through the C ABI over fake banks (only the HOST copy of the table is read, nothing
is launched), the planner driven over the grid by a stand-alone program under AddressSanitizer + UBSan (tests/plan_heads_main.cpp; the
sanitizer runtimes are linked into the program, which runs as a child process), the engine's table bookkeeping over a stub library, and the
driver's key over stub caches.

What the plans must say: a heads call plans as the _typed call of the same step with n_slots = the ENVELOPE, the largest T = rows + grow + 1
of the host table over the call's layers — over all deferred layers for a deferred call — field for field: n_split, launches, workspace.
The whole-step form plans as that step asked for "the split kernel, then the scorer" (phases = 1 | 2): the family has no one-launch build.
Every refusal leaves zero launches and zero bytes."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMPILERS = [c for c in ("g++", "/opt/rocm/llvm/bin/clang++") if shutil.which(c)]
INFO = ("n_split", "one_launch", "two_pass", "wide", "n_qblocks", "qb_rows", "n_col_parts", "fold_in_kernel", "n_launches", "fused_order")
F16, BF16 = 0, 1
OK, ARG, UNSUPPORTED = 0, -1, -2
CALLS = ("ekv_heads_step_check", "ekv_heads_step_info", "ekv_heads_workspace_bytes", "ekv_heads_step_attend")
U64 = 2 ** 64 - 1
LAYERS = 4


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


def _heads(lib, bank, st, dtype, table, grow=0, null=0):
    """null: 1 the struct, 2 the device pointer, 3 the host copy"""
    from easykv_amd import _lib as L
    host = (ctypes.c_int32 * len(table))(*table)
    desc = None if null == 1 else ctypes.byref(L.Heads(None if null == 2 else 256, None if null == 3 else ctypes.addressof(host), grow))
    return _answers(lib.ekv_heads_step_check, lib.ekv_heads_step_info, lib.ekv_heads_workspace_bytes, bank, st, dtype, desc)


def _refused(got, code=UNSUPPORTED):
    d = dict(zip(INFO, got[2:12]))
    return got[0] == code and got[12] == 0 and (got[1] != 0 or (d["n_launches"] == 0 and d["one_launch"] == 0))


def _step(d=128, hq=8, h=4, rows=128, policy=1, n_evict=1, n_split=2, form=0, cap=None, layers=LAYERS):
    from easykv_amd import _lib as L
    bank = L.Bank(256, 256, 256, 256, 256, 256, layers, hq, h, d, cap or (rows + 64 + 3) // 4 * 4, 256, 256, 256)
    st = L.Step()
    st.layer_count, st.q_len, st.n_slots, st.policy, st.n_evict, st.win_tail = layers, 1, 7, policy, n_evict if policy else 0, 8 if policy == 1 else 0
    st.accumulate, st.roco_tail, st.causal, st.roco_k1, st.range_start, st.n_split, st.count_add, st.sm_div = int(policy != 0), 10, 1, 24, -1, n_split, 1.0, 8.0
    if form:
        st.defer_layers, st.phases = layers, form
        if form == 5:
            st.layer_begin = st.defer_index = 1
            st.layer_count = 1
    return bank, st


def _twin(lib, bank, st, dtype, T):
    """The _typed call the heads call must plan as: n_slots = the envelope, the whole-step form as phases = 1 | 2."""
    from easykv_amd import _lib as L
    tw = L.Step()
    ctypes.memmove(ctypes.byref(tw), ctypes.byref(st), ctypes.sizeof(L.Step))
    tw.n_slots = T
    if tw.phases == 0:
        tw.phases = 3
    return _plain(lib, bank, tw, dtype)


def test_heads_calls_are_exported_and_declared(lib):
    from easykv_amd import _lib as L
    header = open(os.path.join(ROOT, "include", "easykv_hip.h")).read()
    declared = set(re.findall(r"\b(ekv_[a-z0-9_]+)\s*\(", header))
    raw = ctypes.CDLL(L.LIB)
    for name in CALLS:
        assert name in declared and name in L.EXPORTS and hasattr(raw, name), name
    assert lib.ekv_abi_version() == 8
    assert re.search(r"typedef struct ekv_heads \{\s*const int32_t \*rows;\s*const int32_t \*rows_host;\s*int32_t grow;\s*\} ekv_heads;", header)
    for text in ("rows[l][h] + grow + 1", "step->n_slots is IGNORED", "ENVELOPE", "dereference no device pointer", "The call never\n * writes the table"):
        assert text in header, text
    assert lib.ekv_heads_step_check(None, None, F16, None) == ARG
    assert lib.ekv_heads_workspace_bytes(None, None, F16, None) == 0
    # every existing struct is untouched: the table is an argument of the four calls
    assert ctypes.sizeof(L.Step) == 31 * 4 and ctypes.sizeof(L.Seq) == 36 and ctypes.sizeof(L.Heads) == 24


def test_manifest_holds_the_heads_lines():
    from easykv_amd import _build
    later = dict(_build.later_objects())
    decode = [f"ekv_attn_decode_d{d}_heads{e}" for d in (32, 64, 96, 128, 256) for e in ("", "_bf16")]
    score = [f"ekv_decode_score_heads{e}" for e in ("", "_bf16")]
    for name in decode:
        a = later[name]
        assert "-DEKV_HEADS=1" in a and "-DEKV_ROPE=false" in a and "-DEKV_BATCH=1" not in a and a[-1].endswith("ekv_attn_decode.inc"), name
        assert ("-DEKV_BF16=1" in a) == name.endswith("_bf16")
    for name in score:
        assert "-DEKV_HEADS=1" in later[name] and later[name][-1].endswith("ekv_decode_score.inc"), name
    everything = _build.objects() + _build.added_objects() + _build.later_objects()
    assert sorted(n for n, a in everything if "-DEKV_HEADS=1" in a) == sorted(decode + score)
    assert not [n for n, _ in _build.objects() + _build.added_objects() if "_heads" in n]
    assert {"EKV_DECODE_HEADS", "EKV_DECODE_SCORE_HEADS"} <= set(_build.FAMILIES)
    # the switch is spelled next to EKV_BATCH, and refuses what it has no instance of at compile time
    kernels_h = open(os.path.join(ROOT, "easykv_amd", "csrc", "ekv_kernels.h")).read()
    assert "#elif defined(EKV_HEADS) && EKV_HEADS" in kernels_h and "#define EKV_BATCH_TAG _heads" in kernels_h and "EKV_HEADS_ONLY" in kernels_h
    inc = open(os.path.join(ROOT, "easykv_amd", "csrc", "ekv_attn_decode.inc")).read()
    assert re.search(r"#if EKV_HEADS && \(EKV_ROPE \|\| EKV_KV8 .*EKV_BATCH .*EKV_SOFTCAP \|\| EKV_SINK \|\| EKV_WINDOW\)\n#error", inc)


def test_heads_plans_and_refusals_by_name(lib):
    # equal counts: the _typed call of the step the table spells out; the whole-step form never the one-launch kernel
    for form in (0, 5, 8):
        for n_split in (1, 3):
            bank, st = _step(form=form, n_split=n_split)
            got = _heads(lib, bank, st, F16, [128] * (LAYERS * 4))
            assert got[0] == OK and got == _twin(lib, bank, st, F16, 129), (form, n_split, got)
            assert got[3] == 0
    bank, st = _step(n_split=1)
    st.n_slots = 129
    assert _plain(lib, bank, st, F16)[3] == 1      # (the plain whole step of this shape IS one launch)
    # a ragged table: the envelope, over the call's layers ...
    table = [40, 64, 97, 128] + [128, 20, 20, 50] + [30] * 8
    for lb, lc, want in ((0, 1, 129), (1, 1, 129), (2, 2, 31), (0, 4, 129)):
        bank, st = _step()
        st.layer_begin, st.layer_count = lb, lc
        got = _heads(lib, bank, st, F16, table)
        assert got[0] == OK and got == _twin(lib, bank, st, F16, want), (lb, lc, got)
    # ... and over ALL deferred layers for a deferred call, whichever layer it launches; `grow` counts
    table = [30] * 12 + [40, 64, 97, 700]
    for form in (5, 8):
        bank, st = _step(rows=900, form=form)
        assert _heads(lib, bank, st, BF16, table, grow=2) == _twin(lib, bank, st, BF16, 703)
        assert _heads(lib, bank, st, BF16, table, grow=2) != _twin(lib, bank, st, BF16, 33)
    # any number of KV heads: 66 are past the by-value table of the batched call, not past this one
    bank, st = _step(d=64, hq=66, h=66, rows=32, form=8)
    got = _heads(lib, bank, st, F16, [32] * (LAYERS * 66))
    assert got[0] == OK and got == _twin(lib, bank, st, F16, 33)
    # the refusals, each on a step the family takes
    table = [40, 64, 97, 700] * LAYERS

    def refuse(form=0, **kw):
        bank, st = _step(rows=700, form=form)
        for k, v in kw.items():
            setattr(bank if k in ("n_q_heads", "cap") else st, k, v)
        return _heads(lib, bank, st, F16, table)
    assert refuse()[0] == OK
    for form in (0, 5, 8):
        for kw in (dict(q_len=2), dict(rope_on_read=1), dict(phases=(form or 0) | 16), dict(policy=3, tova_head_mean=1), dict(n_evict=2), dict(n_q_heads=64)):
            assert _refused(refuse(form, **kw)), (form, kw)
    for form in (0, 8):      # scored shapes only the generic scorer serves, and the range compaction: where the call's launches hold the scorer
        assert _refused(refuse(form, cap=766)), form
        assert _refused(refuse(form, policy=4, range_start=4)), form
        bank, st = _step(rows=6200, form=form)
        assert _refused(_heads(lib, bank, st, F16, [6200] * 16)), form
    # argument errors: nothing planned, nothing counted
    bank, st = _step(rows=700)
    for kw in (dict(null=1), dict(null=2), dict(null=3), dict(grow=-1)):
        assert _refused(_heads(lib, bank, st, F16, table, **kw), ARG), kw
    assert _refused(_heads(lib, bank, st, F16, [40, 0, 97, 700] * LAYERS), ARG), "a count < 1"
    assert _refused(_heads(lib, bank, st, F16, table, grow=64), ARG), "T > cap"
    assert _heads(lib, bank, st, F16, table, grow=63)[0] == OK
    assert _refused(_heads(lib, bank, st, F16, [1, 64, 97, 700] * LAYERS), ARG), "a head with no candidate outside the protected tail"
    assert lib.ekv_heads_step_check(ctypes.byref(bank), ctypes.byref(st), 2, None) == ARG
    bank, st = _step(rows=700, form=5)
    st.layer_begin, st.defer_index = 2, 3      # deferred layers -1 .. 2
    assert _refused(_heads(lib, bank, st, F16, table), ARG)


# ---- the planner as a stand-alone program under the sanitizers ---------------------------------------------------------------------------
@pytest.fixture(scope="module", params=COMPILERS or [None], ids=lambda c: os.path.basename(c) if c else "none")
def program(request, tmp_path_factory):
    if request.param is None:
        pytest.skip("no host C++ compiler on this machine")
    exe = str(tmp_path_factory.mktemp("plan_heads") / "plan_heads_main")
    static = ["-static-libasan", "-static-libubsan"] if os.path.basename(request.param) == "g++" else []
    cmd = [request.param, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", *static,
           "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", os.path.join(ROOT, "tests", "plan_heads_main.cpp"),
           os.path.join(ROOT, "easykv_amd", "csrc", "ekv_plan.cpp"), "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    return exe


def _table(kind, h, rows):
    """The table plan_heads_main.cpp builds for `kind` (0 equal counts, 1 ragged)."""
    t = [rows] * (LAYERS * h)
    if kind == 1:
        for l in range(LAYERS):
            for hh in range(h):
                if not (l == LAYERS - 1 and hh == h - 1):
                    t[l * h + hh] = max(40, rows - 1 - (l * 37 + hh * 101) % rows)
    return t


def test_heads_planner_grid_ends_clean_and_answers_as_the_library(program, lib):
    r = subprocess.run([program], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-4000:])      # (a sanitizer report ends the program with a non-zero status)
    lines = r.stdout.splitlines()
    assert len(lines) > 10000
    n = dict(as_twin=0, equal=0, ragged=0, whole=0, layer_call=0, flush=0, bf16=0, heads66=0, refused=0, arg=0, flush_only=0)
    bad = []
    for i, ln in enumerate(lines):
        left, right = ln.split("=>")
        mine, twin = right.split("|")
        (d, hq, h, layers, cap, q_len, T, policy, n_evict, rope, n_split, dtype, head_mean, phases, defer_layers, grow, kind) = (int(x) for x in left.split())
        got, ref = [int(x) for x in mine.split()], [int(x) for x in twin.split()]
        assert len(got) == 13 and len(ref) == 12 and layers == LAYERS
        ref = [ref[0], 0] + ref[1:]      # (in the layout of `got`: check, info rc, ten fields, bytes)
        form = phases & ~16
        if kind in (0, 1) and dtype in (F16, BF16) and i % 5 == 0:      # the library gives the same answers
            bank, st = _step(d, hq, h, T - grow - 1, policy, n_evict, n_split, form, cap)
            st.q_len, st.rope_on_read, st.tova_head_mean, st.phases, st.policy, st.n_evict = q_len, rope, head_mean, phases, policy, n_evict
            st.range_start = 4 if policy == 4 else -1
            want = _heads(lib, bank, st, dtype, _table(kind, h, T - grow - 1), grow)
            if [x & U64 for x in want] != [x & U64 for x in got]:
                bad.append((ln, want))
        scorer_in_call = form != 5      # (the layer call launches attention + fold: what only the scorer refuses is the flush's to refuse)
        if kind >= 2 or dtype not in (F16, BF16):
            assert _refused(got, ARG), ln
            n["arg"] += 1
        elif q_len != 1 or rope or phases & 16 or head_mean or n_evict > 1 or hq // h > 8:
            assert _refused(got), ln
            n["refused"] += 1
        elif scorer_in_call and policy != 0 and (policy == 4 or T > 6144 or cap % 4):
            assert _refused(got), ln
            n["refused"] += 1
            n["flush_only"] += form == 8
        else:
            assert got[0] == OK and ref[0] == OK and got == ref, ln
            assert got[2 + INFO.index("one_launch")] == 0 and (n_split == 0 or got[2] == min(n_split, (T + 127) // 128)), ln
            n["as_twin"] += 1
            n["equal"] += kind == 0
            n["ragged"] += kind == 1
            n["whole"] += form == 0
            n["layer_call"] += form == 5
            n["flush"] += form == 8
            n["bf16"] += dtype == BF16
            n["heads66"] += h == 66
    assert not bad, bad[:3]
    assert all(v > 0 for v in n.values()), n
    print(f"[heads] planner grid: {n}")


# ---- the engine's table over a stub library ----------------------------------------------------------------------------------------------
class _Lib:
    """Counts the family's calls; every dry run says OK, 4096 bytes, n_split 2."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*a):
            self.calls.append(name)
            if name.endswith("step_info"):
                a[-2][0] = 2
            return 4096 if name.endswith("workspace_bytes") else 0
        call.__name__ = name
        return call


def _stub_bank(L=3, H=4, head_slots=None, n_slots=None):
    from easykv_amd import engine
    bank = engine.KVBank.__new__(engine.KVBank)
    bank.lib = _Lib()
    bank.n_layers, bank.n_kv_heads, bank.n_q_heads, bank.head_dim, bank.cap, bank.device, bank.dtype = L, H, 2 * H, 64, 512, "cpu", torch.float16
    bank._dt, bank._bank, bank._heads, bank.head_table_uploads, bank._defer, bank._ws = 0, ctypes.c_int32(0), None, 0, None, None
    bank.head_slots, bank.n_slots = head_slots, n_slots or [max(r) if r is not None else 100 for r in head_slots]
    bank.extent, bank._tokens, bank._slot_rows, bank._score_done = [0] * L, [0] * L, [False] * L, [None] * L
    bank.sm_scale, bank.logit_cap, bank.sinks, bank.windows, bank.long_rows, bank._fmt = None, None, None, None, False, None
    bank._stream = lambda: None
    return bank


def test_engine_keeps_the_table_and_routes_deferred_ragged_steps():
    from easykv_amd import engine
    from easykv_amd._lib import EkvError
    bank = _stub_bank(head_slots=[[40, 64, 97, 128], None, [128, 20, 20, 50]])
    grow_plan = engine.StepPlan(policy="h2o_head", phase="decode", evict=False, budget=32, n_split=2)
    evict_plan = engine.StepPlan(policy="h2o_head", phase="decode", evict=True, budget=32, n_split=2)
    q, kv = torch.zeros(1, 8, 1, 64, dtype=torch.float16), torch.zeros(1, 4, 1, 64, dtype=torch.float16)

    def token(plan):
        for l in range(3):
            out, ids = bank.attend(plan, q, kv, kv, layer_begin=l, defer=True)
            assert tuple(out.shape) == (1, 8, 1, 64) and ids is None
        return bank.flush()
    assert token(grow_plan) is None
    h = bank._heads
    # one upload; a layer without head_slots counts as uniform lengths; the device table and the host copy agree
    assert bank.head_table_uploads == 1 and list(h["host"]) == [40, 64, 97, 128, 100, 100, 100, 100, 128, 20, 20, 50] == h["dev"].flatten().tolist()
    assert bank.head_slots == [[41, 65, 98, 129], [101] * 4, [129, 21, 21, 51]] and bank.n_slots == [129, 101, 129] and bank._tokens == [1, 1, 1]
    assert h["desc"].grow == 1 and bank.extent == [129, 101, 129]
    assert bank.lib.calls.count("ekv_heads_step_attend") == 4 and "ekv_batch_step_attend" not in bank.lib.calls      # three layers and ONE flush
    token(grow_plan)
    assert bank.head_table_uploads == 1 and h["desc"].grow == 2 and list(h["host"])[:4] == [40, 64, 97, 128]      # uniform growth: only `grow` advances
    # evicting steps: every T stays put, neither the table nor its growth moves, ids are [L][H][1]
    for _ in range(3):
        ids = token(evict_plan)
        assert tuple(ids.shape) == (3, 4, 1) and ids.dtype == torch.int32
    assert bank.head_table_uploads == 1 and h["desc"].grow == 2 and bank.head_slots[0] == [42, 66, 99, 130]
    checks = bank.lib.calls.count("ekv_heads_step_check")
    ids2 = token(evict_plan)
    assert bank.lib.calls.count("ekv_heads_step_check") == checks + 1      # what is constant over a token step is resolved once per step
    assert ids2 is not ids and ids2.data_ptr() != ids.data_ptr()      # a caller may keep a step's ids across tokens
    # lengths that changed in any other way: the table is written anew
    bank.head_slots[1] = [90, 80, 70, 60]
    token(evict_plan)
    assert bank.head_table_uploads == 2 and h["desc"].grow == 0 and list(h["host"])[4:8] == [90, 80, 70, 60]
    # growths that differ between layers likewise
    bank.head_slots[2] = [x + 1 for x in bank.head_slots[2]]
    token(grow_plan)
    assert bank.head_table_uploads == 3
    # uniform growth from outside (every head of every layer one longer): only `grow`
    bank.head_slots = [[x + 1 for x in r] for r in bank.head_slots]
    token(grow_plan)
    assert bank.head_table_uploads == 3 and h["desc"].grow == 3      # (1 from the step above, 1 from outside, 1 from this step)
    # flush() with a layer missing, and a second step before the flush: both raise
    bank.attend(grow_plan, q, kv, kv, layer_begin=0, defer=True)
    with pytest.raises(EkvError, match="1 of 3 layers attended"):
        bank.flush()
    with pytest.raises(EkvError, match="previous step was not flushed"):
        bank.attend(evict_plan, q, kv, kv, layer_begin=1, defer=True)
    bank.attend(grow_plan, q, kv, kv, layer_begin=1, defer=True)
    bank.attend(grow_plan, q, kv, kv, layer_begin=2, defer=True)
    with pytest.raises(EkvError, match="previous step was not flushed"):
        bank.attend(grow_plan, q, kv, kv, layer_begin=0, defer=True)
    bank.flush()
    # anything but a plain decode plan keeps raising on ragged layers
    chunk = engine.StepPlan(policy="h2o_head", phase="prefill", accumulate=True, evict=True, budget=64, stride=8)
    q8, kv8 = torch.zeros(1, 8, 8, 64, dtype=torch.float16), torch.zeros(1, 4, 8, 64, dtype=torch.float16)
    for plan, args in ((chunk, (q8, kv8, kv8)), (engine.StepPlan(policy="h2o_head", phase="decode", pool=3), (q, kv, kv)),
                       (engine.StepPlan(policy="h2o_head", phase="decode", streaming=True), (q, kv, kv))):
        with pytest.raises(EkvError, match="different numbers of rows"):
            bank.attend(plan, *args, layer_begin=0, defer=True)
    # reset() forgets the table's contents, not the counter
    bank.lib.ekv_bank_reset = lambda *a: 0
    bank._slot_min_tail, bank._slot_stretch = [0] * 3, 0
    bank.reset()
    assert bank.head_slots is None and bank._heads["base"] is None and bank.head_table_uploads == 3


# ---- the driver: the cache's routing over a recording bank, the key over stub caches -------------------------------------------------------
class _RecBank:
    def __init__(self, L, head_slots):
        self.n_layers, self.head_slots, self.calls, self.dtype = L, head_slots, [], torch.float16

    def ragged(self, layer):
        return self.head_slots is not None and self.head_slots[layer] is not None

    def abort_step(self):
        return 0

    def attend(self, plan, q, k, v, layer_begin=0, defer=False, out=None, evict_ids=None):
        self.calls.append(("attend", layer_begin, defer))
        return torch.zeros_like(q), (torch.zeros(1, 2, 1, dtype=torch.int32) if not defer and plan.evict else None)

    def flush(self):
        self.calls.append(("flush",))
        return torch.zeros(self.n_layers, 2, 1, dtype=torch.int32)


def _rec_cache(L, head_slots, head_decode=None, record=True):
    from easykv_amd import api
    cache = api.BudgetedKVCache.__new__(api.BudgetedKVCache)
    cache.layer_begin, cache.layer_count, cache.bank, cache.record, cache.evictions = 0, L, _RecBank(L, head_slots), record, []
    cache.score_prefix, cache.defer_chunk_scorer, cache.head_decode, cache._cur = False, True, head_decode, None
    return cache


def test_the_cache_sends_ragged_decode_layers_through_the_deferred_call_only_with_the_key():
    from easykv_amd import engine
    plan = engine.StepPlan(policy="h2o_head", phase="decode", evict=True, budget=32)
    q, kv = torch.zeros(1, 4, 1, 32, dtype=torch.float16), torch.zeros(1, 2, 1, 32, dtype=torch.float16)
    ragged = [[5, 9], None, [7, 7]]
    # without the key: today's routing — the view call, whole, on ragged layers; the uniform deferred call on the others
    for key in (None, "view"):
        cache = _rec_cache(3, [list(r) if r else None for r in ragged], key)
        cache.begin_forward(plan)
        for l in range(3):
            cache.attend(l, q, kv, kv)
        assert cache.bank.calls == [("attend", 0, False), ("attend", 1, True), ("attend", 2, False)], key
    # with the key: one deferred attend per layer and one flush, whose ids are recorded per layer
    cache = _rec_cache(3, ragged, "deferred")
    for _ in range(2):
        cache.bank.calls.clear()
        cache.begin_forward(plan)
        for l in range(3):
            cache.attend(l, q, kv, kv)
        assert cache.bank.calls == [("attend", 0, True), ("attend", 1, True), ("attend", 2, True), ("flush",)]
    assert len(cache.evictions) == 2 and all(len(e) == 3 and tuple(e[0].shape) == (2, 1) for e in cache.evictions)
    # a bank whose heads are all alike is not touched by the key
    cache = _rec_cache(3, None, "deferred")
    cache.begin_forward(plan)
    for l in range(3):
        cache.attend(l, q, kv, kv)
    assert cache.bank.calls == [("attend", 0, True), ("attend", 1, True), ("attend", 2, True), ("flush",)]


from tests.test_oneshot_cpu import OneShotBank, StubCache, _ids, _model, _run, api      # noqa: E402,F401  (`api` is a fixture)


@pytest.fixture
def no_library(monkeypatch):
    """The shared library must not be touched: a refusal of the driver comes before the first bank, and so before the library is loaded."""
    from easykv_amd import _lib

    def load():
        raise AssertionError("_lib.load() was called")
    monkeypatch.setattr(_lib, "load", load)


def test_the_key_marks_the_cache_and_changes_no_plan(api):
    n, m = 200, 4
    for mode, policy, pool in (("encoding", "h2o_head", 7), ("auto", "tova", 3)):
        base = dict(kv_policy=policy, budget=80, max_new_tokens=m, prefill="one_shot", obs_window=16, score_pool=pool, head_budgets="adaptive")
        ref = _run(api, _model(), n, base, mode)
        handed = list(OneShotBank.handed)
        assert getattr(ref[1], "head_decode", None) is None
        for key in (None, "view", "deferred"):
            OneShotBank.handed.clear()
            got = _run(api, _model(), n, dict(base, head_decode=key), mode)
            assert got[0] == ref[0] and got[2] == ref[2] and got[1].log == ref[1].log and OneShotBank.handed == handed[-1:], key
            assert getattr(got[1], "head_decode", None) == ("deferred" if key == "deferred" else None)


def test_the_key_without_adaptive_head_budgets_raises_before_the_library_is_loaded(api, no_library):
    model, ids = _model(), _ids(200)
    gen = dict(kv_policy="h2o_head", budget=80, max_new_tokens=4, prefill="one_shot")
    for extra, match in ((dict(head_decode="deferred"), "needs generation_config\\['head_budgets'\\] = 'adaptive'"),
                         (dict(head_decode="view", head_budgets="uniform"), "needs generation_config\\['head_budgets'\\] = 'adaptive'"),
                         (dict(head_decode="eager", head_budgets="adaptive"), "'view' or 'deferred'")):
        with pytest.raises(ValueError, match=match):
            api.generate(model, ids, dict(gen, **extra), kv_mode="encoding", stride=4)
    with pytest.raises(ValueError, match="head_budgets"):
        api.generate(model, ids, dict(kv_policy="roco", budget=80, max_new_tokens=4, head_decode="deferred"), kv_mode="auto", stride=4)
    assert StubCache.made == 0
