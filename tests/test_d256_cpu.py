"""head_dim 256 without a GPU: dry runs of the step family through the C ABI over a fake bank (the pattern of
tests/test_host_cpu.py::_fake_bank_step), the new manifest lines, and the planner driven over a head_dim-256 grid by a stand-alone
program under AddressSanitizer + UBSan (tests/d256_plan_main.cpp; the pattern of tests/test_plan_host_cpu.py — the sanitizer runtimes
are linked into the program, which runs as a child process; nothing is loaded into Python under a sanitizer).

What the plans must say: a 16-bit bank of head_dim 256 with plain keys is served by the decode kernels (one launch in both wave
counts, split with the fast or the generic scorer, batches) and by the 16x16x32 chunk kernel in blocks of at most 32 folded rows —
never by the wide, the logits-in-LDS or the logits-resident kernel; RoPE-on-read and every quantised row format are refused before
a launch."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests.test_dispatch_table import KEYS
from tests.test_host_cpu import _fake_bank_step

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMPILERS = [c for c in ("g++", "/opt/rocm/llvm/bin/clang++") if shutil.which(c)]
SEQ_KEYS = ("layer", "n_slots", "score_off", "n_evict", "win_lo", "win_tail", "roco_k1", "range_start", "phys_extent")
INFO = ("n_split", "one_launch", "two_pass", "wide", "n_qblocks", "qb_rows", "n_col_parts", "fold_in_kernel", "n_launches", "fused_order")
F16, BF16 = 0, 1
OK, UNSUPPORTED = 0, -2


@pytest.fixture(scope="module")
def lib():
    from easykv_amd import _build, _lib
    if not os.path.exists(_build.LIB):
        _build.build_lib()
    return _lib.load()


def _step(**kw):
    """A decode step on a fake head_dim-256 bank (8 KV heads, MHA unless `hq` / `h` say otherwise)."""
    kw.setdefault("hq", 8)
    kw.setdefault("h", 8)
    return _fake_bank_step(head_dim=256, **kw)


def _chunk(n, t_prev, two_pass=0, **kw):
    """An evicting strided chunk step of the encoding rule: n new rows onto t_prev cached ones, roco, sink 4, recent 10 %."""
    T = t_prev + n
    return _step(cap=(T + 64 + 63) // 64 * 64, q_len=n, n_slots=T, n_evict=n, win_lo=4, win_tail=T // 10, roco_k1=max(T - T // 10 - 4, n),
                 count_add=float(n), count_tail_step=-1.0, two_pass=two_pass, **kw)


def _answers(lib, bank, st, dtype=F16):
    """(check, info as a dict, workspace bytes) of the 16-bit call, with the consistency every dry run owes: the three calls and
    ekv_step_plan describe one plan."""
    b, s = ctypes.byref(bank), ctypes.byref(st)
    info = (ctypes.c_int32 * 10)(*([-7] * 10))
    rc = lib.ekv_step_check_typed(b, s, dtype)
    assert lib.ekv_step_info_typed(b, s, dtype, info, 10) == 0
    d = dict(zip(INFO, info))
    nbytes = lib.ekv_workspace_bytes_typed(b, s, dtype)
    if dtype == F16:
        assert lib.ekv_step_check(b, s) == rc and lib.ekv_workspace_bytes(b, s) == nbytes
        ns, fu = ctypes.c_int32(-7), ctypes.c_int32(-7)
        assert lib.ekv_step_plan(b, s, ctypes.byref(ns), ctypes.byref(fu)) == 0
        assert (ns.value, fu.value) == (d["n_split"], d["one_launch"])
    if rc == OK:
        assert d["n_launches"] >= 1 and d["n_split"] >= 1 and nbytes > 0
        assert d["n_launches"] == 1 or not d["one_launch"]
    else:
        assert d["n_launches"] == 0 and d["one_launch"] == 0
    return rc, d, nbytes


def test_decode_steps_plan_at_head_dim_256(lib):
    # one launch, 4-wave build (16 heads in the launch) and 8-wave build (256 heads): nothing split, one kernel
    # (few heads: the caller keeps the heads unsplit, as a layer-per-call model does; 256 heads: the planner's own choice)
    for kw, dtype in ((dict(n_layers=2, n_split=1), F16), (dict(n_layers=2, n_split=1), BF16), (dict(n_layers=32), F16), (dict(n_layers=32), BF16)):
        rc, d, _ = _answers(lib, *_step(**kw), dtype=dtype)
        assert rc == OK and (d["one_launch"], d["n_launches"], d["n_split"], d["wide"]) == (1, 1, 1, 0), (kw, d)
    # few heads left to the planner: key-range splits, attention + the fast scorer
    rc, d, _ = _answers(lib, *_step(n_layers=2))
    assert rc == OK and d["one_launch"] == 0 and d["n_split"] > 1 and d["n_launches"] == 2, d
    # an explicit split: attention + the fast scorer
    rc, d, _ = _answers(lib, *_step(n_split=3))
    assert rc == OK and (d["one_launch"], d["n_split"], d["n_launches"], d["wide"]) == (0, 3, 2, 0), d
    # GQA factor 3 (the padded REP = 4 build) in one launch, in both wave counts; factor 12 (groups of 8, the generic scorer)
    for kw in (dict(n_layers=2, n_split=1), dict(n_layers=32)):
        rc, d, _ = _answers(lib, *_step(hq=24, h=8, **kw))
        assert rc == OK and (d["one_launch"], d["n_launches"]) == (1, 1), (kw, d)
    rc, d, _ = _answers(lib, *_step(hq=48, h=4))
    assert rc == OK and (d["one_launch"], d["n_launches"]) == (0, 2), d
    # the slot-indexed layout, where the planner's rule picks it (ABI 6, EKV_PHASE_SLOT_ROWS = 16)
    rc, d, _ = _answers(lib, *_step(n_layers=32, layer_count=32, phases=16, phys_extent=2112))
    assert rc == OK and d["one_launch"] == 1, d
    # the workspace holds the partials of head_dim 256: [layers][Hq][1][n_split][258] floats
    _, d, nbytes = _answers(lib, *_step(n_split=3))
    assert nbytes >= 2 * 8 * 3 * 258 * 4


def test_chunk_steps_plan_on_the_16x16_kernel_at_head_dim_256(lib):
    for n in (3, 8, 64, 130):
        for two_pass in (1, -1):
            rc, d, _ = _answers(lib, *_chunk(n, 400, two_pass))
            assert rc == OK, (n, two_pass, d)
            # never the wide kernel; blocks of at most 32 folded rows (one 16-row tile per wave); the scheme is the caller's
            assert d["wide"] == 0 and d["qb_rows"] == min(n, 32) and d["n_qblocks"] == -(-n // 32), (n, two_pass, d)
            assert d["two_pass"] == (1 if two_pass == 1 else 0), (n, two_pass, d)
            # one launch only as the one-pass kernel with the scorer as its tail: one block, heads not split, at most 64 rows — a
            # logits-in-LDS or logits-resident step would be one launch under two_pass = 0 alone and needs a smaller head_dim
            if d["one_launch"]:
                assert two_pass == -1 and d["n_qblocks"] == 1 and d["n_split"] == 1 and n <= 32, (n, d)
    for n in (3, 8, 64, 130):      # the planner's own choice of scheme: still neither of the two whole-step kernels
        rc, d, _ = _answers(lib, *_chunk(n, 400, 0, n_layers=32))
        assert rc == OK and d["wide"] == 0, (n, d)
        assert not (d["one_launch"] and d["two_pass"]), (n, d)      # (the logits-resident step reports two_pass = 1, one launch)
    # the same step at head_dim 128 is what those kernels exist for: the refusal above is the head_dim's
    b, s = _chunk(8, 400, 0, n_layers=32)
    b.head_dim, s.sm_div = 128, 128 ** 0.5
    assert _answers(lib, b, s)[1]["one_launch"] == 1
    # GQA: 4 query heads share a block of 8 queries; a factor above 32 does not fit a block and is refused
    rc, d, _ = _answers(lib, *_chunk(16, 400, 1, hq=32, h=8))
    assert rc == OK and (d["qb_rows"], d["n_qblocks"], d["wide"]) == (8, 2, 0), d
    assert _answers(lib, *_chunk(8, 400, 0, hq=40, h=1))[0] == UNSUPPORTED
    # the dense prefix
    rc, d, _ = _answers(lib, *_step(cap=1088, q_len=1000, n_slots=1000, policy=0, n_evict=0, accumulate=0))
    assert rc == OK and (d["wide"], d["qb_rows"], d["n_qblocks"]) == (0, 32, 32), d


def test_refusals_at_head_dim_256_come_before_a_launch(lib):
    from easykv_amd import _lib as L
    # RoPE-on-read: decode and chunk steps
    for bank, st in (_step(rope_on_read=1), _chunk(8, 400, 0, rope_on_read=1), _step(n_layers=32, rope_on_read=1)):
        rc, d, _ = _answers(lib, bank, st)
        assert rc == UNSUPPORTED and d["n_launches"] == 0
    # every quantised row format
    bank, st = _step()
    b, s = ctypes.byref(bank), ctypes.byref(st)
    descs = {"kv8": L.Kv8(256, 256, 256, 256), "kv4": L.Kv4(256, 256, 256, 256), "kv6": L.Kv6(256, 256, 256, 256),
             "kv84": L.Kv84(256, 256, 256, 256), "kv164": L.Kv164(256, 256)}
    tb = (L.Seq * 2)()
    for i in range(2):
        tb[i].layer, tb[i].n_slots, tb[i].n_evict, tb[i].roco_k1, tb[i].range_start = i, st.n_slots, 1, st.roco_k1, -1
    for rows, q in descs.items():
        for dtype in (F16, BF16):
            assert getattr(lib, f"ekv_{rows}_step_check")(b, s, dtype, ctypes.byref(q)) == UNSUPPORTED, rows
            info = (ctypes.c_int32 * 10)(*([-7] * 10))
            assert getattr(lib, f"ekv_{rows}_step_info")(b, s, dtype, ctypes.byref(q), info, 10) == 0
            assert dict(zip(INFO, info))["n_launches"] == 0
            assert getattr(lib, f"ekv_{rows}_batch_step_check")(b, s, dtype, ctypes.byref(q), tb, 2) == UNSUPPORTED, rows
            assert getattr(lib, f"ekv_{rows}_batch_workspace_bytes")(b, s, dtype, ctypes.byref(q), tb, 2) == 0, rows
    # a 16-bit batch table is served, and plans as the two-layer step it spells out
    for dtype in (F16, BF16):
        assert lib.ekv_batch_step_check(b, s, dtype, tb, 2) == OK
        assert lib.ekv_batch_workspace_bytes(b, s, dtype, tb, 2) == lib.ekv_workspace_bytes_typed(b, s, dtype) > 0
        info = (ctypes.c_int32 * 10)(*([-7] * 10))
        assert lib.ekv_batch_step_info(b, s, dtype, tb, 2, info, 10) == 0
        assert list(info)[:9] == [_answers(lib, bank, st, dtype)[1][k] for k in INFO[:9]]
    # head_dims nobody builds stay refused
    for d in (48, 192, 512):
        assert lib.ekv_step_check(*map(ctypes.byref, _fake_bank_step(head_dim=d, hq=8, h=8))) == UNSUPPORTED


def test_manifest_holds_the_head_dim_256_lines():
    from easykv_amd import _build
    later = dict(_build.later_objects())
    names = [f"ekv_attn_decode_d256_plain{b}{e}" for b in ("", "_batch") for e in ("", "_bf16")] + \
            [f"ekv_attn_chunk_d256_m{m}{e}" for m in (0, 1, 2) for e in ("", "_bf16")]
    for name in names:
        assert name in later, name
        assert "-DEKV_D=256" in later[name]
    assert "-DEKV_ROPE=false" in later["ekv_attn_decode_d256_plain"] and "-DEKV_BATCH=1" in later["ekv_attn_decode_d256_plain_batch"]
    assert "-DEKV_CHUNK_MODE=2" in later["ekv_attn_chunk_d256_m2_bf16"] and "-DEKV_BF16=1" in later["ekv_attn_chunk_d256_m2_bf16"]
    # the pinned lists do not know them, and no line of any manifest asks for a RoPE or quantised build at 256
    pinned = [n for n, _ in _build.objects() + _build.added_objects()]
    assert not [n for n in pinned if "d256" in n]
    words = [w for _, w in _build.instances(_build.LATER_MANIFEST) if w and w[0] == "256"]
    assert len(words) == 10 and all("rope" not in w and not any(x.startswith("kv") and x != "kv16" for x in w) for w in words)


# ---- the planner as a stand-alone program under the sanitizers ---------------------------------------------------------------------------
@pytest.fixture(scope="module", params=COMPILERS or [None], ids=lambda c: os.path.basename(c) if c else "none")
def program(request, tmp_path_factory):
    if request.param is None:
        pytest.skip("no host C++ compiler on this machine")
    exe = str(tmp_path_factory.mktemp("d256_plan") / "d256_plan_main")
    static = ["-static-libasan", "-static-libubsan"] if os.path.basename(request.param) == "g++" else []
    cmd = [request.param, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", *static,
           "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", os.path.join(ROOT, "tests", "d256_plan_main.cpp"),
           os.path.join(ROOT, "easykv_amd", "csrc", "ekv_plan.cpp"), "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    return exe


def _library(L, lib, c, dtype, kv8, seqs):
    """The call of one printed line through the C ABI of the library: the row the program prints behind '=>'."""
    bank = L.Bank(256, 256, 256, 256, 256, 256, c["n_layers"], c["hq"], c["h"], c["head_dim"], c["cap"], 256, 256, 256)
    st = L.Step()
    for k in KEYS[9:]:
        if k != "count_add2":
            setattr(st, k, c[k])
    st.count_add, st.count_tail_step, st.sm_div = c["count_add2"] / 2, -1.0 if c["q_len"] > 1 else 0.0, 16.0
    b, s = ctypes.byref(bank), ctypes.byref(st)
    info = (ctypes.c_int32 * 10)(*([-7] * 10))
    plan = [-7, -7, -7]
    q8 = ctypes.byref(L.Kv8(256, 256, 256, 256))
    if seqs is not None:
        tb = (L.Seq * len(seqs))()
        for i, e in enumerate(seqs):
            for k, v in zip(SEQ_KEYS, e):
                setattr(tb[i], k, v)
        if kv8:
            rc = [lib.ekv_kv8_batch_step_check(b, s, dtype, q8, tb, len(seqs)), lib.ekv_kv8_batch_step_info(b, s, dtype, q8, tb, len(seqs), info, 10),
                  lib.ekv_kv8_batch_workspace_bytes(b, s, dtype, q8, tb, len(seqs))]
        else:
            rc = [lib.ekv_batch_step_check(b, s, dtype, tb, len(seqs)), lib.ekv_batch_step_info(b, s, dtype, tb, len(seqs), info, 10),
                  lib.ekv_batch_workspace_bytes(b, s, dtype, tb, len(seqs))]
    elif kv8:
        rc = [lib.ekv_kv8_step_check(b, s, dtype, q8), lib.ekv_kv8_step_info(b, s, dtype, q8, info, 10), lib.ekv_kv8_workspace_bytes(b, s, dtype, q8)]
    else:
        rc = [lib.ekv_step_check_typed(b, s, dtype), lib.ekv_step_info_typed(b, s, dtype, info, 10), lib.ekv_workspace_bytes_typed(b, s, dtype)]
        if dtype == F16:
            ns, fu = ctypes.c_int32(-7), ctypes.c_int32(-7)
            plan = [lib.ekv_step_plan(b, s, ctypes.byref(ns), ctypes.byref(fu)), ns.value, fu.value]
    return [rc[0]] + plan + [rc[1]] + list(info) + [rc[2]]


def test_planner_grid_at_head_dim_256_ends_clean_and_answers_as_the_library(program, lib):
    from easykv_amd import _lib as L
    r = subprocess.run([program], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-4000:])      # (a sanitizer report ends the program with a non-zero status)
    lines = r.stdout.splitlines()
    assert len(lines) > 20000
    n = dict(ok=0, refused=0, one_launch=0, batch=0, chunk=0, rope=0, kv8=0)
    bad = []
    for ln in lines:
        left, right = ln.split("=>")
        v = [int(x) for x in left.split()]
        got = [int(x) for x in right.split()]
        c = dict(zip(KEYS, v[:len(KEYS)]))
        dtype, kv8, nulls, batch, n_seq = v[len(KEYS):len(KEYS) + 5]
        assert c["head_dim"] == 256 and nulls == 0 and len(got) == 16
        rest = v[len(KEYS) + 5:]
        seqs = [rest[9 * i:9 * i + 9] for i in range(n_seq)] if batch else None
        assert len(rest) == (9 * n_seq if batch else 0)
        want = _library(L, lib, c, dtype, kv8, seqs)
        if [x & (2 ** 64 - 1) for x in want] != [x & (2 ** 64 - 1) for x in got]:
            bad.append((c, dtype, kv8, batch, want, got))
        info = dict(zip(INFO, got[5:15]))
        # what holds for every call of the grid, whatever its shape
        assert info["wide"] in (0, -7) and got[0] in (OK, UNSUPPORTED, -1), (c, got)
        if kv8 or c["rope_on_read"]:
            assert got[0] in (UNSUPPORTED, -1) and info["n_launches"] == 0, (c, got)
            assert not (batch and got[15] != 0), (c, got)
        if got[0] == OK and c["q_len"] > 1:
            assert info["qb_rows"] * (c["hq"] // c["h"]) <= 32 and not (info["one_launch"] and info["two_pass"]), (c, got)
        n["ok" if got[0] == OK else "refused"] += 1
        n["one_launch"] += got[0] == OK and info["one_launch"] == 1
        n["batch"] += bool(batch) and got[0] == OK
        n["chunk"] += c["q_len"] > 1 and got[0] == OK
        n["rope"] += bool(c["rope_on_read"])
        n["kv8"] += bool(kv8)
    assert not bad, (len(bad), bad[:3])
    print(f"head_dim-256 planner grid: {len(lines)} calls, {n}")
    assert min(n.values()) > 100, n      # the grid reaches every kind of answer
