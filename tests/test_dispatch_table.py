"""The host dispatch of ekv_step_attend, pinned on a CPU: for a fixed, seeded grid of (bank, step) cases with dummy non-null
pointers (nothing is dereferenced, nothing is launched) the answers of ekv_step_check, ekv_step_plan, ekv_step_info (all 9 fields)
and ekv_workspace_bytes must equal tests/golden/dispatch/dispatch_table.npz exactly.  The A/B switches EKV_NO_WIDE, EKV_NO_RESIDENT,
EKV_FUSED_NW and EKV_NO_WIDE_TAIL are read once per process, so every table is computed in a child process of its own.

The tables were recorded on the dispatch that planned the workspace, the launch sequence and the introspection answers in separate
places, and carried over unchanged to the single planner (ekv_plan_step), with two deliberate exceptions: the EKV_NO_WIDE_TAIL table
(a resident-shaped step is planned as an ordinary one when the wide-kernel scorer tail is off; before, the call failed at launch),
and the ekv_step_plan / ekv_step_info answers for a deferred call whose layer_count differs from defer_layers (13 of the cases),
which now report the tiling the call uses — planned over all deferred layers — instead of that of a stand-alone call.

Regenerate (only when a dispatch decision changes on purpose): python -m tests.test_dispatch_table --record"""
import ctypes
import math
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "dispatch", "dispatch_table.npz")
ENVS = {"default": {}, "EKV_NO_WIDE": {"EKV_NO_WIDE": "1"}, "EKV_NO_RESIDENT": {"EKV_NO_RESIDENT": "1"},
        "EKV_FUSED_NW": {"EKV_FUSED_NW": "4"}, "EKV_NO_WIDE_TAIL": {"EKV_NO_WIDE_TAIL": "1"}}
SWITCHES = ("EKV_NO_WIDE", "EKV_NO_RESIDENT", "EKV_FUSED_NW", "EKV_NO_WIDE_TAIL", "EKV_NO_BIG_TILE", "EKV_RESIDENT_MIN_ROWS",
            "EKV_RESIDENT_LONG_MIN_T")

BANK_KEYS = ("head_dim", "hq", "h", "n_layers", "cap", "arrive", "birth", "score_sum", "score_sq")
STEP_KEYS = ("layer_begin", "layer_count", "q_len", "n_slots", "score_off", "policy", "accumulate", "n_evict", "win_lo", "win_tail",
             "roco_k1", "roco_tail", "range_start", "tova_head_mean", "causal", "rope_on_read", "n_split", "phases", "count_add2",
             "two_pass", "phys_extent", "defer_layers", "defer_index", "q_token_stride", "q_head_stride", "kv_token_stride",
             "kv_head_stride", "out_token_stride", "out_head_stride")
KEYS = BANK_KEYS + STEP_KEYS


def _case(**kw):
    """The north-star decode step (32 heads, roco, one victim) with `kw` changed."""
    c = dict(head_dim=128, hq=32, h=32, n_layers=2, cap=2112, arrive=1, birth=1, score_sum=1, score_sq=1,
             layer_begin=0, layer_count=None, q_len=1, n_slots=2049, score_off=0, policy=2, accumulate=1, n_evict=1, win_lo=0,
             win_tail=0, roco_k1=1434, roco_tail=10, range_start=-1, tova_head_mean=0, causal=1, rope_on_read=0, n_split=0, phases=0,
             count_add2=2, two_pass=0, phys_extent=0, defer_layers=0, defer_index=0, q_token_stride=0, q_head_stride=0,
             kv_token_stride=0, kv_head_stride=0, out_token_stride=0, out_head_stride=0)
    c.update(kw)
    if c["layer_count"] is None:
        c["layer_count"] = c["n_layers"] - c["layer_begin"]
    return c


def _chunk(L, hq, h, n, t_prev, d=128, **kw):
    """A strided chunk step of the encoding / ppl prefill: n new rows onto t_prev cached ones, roco, sink 4, recent 10 %."""
    T = t_prev + n
    c = dict(head_dim=d, hq=hq, h=h, n_layers=L, cap=(T + 64 + 63) // 64 * 64, q_len=n, n_slots=T, n_evict=n if t_prev > n else 0,
             win_lo=4 if t_prev > 100 else 0, win_tail=T // 10, roco_k1=max(T - T // 10 - 4, n), count_add2=2 * n)
    c.update(kw)
    return _case(**c)


def named_cases():
    """One or more cases of every branch of the dispatch (see the comments)."""
    cs = []
    # fused decode: 8-wave (256 heads in the launch), 4-wave (explicit single split, short cache), GQA x3 / x12, head_dim 96
    cs += [_case(n_layers=32), _case(n_layers=4, n_split=1), _case(n_slots=100, cap=192, roco_k1=80), _case(n_layers=32, hq=24, h=8),
           _case(n_layers=4, hq=48, h=4), _case(n_layers=32, head_dim=96), _case(n_layers=32, phys_extent=2112)]
    # slot-indexed rows: accepted, refused (tests/test_host_cpu.py::test_step_check_is_a_dry_run_of_step_attend)
    slot = dict(n_layers=32, phases=16, phys_extent=2112)
    cs += [_case(**slot), _case(**dict(slot, phases=16 | 32)), _case(**dict(slot, score_off=5)), _case(**dict(slot, policy=1, win_lo=4, win_tail=100)),
           _case(**dict(slot, rope_on_read=1)), _case(**dict(slot, count_add2=3)), _case(**dict(slot, layer_count=1)),
           _case(**dict(slot, q_len=8, n_slots=2064, n_evict=8, roco_k1=1847, win_lo=4, win_tail=205)), _case(**dict(slot, birth=0)),
           _case(**dict(slot, score_sq=0)), _case(**dict(slot, n_slots=7000, cap=7040, phys_extent=7040, roco_k1=5000))]
    # split decode: in-kernel fold ('full', attention + fold phases), the fast scorer, the generic scorer with big_rows, no arrive counters
    for extra in ({}, {"arrive": 0}):
        cs += [_case(policy=0, n_evict=0, **extra), _case(phases=1 | 4, **extra), _case(**extra), _case(layer_count=1, **extra),
               _case(policy=1, win_tail=200, **extra), _case(policy=3, **extra), _case(policy=3, tova_head_mean=1, **extra),
               _case(policy=4, range_start=4, **extra), _case(n_slots=12000, cap=12096, roco_k1=9000, **extra),
               _case(n_slots=12000, cap=12096, roco_k1=9000, hq=32, h=8, **extra), _case(phases=2, **extra), _case(phases=8, **extra),
               _case(phases=1, **extra), _case(policy=0, n_evict=0, hq=48, h=4, **extra)]
    # chunk steps: configs[1] (logits in LDS), configs[2] and the LONG shape (resident), configs[3] (wide + tail) and one layer per call
    # (wide two-pass split + scorer), configs[4] (RoPE-on-read on the wide kernel)
    c1 = _chunk(32, 32, 32, 8, 2056)
    cs += [c1, _chunk(32, 32, 8, 16, 1232), _chunk(3, 8, 2, 8, 2056), _chunk(3, 4, 4, 32, 1000), _chunk(3, 8, 2, 4, 700),
           _chunk(32, 32, 32, 96, 5002), _chunk(32, 32, 32, 96, 5002, layer_count=1), _chunk(16, 32, 32, 96, 9898),
           _chunk(40, 40, 40, 96, 4000, rope_on_read=1), _chunk(40, 40, 40, 96, 4000, rope_on_read=1, layer_count=1)]
    # the 16x16 kernel: one pass with the fused scorer, two passes (head_dim 96), RoPE-on-read (head_dim 32), exported logits
    cs += [_chunk(32, 32, 32, 16, 4096), _chunk(32, 32, 32, 48, 4000, d=96), _chunk(4, 32, 32, 96, 2000, d=32, rope_on_read=1),
           _chunk(4, 32, 32, 96, 2000, d=32), _chunk(32, 32, 32, 16, 4096, two_pass=-1), _chunk(32, 32, 32, 96, 5002, two_pass=-1),
           _chunk(32, 32, 8, 16, 1232, two_pass=1), _chunk(32, 32, 32, 16, 4096, n_split=-1), _chunk(32, 32, 32, 16, 4096, d=64)]
    # the dense prefix: unscored ('full') and scored
    cs += [_chunk(32, 32, 32, 4906, 0, policy=0, accumulate=0, n_evict=0), _chunk(32, 32, 32, 4906, 0),
           _chunk(32, 32, 8, 2048, 0, policy=0, accumulate=0, n_evict=0), _chunk(2, 32, 32, 4906, 0, d=64, policy=0, accumulate=0)]
    # policies of chunk steps: h2o_head, tova (+ head mean), recency / random, full
    cs += [_chunk(32, 32, 32, 96, 5002, policy=1), _chunk(32, 32, 32, 96, 5002, policy=3), _chunk(32, 32, 32, 96, 5002, policy=3, tova_head_mean=1),
           _chunk(32, 32, 32, 8, 2056, policy=3, tova_head_mean=1), _chunk(32, 32, 32, 96, 5002, policy=4, range_start=4),
           _chunk(32, 32, 32, 96, 5002, policy=0, n_evict=0), _chunk(32, 32, 32, 96, 5002, accumulate=0)]
    # phases (one layer per call, split heads) and the deferred scorer: per-layer calls and the flush, unsplit and split
    fl = dict(layer_count=1, n_split=4)
    for ph in (1, 2, 1 | 4, 8, 3, 5, 9, 12, 16, 64):
        cs += [_chunk(32, 32, 32, 96, 5002, phases=ph, **fl), _chunk(32, 32, 32, 16, 4096, phases=ph, **fl), _case(phases=ph)]
    for L, h in ((32, 32), (4, 8), (40, 40)):
        for rope in (0, 1):
            d = dict(defer_layers=L, n_split=4, rope_on_read=rope)
            cs += [_chunk(L, h, h, 96, 5002, phases=8, **d), _chunk(L, h, h, 96, 5002, phases=1 | 4, layer_count=1, layer_begin=3, defer_index=3, **d),
                   _chunk(L, h, h, 16, 4096, phases=8, **d), _chunk(L, h, h, 16, 4096, phases=1 | 4, layer_count=1, defer_index=L - 1, layer_begin=L - 1, **d),
                   _case(n_layers=L, hq=h, h=h, phases=1 | 4, layer_count=1, defer_index=1, layer_begin=1, **d), _case(n_layers=L, hq=h, h=h, phases=8, **d)]
    cs += [_chunk(32, 32, 32, 96, 5002, defer_layers=32, n_split=4, phases=8, n_slots=20000, cap=20032)]
    # refusals: W > 39 000, a head_dim that is not built, the EKV_E_ARG cases of test_step_check_is_a_dry_run_of_step_attend
    cs += [_case(cap=60032, n_slots=60000, roco_k1=30000, n_split=-1), _case(head_dim=48), _case(roco_k1=4000), _case(n_slots=4000),
           _case(policy=4, range_start=-1), _case(layer_count=3), _case(defer_layers=2, n_split=8, phases=8), _case(defer_layers=2, n_split=0, phases=8),
           _case(score_sum=0), _case(score_sq=0), _case(q_token_stride=7), _case(q_head_stride=64), _case(q_head_stride=128),
           _chunk(32, 32, 32, 96, 5002, q_token_stride=4096, q_head_stride=128), _chunk(32, 32, 32, 96, 5002, out_token_stride=-8),
           _chunk(32, 32, 32, 96, 5002, kv_token_stride=1024, kv_head_stride=128), _case(n_evict=2049), _case(policy=5), _case(policy=0)]
    return cs


def random_cases(n=2400, seed=20261016):
    rs = np.random.RandomState(seed)
    pick = lambda xs: xs[rs.randint(len(xs))]
    out = []
    for _ in range(n):
        d = pick([32, 64, 96, 128, 128, 128, 64, 48])
        hq, h = pick([(32, 32), (32, 8), (8, 2), (4, 4), (40, 40), (16, 2), (24, 8), (48, 4), (8, 8), (64, 8), (4, 2)])
        L = pick([1, 2, 3, 4, 16, 32, 40])
        lc = pick([L, L, 1, max(1, L // 2)])
        lb = rs.randint(0, L - lc + 1)
        n = pick([1, 1, 1, 1, 2, 4, 8, 9, 12, 16, 20, 24, 32, 33, 40, 48, 64, 96, 128, 200, 512])
        t_prev = pick([0, 5, 100, 300, 700, 1000, 1232, 1500, 2048, 2056, 3000, 4096, 5002, 9994, 12000, 20000, 45000])
        T = t_prev + n
        cap = pick([(T + 64 + 63) // 64 * 64, (T + 63) // 64 * 64, T + 1, T])
        policy = pick([0, 1, 2, 2, 2, 3, 4])
        W_off = pick([0, 0, 0, min(4, T - 1), max(0, T - n - 1)])
        W = T - W_off
        n_evict = pick([0, 1 if n == 1 else n, 1 if n == 1 else n])
        win_lo = pick([0, 4]) if W > 100 else 0
        win_tail = pick([0, W // 10, W // 20])
        c = dict(head_dim=d, hq=hq, h=h, n_layers=L, cap=cap, arrive=int(rs.rand() < 0.8), birth=int(rs.rand() < 0.7),
                 score_sum=int(rs.rand() < 0.97), score_sq=int(rs.rand() < 0.9), layer_begin=lb, layer_count=lc, q_len=n, n_slots=T,
                 score_off=W_off, policy=policy, accumulate=int(rs.rand() < 0.85), n_evict=n_evict, win_lo=win_lo, win_tail=win_tail,
                 roco_k1=pick([max(n_evict, W - W // 10 - win_lo), n_evict, W, W + 1]), roco_tail=10, range_start=pick([-1, 0, 4, max(0, T - n_evict - 3)]),
                 tova_head_mean=int(rs.rand() < 0.3), causal=int(rs.rand() < 0.95), rope_on_read=int(rs.rand() < 0.2),
                 n_split=pick([0, 0, 0, 0, -1, 1, 2, 4, 8]), phases=pick([0] * 12 + [1, 2, 1 | 4, 8, 3, 16, 16 | 32, 5, 12]),
                 count_add2=pick([2, 2 * n, 3]), two_pass=pick([0, 0, 0, 1, -1]), phys_extent=pick([0, 0, T, cap, cap + 64]))
        if rs.rand() < 0.12:      # deferred scorer
            c.update(defer_layers=L + pick([0, 0, 0, 1]), defer_index=lb, n_split=pick([1, 2, 4, 8, 0]), phases=pick([1 | 4, 8, 8, 0]))
        r = rs.rand()
        if r < 0.1:               # explicit dense strides
            c.update(q_token_stride=d, q_head_stride=n * d, kv_token_stride=d, kv_head_stride=n * d, out_token_stride=d, out_head_stride=n * d)
        elif r < 0.2:             # padded rows (token-major packing of a projection)
            c.update(q_token_stride=hq * d, q_head_stride=d, kv_token_stride=h * d + pick([0, 8, 3]), kv_head_stride=d,
                     out_token_stride=hq * d, out_head_stride=pick([d, 0]))
        out.append(_case(**c))
    return out


def cases():
    return named_cases() + random_cases()


def _structs(c):
    from easykv_amd._lib import Bank, Step
    p = lambda on: 256 if on else None
    bank = Bank(256, 256, 256, p(c["score_sum"]), p(c["score_sq"]), p(c["score_sq"]), c["n_layers"], c["hq"], c["h"], c["head_dim"],
                c["cap"], p(c["arrive"]), p(c["birth"]), p(c["birth"]))       # (dummy non-null pointers: nothing is dereferenced)
    st = Step()
    for k in STEP_KEYS:
        if k != "count_add2":
            setattr(st, k, c[k])
    st.count_add, st.count_tail_step, st.sm_div = c["count_add2"] / 2, -1.0 if c["q_len"] > 1 else 0.0, math.sqrt(c["head_dim"])
    return bank, st


def table(cs):
    """One row per case: check rc, plan rc, n_split, fused, info rc, the 9 info fields, workspace bytes."""
    from easykv_amd import _lib
    lib = _lib.load()
    rows = []
    for c in cs:
        bank, st = _structs(c)
        b, s = ctypes.byref(bank), ctypes.byref(st)
        ns, fu = ctypes.c_int32(-7), ctypes.c_int32(-7)
        info = (ctypes.c_int32 * 9)(*([-7] * 9))
        check = lib.ekv_step_check(b, s)
        prc = lib.ekv_step_plan(b, s, ctypes.byref(ns), ctypes.byref(fu))
        irc = lib.ekv_step_info(b, s, info, 9)
        rows.append([check, prc, ns.value, fu.value, irc] + list(info) + [lib.ekv_workspace_bytes(b, s)])
    return np.array(rows, dtype=np.int64)


def params(cs):
    return np.array([[c[k] for k in KEYS] for c in cs], dtype=np.int32)


def _child_table(name, path):
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env.update(ENVS[name])
    r = subprocess.run([sys.executable, "-m", "tests.test_dispatch_table", "--emit", path], cwd=ROOT, env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return np.load(path)


@pytest.fixture(scope="module")
def golden():
    from easykv_amd import _build
    if not os.path.exists(_build.LIB):
        _build.build_lib()
    return np.load(GOLDEN)


def test_grid_is_the_recorded_one(golden):
    assert np.array_equal(golden["params"], params(cases()))


@pytest.mark.parametrize("name", list(ENVS))
def test_dispatch_table_is_unchanged(golden, name, tmp_path):
    got = _child_table(name, str(tmp_path / f"{name}.npy"))
    want = golden[name]
    assert got.shape == want.shape
    bad = np.nonzero((got != want).any(axis=1))[0]
    cs = cases()
    assert len(bad) == 0, [(int(i), {k: v for k, v in cs[i].items()}, want[i].tolist(), got[i].tolist()) for i in bad[:5]]


def test_resident_shapes_without_the_wide_tail_plan_as_ordinary_steps(tmp_path):
    """The logits-resident kernel's scorer is the wide column-sum pass's tail: with EKV_NO_WIDE_TAIL=1 a resident-shaped step (configs[2]:
    64 rows x 1248 keys; 32 rows x 2064 keys) is planned from scratch as an ordinary step — the launches it would have without the
    resident kernel (EKV_NO_RESIDENT=1) — and not as the one launch it cannot make."""
    cs = [_chunk(32, 32, 8, 16, 1232), _chunk(3, 8, 2, 8, 2056), _chunk(3, 4, 4, 32, 1000), _chunk(3, 8, 2, 4, 700)]
    idx = [named_cases().index(c) for c in cs]
    no_tail = _child_table("EKV_NO_WIDE_TAIL", str(tmp_path / "a.npy"))[idx]
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env.update(EKV_NO_WIDE_TAIL="1", EKV_NO_RESIDENT="1")
    r = subprocess.run([sys.executable, "-m", "tests.test_dispatch_table", "--emit", str(tmp_path / "b.npy")], cwd=ROOT, env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    ordinary = np.load(str(tmp_path / "b.npy"))[idx]
    default = _child_table("default", str(tmp_path / "c.npy"))[idx]
    assert (default[:, 0] == 0).all() and (default[:, 3] == 1).all() and (default[:, 13] == 1).all()      # resident: one launch
    assert (no_tail[:, 0] == 0).all() and (no_tail[:, 3] == 0).all() and (no_tail[:, 13] >= 2).all(), no_tail
    assert np.array_equal(no_tail, ordinary)
    assert no_tail[0, 13] == 3 and no_tail[0, 7] == 1      # configs[2]: wide two-pass, one pass + column-sum pass + scorer


if __name__ == "__main__":
    if sys.argv[1] == "--emit":
        np.save(sys.argv[2], table(cases()))
    elif sys.argv[1] == "--record":
        import tempfile
        with tempfile.TemporaryDirectory() as d:
            tabs = {name: _child_table(name, os.path.join(d, f"{name}.npy")) for name in ENVS}
        np.savez_compressed(GOLDEN, params=params(cases()), **tabs)
        print({k: v.shape for k, v in tabs.items()}, os.path.getsize(GOLDEN))
