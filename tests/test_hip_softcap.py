"""Soft-capped attention logits (Gemma 2: attn_logit_softcapping) on the GPU: the cap function, decode steps, chunk steps and the dense
prefix of a KVBank(logit_cap=...) against the oracle with HF's eager Gemma 2 attention as its `attention_core` (tests/softcap_ref.py).

(a) The function.  ekv_softcap_eval runs the one inline every capped kernel calls.  Truth: float64 cap * tanh(x / cap).  Yardstick:
torch's fp32 evaluation of HF's three ops (w / cap, tanh, * cap) at the same points, on the CPU (the stricter of the two torch
backends: correctly scaled, <= 1 ulp tanh).  Per decade of |x| / cap the kernel's largest absolute error must not exceed twice the
yardstick's largest error in that decade, with a floor of one fp32 ulp of the largest result in the decade.

(b) / (c) follow the protocol of tests/test_hip_d256.py (run_decode_case / run_chunk_case): seeded randn(...).half() streams, outputs
held to out_close, victims compared exactly wherever the Probe of tests/test_hip_fullsize.py calls the decision stable, the slot map a
permutation at the end; a case compares at least 10 decisions and at least half of its evicting (step, layer, head) triples (the seeds
were chosen by running each case with oracle_only=True on a CPU).  Two regimes: cap 2.0 on randn rows (logit std 1: the cap reshapes
most of the row) and cap 50.0 with the queries scaled by 6 (the magnitude regime of a real Gemma 2).  Every decode case prints its
distance to the uncapped oracle — max |o_capped - o_uncapped| over the run, on the CPU oracle alone — and asserts it is at least ten
times the out_close bound: without the feature the case cannot pass."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest
import torch

from tests.golden_util import out_close
from tests.softcap_ref import patched
from tests.test_hip_d256 import _enough, _permutation, _ProbeAndCapture
from tests.test_hip_fullsize import Probe

pytestmark = pytest.mark.gpu
OUT_BOUND = 1e-3      # out_close's flat bound
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _mk(L, H, n, g, d, gain=1.0):
    x = torch.randn(L, H, n, d, generator=g)
    return (x * gain if gain != 1.0 else x).half()


# ---- (a) the function -------------------------------------------------------------------------------------------------------------------
CAPS = (2.0, 30.0, 50.0)
DECADES = (1e-4, 1e-3, 1e-2, 1e-1, 1.0)


def _eval(x, cap, sm_div=1.0):
    from easykv_amd import _lib
    lib = _lib.load()
    xd = torch.as_tensor(x, dtype=torch.float32).cuda().contiguous()
    out = torch.empty_like(xd)
    _lib.check(lib.ekv_softcap_eval(C.c_void_p(xd.data_ptr()), xd.numel(), sm_div, cap, C.c_void_p(out.data_ptr()),
                                    C.c_void_p(torch.cuda.current_stream().cuda_stream)), "ekv_softcap_eval")
    return out.cpu().numpy()


def _grid(cap):
    ax = np.logspace(math.log10(1e-4 * cap), math.log10(8 * cap), 4096)
    return np.concatenate([-ax[::-1], ax]).astype(np.float32)


def _tables(cap):
    x = _grid(cap)
    truth = cap * np.tanh(x.astype(np.float64) / cap)
    got = _eval(x, cap)
    tx = torch.from_numpy(x)
    yard = (torch.tanh(tx / cap) * cap).numpy()
    yard_gpu = (torch.tanh(tx.cuda() / cap) * cap).cpu().numpy()
    r = np.abs(x.astype(np.float64)) / cap
    rows = []
    for lo in DECADES:
        m = (r >= lo) & (r < 10 * lo)
        rows.append(dict(decade=[lo, 10 * lo], points=int(m.sum()), kernel=float(np.abs(got[m] - truth[m]).max()),
                         torch_cpu=float(np.abs(yard[m] - truth[m]).max()), torch_gpu=float(np.abs(yard_gpu[m] - truth[m]).max()),
                         ulp_of_largest=float(np.spacing(np.float32(np.abs(truth[m]).max())))))
    return x, got, rows


def test_cap_function_is_as_close_to_the_truth_as_torchs_three_ops():
    report = {}
    failures = []
    for cap in CAPS:
        x, got, rows = _tables(cap)
        report[str(cap)] = rows
        for row in rows:
            bound = max(2.0 * row["torch_cpu"], row["ulp_of_largest"])
            print(f"[softcap] cap {cap:g} |x|/cap in [{row['decade'][0]:g}, {row['decade'][1]:g}): kernel {row['kernel']:.3e} torch(cpu) {row['torch_cpu']:.3e} "
                  f"torch(gpu) {row['torch_gpu']:.3e} ulp {row['ulp_of_largest']:.3e} bound {bound:.3e}")
            if not row["kernel"] <= bound:
                failures.append((cap, row))
        # odd in x, monotone over the sorted grid
        assert np.array_equal(got, -got[::-1]), cap
        assert bool(np.all(np.diff(got.astype(np.float64)) >= 0)), cap
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)      # (the recorded tables: profiles/softcap_accuracy.json, as the fidelity files)
    with open(os.path.join(ROOT, "profiles", "softcap_accuracy.json"), "w") as f:
        json.dump(dict(truth="float64 cap * tanh(x / cap)", grid="4096 log-spaced |x| in [1e-4 cap, 8 cap], both signs; largest |error| per decade of |x| / cap",
                       caps=report), f, indent=1)
    assert not failures, failures


def test_cap_function_special_values_and_scale():
    for cap in CAPS:
        got = _eval(np.array([0.0, -0.0, np.inf, -np.inf, np.nan], np.float32), cap)
        assert got[0] == 0.0 and got[1] == 0.0 and got[2] == np.float32(cap) and got[3] == -np.float32(cap) and np.isnan(got[4]), (cap, got)
    # x / sm_div is the quotient the kernels form: a power-of-two divisor changes nothing but the argument
    x = _grid(30.0)
    assert np.array_equal(_eval(x, 30.0, sm_div=4.0), _eval(x / np.float32(4.0), 30.0))
    from easykv_amd import _lib
    lib = _lib.load()
    t = torch.zeros(4, device="cuda")
    for cap in (0.0, -1.0, float("inf"), float("nan")):
        assert lib.ekv_softcap_eval(C.c_void_p(t.data_ptr()), 4, 1.0, cap, C.c_void_p(t.data_ptr()), None) == -1, cap


# ---- (b) decode steps -------------------------------------------------------------------------------------------------------------------
REGIMES = {"cap2": (2.0, 1.0), "cap50x6": (50.0, 6.0),      # name -> (cap, gain on the queries)
           "scale_only": (None, 1.0)}      # (no cap: the free softmax scale alone, tests/test_hip_sm_scale.py)
DECODE_SHAPES = {
    # id: rep, H, L, budget, n_split, policy, one_launch
    "mha_roco_fused4": (1, 4, 2, 140, 1, "roco", True),                 # one launch, 4 waves
    "gqa2_h2o_split2": (2, 2, 2, 160, 2, "h2o_head", None),            # moves from one launch to the split path
    "gqa4_tova_split3": (4, 2, 2, 200, 3, "tova", None),               # split + in-kernel fold
    "gqa8_h2o_fused4": (8, 1, 3, 60, 1, "h2o_head", True),             # one launch
    "mha_tova_fused8_256_heads": (1, 16, 16, 60, 0, "tova", True),     # 256 heads, the 8-wave build
}
DECODE_CASES = [
    # shape, head_dim, regime, sm_scale, seed
    ("mha_roco_fused4", 256, "cap2", None, 1), ("mha_roco_fused4", 128, "cap2", None, 1),
    ("gqa2_h2o_split2", 256, "cap2", 224 ** -0.5, 2), ("gqa2_h2o_split2", 128, "cap2", 144 ** -0.5, 2),
    ("gqa4_tova_split3", 256, "cap2", None, 3), ("gqa4_tova_split3", 128, "cap2", None, 3),
    ("gqa8_h2o_fused4", 256, "cap2", None, 4), ("gqa8_h2o_fused4", 128, "cap2", None, 4),
    ("mha_tova_fused8_256_heads", 256, "cap2", None, 5), ("mha_tova_fused8_256_heads", 128, "cap2", None, 5),
    ("mha_roco_fused4", 256, "cap50x6", None, 6), ("mha_roco_fused4", 128, "cap50x6", None, 6),
    ("gqa4_tova_split3", 256, "cap50x6", None, 7), ("gqa4_tova_split3", 128, "cap50x6", None, 7),
]


def run_decode_case(shape, D, regime, sm_scale, seed, oracle_only=False, stream=False):
    """shape: a key of DECODE_SHAPES or its tuple; stream: RoPE-on-read (uncapped banks only)."""
    from oracle import easykv_oracle as O
    rep, H, L, budget, n_split, policy, one_launch = DECODE_SHAPES[shape] if isinstance(shape, str) else shape
    cap, gain = REGIMES[regime]
    name = f"{shape if isinstance(shape, str) else 'x'.join(map(str, shape[:5]))}_d{D}_{regime}" + ("_scaled" if sm_scale is not None else "") + ("_rope" if stream else "")
    Hq, P = H * rep, 5
    steps = budget + 25
    g = torch.Generator().manual_seed(31000 + 100 * seed + D)
    qs, ks, vs = _mk(L, Hq, P + steps, g, D, gain), _mk(L, H, P + steps, g, D), _mk(L, H, P + steps, g, D)
    bank = None
    if not oracle_only:
        from easykv_amd import KVBank, StepPlan
        bank = KVBank(L, Hq, H, D, cap=P + budget + 1, logit_cap=cap, sm_scale=sm_scale)
        if stream:
            bank.set_rope(*O.rope_tables(P + budget + 72, D))
        bank.load_rows(ks[:, :, :P].cuda(), vs[:, :, :P].cuda())
        bank.state_init(budget + 1, 0)
    cos, sin = O.rope_tables(P + budget + 72, D) if stream else (None, None)
    sts = []
    for l in range(L):
        st = O.LayerState(k=ks[l:l + 1, :, :P].float(), v=vs[l:l + 1, :, :P].float())
        st.s, st.q, st.c = O.init_state_decoding((H,), budget)
        sts.append(st)
    alive = torch.ones(L, H, dtype=torch.bool)
    probe = Probe()
    O.SELECT_HOOK = probe
    n_checked = n_total = n_fused = 0
    dist = [0.0]
    try:
        with patched(cap, sm_scale, dist):
            for i in range(steps):
                t = P + i
                T_prev = P + i if i <= budget else P + budget
                evict = (T_prev + 1 - P) > budget
                kw = dict(policy=policy, phase="decode", evict=evict, score_off=P, budget=budget, range_start=-1, streaming=stream)
                if bank is not None:
                    assert bank.n_slots[0] == T_prev
                    plan = StepPlan(n_split=n_split, **kw)
                    info = bank.step_info(plan, 1)
                    fused = bool(info["fused"])
                    if one_launch is not None:
                        assert fused == one_launch, (name, i, info)
                    n_fused += fused
                    out, ids = bank.attend(plan, qs[:, :, t:t + 1].cuda().contiguous(), ks[:, :, t:t + 1].cuda().contiguous(),
                                           vs[:, :, t:t + 1].cuda().contiguous())
                for l in range(L):
                    if not bool(alive[l].any()):
                        continue
                    o_ref, ids_ref = O.layer_step(sts[l], qs[l:l + 1, :, t:t + 1].float(), ks[l:l + 1, :, t:t + 1].float(),
                                                  vs[l:l + 1, :, t:t + 1].float(), O.StepPlan(**kw), cos, sin)
                    if bank is not None:
                        rows = alive[l].repeat_interleave(rep)
                        got_o, ref_o = out[l].float().cpu(), o_ref[0]
                        assert out_close(got_o[rows], ref_o[rows]), (name, i, l, float((got_o[rows] - ref_o[rows]).abs().max()))
                    if evict:
                        ok = ~probe.last_unstable
                        same = torch.ones(H, dtype=torch.bool)
                        if bank is not None:
                            same = ids[l, :, 0].cpu().long() == ids_ref[:, 0] + P
                            assert bool(same[ok & alive[l]].all()), (name, i, l, ids[l, :, 0].tolist(), (ids_ref[:, 0] + P).tolist())
                        n_total += H
                        n_checked += int((ok & alive[l]).sum())
                        alive[l] &= ok & same
    finally:
        O.SELECT_HOOK = None
    if bank is not None:
        if one_launch is None:
            assert 0 < n_fused < steps, (name, n_fused)      # both paths were visited
        assert bank.n_slots == [P + budget] * L
        _permutation(bank)
    print(f"[softcap] {name}: max |o - o of the uncapped, standard-scale oracle| over the run = {dist[0]:.3e} (out_close bound {OUT_BOUND:g})")
    assert dist[0] >= 10 * OUT_BOUND, (name, dist[0])
    _enough(name, n_checked, n_total)
    return n_checked, n_total, dist[0]


@pytest.mark.parametrize("shape,D,regime,sm_scale,seed", DECODE_CASES,
                         ids=[f"{c[0]}-d{c[1]}-{c[2]}" + ("-scaled" if c[3] is not None else "") for c in DECODE_CASES])
def test_capped_decode_steps(shape, D, regime, sm_scale, seed):
    run_decode_case(shape, D, regime, sm_scale, seed)


SLOT_SEED = 1


def run_slot_case(oracle_only=False, seed=SLOT_SEED):
    """Whole-cache decode steps (score_off = 0) of 528 heads at head_dim 128: the 4-wave one-launch build on the slot-indexed score rows,
    with mixed phase orders (the K phase forms its own logits) and resident rows — the flagship instance's capped twin."""
    from oracle import easykv_oracle as O
    D, L, H, budget, steps, cap = 128, 33, 16, 70, 12, 2.0
    T = budget + 1
    g = torch.Generator().manual_seed(31900 + seed)
    k0, v0 = _mk(L, H, budget, g, D), _mk(L, H, budget, g, D)
    warm = torch.rand(L, H, T, generator=g) * 1e-3
    bank = None
    if not oracle_only:
        from easykv_amd import KVBank, StepPlan
        bank = KVBank(L, H, H, D, cap=T + 63, logit_cap=cap)
        bank.load_rows(k0.cuda(), v0.cuda())
        bank.state_init(T, 0)
        bank.score_sum[:, :, :T] += warm.cuda()
        bank.score_sq[:, :, :T] += (warm ** 2).cuda()
        plan = StepPlan(policy="roco", phase="decode", evict=True, budget=budget)
        info = bank.step_info(plan, 1)
        assert info["fused"] == 1 and info["n_launches"] == 1, info
    sts = []
    for l in range(L):
        st = O.LayerState(k=k0[l:l + 1].float(), v=v0[l:l + 1].float())
        st.s, st.q, st.c = O.init_state_decoding((H,), budget)
        st.s += warm[l]
        st.q += warm[l] ** 2
        sts.append(st)
    alive = torch.ones(L, H, dtype=torch.bool)
    probe = Probe()
    O.SELECT_HOOK = probe
    n_checked = n_total = n_slot = 0
    orders = set()
    try:
        with patched(cap):
            for i in range(steps):
                q, k, v = _mk(L, H, 1, g, D), _mk(L, H, 1, g, D), _mk(L, H, 1, g, D)
                if bank is not None:
                    out, ids = bank.attend(plan, q.cuda(), k.cuda(), v.cuda())
                    n_slot += int(all(bank._slot_rows))
                    orders.add(bank.step_info(plan, 1, phases=16)["fused_order"])
                for l in range(L):
                    o_ref, ids_ref = O.layer_step(sts[l], q[l:l + 1].float(), k[l:l + 1].float(), v[l:l + 1].float(),
                                                  O.StepPlan(policy="roco", phase="decode", evict=True, budget=budget))
                    ok = ~probe.last_unstable
                    same = torch.ones(H, dtype=torch.bool)
                    if bank is not None:
                        got_o = out[l].float().cpu()
                        assert out_close(got_o[alive[l]], o_ref[0][alive[l]]), (i, l)
                        same = ids[l, :, 0].cpu().long() == ids_ref[:, 0]
                        assert bool(same[ok & alive[l]].all()), (i, l)
                    n_total += H
                    n_checked += int((ok & alive[l]).sum())
                    alive[l] &= ok & same
    finally:
        O.SELECT_HOOK = None
    if bank is not None:
        assert n_slot == steps, n_slot      # every step ran on the slot-indexed layout
        if "EKV_FUSED_ORDER" not in os.environ:
            assert orders == {1}, orders      # mixed phase orders: some workgroups form their logits in the K phase
        _permutation(bank)
    _enough("slot_rows_capped_d128", n_checked, n_total)
    return n_checked, n_total


def test_capped_decode_steps_on_the_slot_indexed_layout():
    run_slot_case()


def test_capped_decode_steps_deferred():
    """One layer per call with the scorer deferred: attend(defer=True) per layer + one flush per token, on a capped bank."""
    from easykv_amd import KVBank, StepPlan
    from oracle import easykv_oracle as O
    D, L, H, rep, budget, steps, cap = 256, 4, 2, 2, 48, 30, 2.0
    Hq, T = H * rep, budget + 1
    g = torch.Generator().manual_seed(31950)
    k0, v0 = _mk(L, H, budget, g, D), _mk(L, H, budget, g, D)
    bank = KVBank(L, Hq, H, D, cap=T + 8, logit_cap=cap)
    bank.load_rows(k0.cuda(), v0.cuda())
    bank.state_init(T, 0)
    sts = []
    for l in range(L):
        st = O.LayerState(k=k0[l:l + 1].float(), v=v0[l:l + 1].float())
        st.s, st.q, st.c = O.init_state_decoding((H,), budget)
        sts.append(st)
    plan = StepPlan(policy="h2o_head", phase="decode", evict=True, budget=budget)
    kw = dict(policy="h2o_head", phase="decode", evict=True, budget=budget)
    alive = torch.ones(L, H, dtype=torch.bool)
    probe = Probe()
    O.SELECT_HOOK = probe
    n_checked = n_total = 0
    try:
        with patched(cap):
            for i in range(steps):
                q, k, v = _mk(L, Hq, 1, g, D), _mk(L, H, 1, g, D), _mk(L, H, 1, g, D)
                outs = [bank.attend(plan, q[l:l + 1].cuda(), k[l:l + 1].cuda(), v[l:l + 1].cuda(), layer_begin=l, defer=True)[0] for l in range(L)]
                ids = bank.flush()
                out = torch.cat(outs)
                for l in range(L):
                    o_ref, ids_ref = O.layer_step(sts[l], q[l:l + 1].float(), k[l:l + 1].float(), v[l:l + 1].float(), O.StepPlan(**kw))
                    rows = alive[l].repeat_interleave(rep)
                    got_o = out[l].float().cpu()
                    assert out_close(got_o[rows], o_ref[0][rows]), (i, l)
                    ok = ~probe.last_unstable
                    same = ids[l, :, 0].cpu().long() == ids_ref[:, 0]
                    assert bool(same[ok & alive[l]].all()), (i, l)
                    n_total += H
                    n_checked += int((ok & alive[l]).sum())
                    alive[l] &= ok & same
    finally:
        O.SELECT_HOOK = None
    assert bank.n_slots == [budget] * L
    _permutation(bank)
    _enough("deferred_capped_d256", n_checked, n_total)


def _pv_capped(q, k_all, v_all, t_prev, cap, gain_scale=None):
    """p.|V| of the capped oracle's fp32 probabilities (the term of the bf16 bar of tests/test_hip_bf16.py)."""
    hq, n, d = q.shape
    rep = hq // k_all.shape[0]
    k, v = k_all.repeat_interleave(rep, 0), v_all.repeat_interleave(rep, 0)
    s = q @ k.transpose(1, 2) / math.sqrt(d)
    s = torch.tanh(s / cap) * cap
    T = k.shape[1]
    mask = torch.arange(T)[None, :] > (t_prev + torch.arange(n))[:, None]
    s = s.masked_fill(mask, float("-inf"))
    return torch.softmax(s, dim=-1) @ v.abs()


@pytest.mark.parametrize("D", [256, 128])
def test_capped_decode_steps_bf16(D):
    """bf16 rows on a capped bank, the split path with the fold, under the bf16 bar and the tolerance classes of tests/test_hip_bf16.py."""
    import tests.test_hip_bf16 as TBF
    from easykv_amd import KVBank, StepPlan
    from oracle import easykv_oracle as O
    from tests.test_hip_lockstep import Hook
    BF = torch.bfloat16
    L, hq, h, budget, policy, n_split, steps, cap = 2, 6, 2, 300, "roco", 2, 24, 2.0
    T = budget + 1
    g = torch.Generator().manual_seed(31960 + D)
    bank = KVBank(L, hq, h, D, cap=T + 8, dtype=BF, logit_cap=cap)
    bank.load_rows(torch.randn(L, h, budget, D, generator=g).to(BF).cuda(), torch.randn(L, h, budget, D, generator=g).to(BF).cuda())
    bank.state_init(T, 0)
    warm = torch.rand(L, h, budget, generator=g) * 1e-3
    bank.score_sum[:, :, :budget] += warm.cuda()
    bank.score_sq[:, :, :budget] += (warm ** 2).cuda()
    states = TBF._seed(bank, T)
    plan = StepPlan(policy=policy, phase="decode", evict=True, score_off=0, budget=budget, n_split=n_split)
    oplan = O.StepPlan(policy=policy, phase="decode", evict=True, score_off=0, budget=budget)
    info = bank.step_info(plan, 1)
    assert info["fused"] == 0 and info["n_split"] == 2, info
    hook = Hook()
    O.SELECT_HOOK = hook
    try:
        with patched(cap):
            for i in range(steps):
                q, k, v = (torch.randn(L, hh, 1, D, generator=g).to(BF) for hh in (hq, h, h))
                out, ids = bank.attend(plan, q.cuda(), k.cuda(), v.cuda())
                assert out.dtype == BF
                reseed = []
                for l in range(L):
                    st = states[l]
                    k_all, v_all = torch.cat([st.k[0], k[l].float()], 1), torch.cat([st.v[0], v[l].float()], 1)
                    pv = _pv_capped(q[l].float(), k_all, v_all, k_all.shape[1] - 1, cap)
                    o_ref, ids_ref = O.layer_step(st, q[l:l + 1].float(), k[l:l + 1].float(), v[l:l + 1].float(), oplan)
                    TBF._check_out(out[l], o_ref[0], pv, ("capped bf16", D, i, l))
                    if TBF._check_ids(hook, ids[l].cpu(), ids_ref.view(h, -1), ("capped bf16", D, i, l)):
                        reseed.append(l)
                if reseed:
                    fresh = TBF._seed(bank, T)
                    for l in set(reseed):
                        states[l] = fresh[l]
                        states[l].s, states[l].q, states[l].c = states[l].s[:, :T], states[l].q[:, :T], states[l].c[:, :T]
    finally:
        O.SELECT_HOOK = None


# ---- (c) chunk steps and the dense prefix -----------------------------------------------------------------------------------------------
CHUNK_SHAPES = {
    # id: rep, H, stride, idx, policy, two_pass, n_split
    "mha_s8_one_pass_tail": (1, 3, 8, 210, "roco", 0, 0),             # mode 0 + the scorer as the kernel's tail
    "gqa2_s16_two_pass": (2, 2, 16, 300, "h2o_head", 1, 0),           # modes 1 + 2
    "gqa4_s8_full_block": (4, 2, 8, 230, "roco", 0, 0),               # 32 folded rows: a full block
    "mha_s40_two_blocks": (1, 2, 40, 330, "roco", 0, 0),              # two blocks (32 + 8 rows), two passes by the planner's rule
    "mha_s16_split2": (1, 3, 16, 400, "h2o_head", 0, 2),              # a key range split in two
    "mha_s16_split2_two_pass": (1, 3, 16, 400, "roco", 1, 2),
}
CHUNK_CASES = [(shape, D, "cap2", 1 + i) for D in (256, 128) for i, shape in enumerate(CHUNK_SHAPES)] + \
              [("gqa2_s16_two_pass", 256, "cap50x6", 11), ("mha_s8_one_pass_tail", 128, "cap50x6", 12)]


def run_chunk_case(shape, D, regime, seed, oracle_only=False, sm_scale=None, expect=None):
    """shape: a key of CHUNK_SHAPES or its tuple; expect: step_info fields every step must report (which kernel served it)."""
    from oracle import easykv_oracle as O
    from tests.select_rule import feasible_classes, valid_victims
    rep, H, s, idx, policy, two_pass, n_split = CHUNK_SHAPES[shape] if isinstance(shape, str) else shape
    cap, gain = REGIMES[regime]
    name = f"{shape if isinstance(shape, str) else 'x'.join(map(str, shape[:5]))}_d{D}_{regime}" + ("_scaled" if sm_scale is not None else "")
    Hq, L, n_steps = H * rep, 2, 4
    budget_p, recent, sink = idx + s // 2, int(idx * 0.2), 4
    g = torch.Generator().manual_seed(32000 + 100 * seed + D)
    k0, v0 = _mk(L, H, idx, g, D), _mk(L, H, idx, g, D)
    bank = None
    if not oracle_only:
        from easykv_amd import KVBank, StepPlan
        bank = KVBank(L, Hq, H, D, cap=idx + s, logit_cap=cap, sm_scale=sm_scale)
        bank.load_rows(k0.cuda(), v0.cuda())
        bank.state_init(idx + s, 2, s)
    sts = []
    for l in range(L):
        st = O.LayerState(k=k0[l:l + 1].float(), v=v0[l:l + 1].float())
        st.s, st.q, st.c = O.init_state_prefill((H,), idx, s, False)
        sts.append(st)
    hook = _ProbeAndCapture()
    O.SELECT_HOOK = hook
    alive = torch.ones(L, H, dtype=torch.bool)
    n_checked = 0
    k1 = max(budget_p - recent - sink, s)
    dist = [0.0]
    try:
        with patched(cap, sm_scale, dist):
            for step in range(n_steps):
                q, k, v = _mk(L, Hq, s, g, D, gain), _mk(L, H, s, g, D), _mk(L, H, s, g, D)
                kw = dict(policy=policy, phase="prefill", accumulate=True, evict=True, budget=budget_p, recent=recent, sink=sink, stride=s,
                          tova_head_mean=False)
                if bank is not None:
                    plan = StepPlan(two_pass=two_pass, n_split=n_split, **kw)
                    info = bank.step_info(plan, s)
                    # a capped step: never the wide, the logits-in-LDS or the resident kernel — blocks of <= 32 folded rows on the 16x16 kernel
                    assert cap is None or (info["wide"] == 0 and info["qb_rows"] * rep <= 32 and info["n_qblocks"] == -(-s // info["qb_rows"])), (name, info)
                    assert expect is None or all(info[k_] == v_ for k_, v_ in expect.items()), (name, info, expect)
                    assert two_pass == 0 or info["two_pass"] == (1 if two_pass == 1 else 0), (name, info)
                    assert n_split == 0 or (info["n_split"] == n_split and not info["fused"]), (name, info)
                    if shape == "mha_s8_one_pass_tail":
                        assert info["fused"] == 1 and info["two_pass"] == 0 and info["n_launches"] == 1, (name, info)
                    if shape == "mha_s40_two_blocks":
                        assert info["n_qblocks"] == 2 and info["two_pass"] == 1, (name, info)
                    out, ids = bank.attend(plan, q.cuda(), k.cuda(), v.cuda())
                for l in range(L):
                    if not bool(alive[l].any()):
                        continue
                    o_ref, ids_ref = O.layer_step(sts[l], q[l:l + 1].float(), k[l:l + 1].float(), v[l:l + 1].float(), O.StepPlan(**kw))
                    ref = torch.sort(ids_ref, dim=-1)[0]
                    if bank is not None:
                        rows = alive[l].repeat_interleave(rep)
                        got_o = out[l].float().cpu()
                        assert out_close(got_o[rows], o_ref[0][rows]), (name, step, l, float((got_o[rows] - o_ref[0][rows]).abs().max()))
                        got = torch.sort(ids[l].cpu().long(), dim=-1)[0]
                    for h in range(H):
                        if not bool(alive[l, h]):
                            continue
                        if bool(hook.probe.last_unstable[h]):
                            alive[l, h] = False
                            continue
                        tied = False
                        if policy == "roco":
                            c = hook.cap
                            forced, pool, need = feasible_classes(O.roco_std(c.s, c.q, c.c, sink)[h], k1)
                            tied = len(pool) != need
                            if bank is not None:
                                assert valid_victims(got[h].tolist(), (c.s / c.c)[h], forced, pool, need, s), (name, step, l, h)
                        if tied:
                            alive[l, h] = False
                            continue
                        if bank is not None:
                            assert bool((got[h] == ref[h]).all()), (name, step, l, h, got[h].tolist(), ref[h].tolist())
                        n_checked += 1
    finally:
        O.SELECT_HOOK = None
    if bank is not None:
        assert bank.n_slots == [idx] * L
        _permutation(bank)
    print(f"[softcap] {name}: max |o - o of the uncapped, standard-scale oracle| over the run = {dist[0]:.3e}")
    assert dist[0] >= 10 * OUT_BOUND, (name, dist[0])
    _enough(name, n_checked, n_steps * L * H)
    return n_checked, n_steps * L * H, dist[0]


@pytest.mark.parametrize("shape,D,regime,seed", CHUNK_CASES, ids=[f"{c[0]}-d{c[1]}-{c[2]}" for c in CHUNK_CASES])
def test_capped_chunk_steps(shape, D, regime, seed):
    run_chunk_case(shape, D, regime, seed)


@pytest.mark.parametrize("D", [256, 128])
def test_capped_dense_prefix_of_three_blocks(D):
    """An unscored causal prefix of 70 tokens: three query blocks of the one-tile build (32 + 32 + 6 rows), every block stopping at its
    own causal bound."""
    from easykv_amd import KVBank, StepPlan
    from oracle import easykv_oracle as O
    L, H, n, cap = 2, 2, 70, 2.0
    g = torch.Generator().manual_seed(32900 + D)
    q, k, v = _mk(L, H, n, g, D), _mk(L, H, n, g, D), _mk(L, H, n, g, D)
    bank = KVBank(L, H, H, D, cap=n + 64, logit_cap=cap)
    kw = dict(policy="full", phase="prefill", accumulate=False, evict=False, stride=n)
    info = bank.step_info(StepPlan(**kw), n)
    assert info["wide"] == 0 and info["n_qblocks"] == 3 and info["qb_rows"] == 32, info
    out, _ = bank.attend(StepPlan(**kw), q.cuda(), k.cuda(), v.cuda())
    dist = [0.0]
    with patched(cap, None, dist):
        for l in range(L):
            st = O.LayerState(k=torch.zeros(1, H, 0, D), v=torch.zeros(1, H, 0, D))
            o_ref, _ = O.layer_step(st, q[l:l + 1].float(), k[l:l + 1].float(), v[l:l + 1].float(), O.StepPlan(**kw))
            assert out_close(out[l].float().cpu(), o_ref[0]), (D, l, float((out[l].float().cpu() - o_ref[0]).abs().max()))
    assert dist[0] >= 10 * OUT_BOUND, dist[0]
    assert bank.n_slots == [n] * L


@pytest.mark.parametrize("D", [256, 128])
def test_capped_chunk_steps_bf16(D):
    """bf16 rows: the two-pass scheme of the capped 16x16 kernel under the bf16 bar of tests/test_hip_bf16.py."""
    import tests.test_hip_bf16 as TBF
    from easykv_amd import KVBank, StepPlan
    from oracle import easykv_oracle as O
    from tests.test_hip_lockstep import Hook
    BF = torch.bfloat16
    L, hq, h, idx, stride, policy, cap = 2, 4, 2, 480, 16, "h2o_head", 2.0
    W = idx + stride
    g = torch.Generator().manual_seed(32950 + D)
    bank = KVBank(L, hq, h, D, cap=W, dtype=BF, logit_cap=cap)
    bank.load_rows(torch.randn(L, h, idx, D, generator=g).to(BF).cuda(), torch.randn(L, h, idx, D, generator=g).to(BF).cuda())
    bank.state_init(W, 2, stride)
    kw = dict(policy=policy, phase="prefill", accumulate=True, evict=True, budget=idx, recent=int(idx * 0.1), sink=4, stride=stride)
    plan, oplan = StepPlan(two_pass=1, **kw), O.StepPlan(**kw)
    info = bank.step_info(plan, stride)
    assert info["wide"] == 0 and info["two_pass"] == 1, info
    hook = Hook()
    O.SELECT_HOOK = hook
    try:
        with patched(cap):
            for i in range(3):
                states = TBF._seed(bank, W)
                q, k, v = (torch.randn(L, hh, stride, D, generator=g).to(BF) for hh in (hq, h, h))
                out, ids = bank.attend(plan, q.cuda(), k.cuda(), v.cuda())
                assert out.dtype == BF
                for l in range(L):
                    st = states[l]
                    k_all, v_all = torch.cat([st.k[0], k[l].float()], 1), torch.cat([st.v[0], v[l].float()], 1)
                    pv = _pv_capped(q[l].float(), k_all, v_all, idx, cap)
                    o_ref, ids_ref = O.layer_step(st, q[l:l + 1].float(), k[l:l + 1].float(), v[l:l + 1].float(), oplan)
                    TBF._check_out(out[l], o_ref[0], pv, ("capped bf16 chunk", D, i, l))
                    TBF._check_ids(hook, ids[l].cpu(), ids_ref, ("capped bf16 chunk", D, i, l))
    finally:
        O.SELECT_HOOK = None
    assert bank.n_slots == [idx] * L
