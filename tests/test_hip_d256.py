"""head_dim 256 (Gemma-shaped models) on the GPU: every call that serves a 16-bit, plain-key bank serves one of head_dim 256.

The reference's attention has no notion of a head_dim (`repeat_kv`, `matmul`, `softmax`: easykv/llama_patch.py:19-29, :198-222).  Here a 512-byte row is 32 pieces of 16 bytes: the decode stream runs on lane groups of 32 (two rows per wave-load, the
group sums cross the DPP row boundary) and the chunk steps on the 16x16x32 MFMA kernel in blocks of at most 32 folded rows (eight
k-steps of QK^T, sixteen d-blocks of O^T).  Modelled on tests/test_hip_shape_generality.py: seeded randn(...).half() streams, the
oracle is O.layer_step per layer, outputs are held to tests.golden_util.out_close (the project's 1e-3 bar with its half-ulp
allowance), victims are compared exactly wherever the Probe of tests/test_hip_fullsize.py calls the decision stable, and the slot map
must end as a permutation of [0, cap).

The cap on what the probe may leave out: a case compares at least 10 decisions AND at least half of its evicting (step, layer, head)
triples.  Which decisions are unstable depends on the oracle alone, so the seeds below were chosen by running each case's oracle loop
with the probe on a CPU (`oracle_only=True` of the two case runners) — the compared / total counts a case prints on the GPU are the
ones that run printed.  The bf16 cases go through the case runners of tests/test_hip_bf16.py and are held to that file's bf16 bar."""
import contextlib
import io

import numpy as np
import pytest
import torch

from tests.golden_util import out_close
from tests.test_hip_fullsize import Probe

pytestmark = pytest.mark.gpu
D = 256


def _mk(L, H, n, g, d=D):
    return torch.randn(L, H, n, d, generator=g).half()


def _permutation(bank):
    m = bank.slot_of_pos.cpu().numpy()
    for l in range(m.shape[0]):
        for h in range(m.shape[1]):
            assert np.array_equal(np.sort(m[l, h]), np.arange(bank.cap)), (l, h)


def _enough(tag, n_checked, n_total):
    print(f"[d256] {tag}: compared {n_checked} of {n_total} evicting (step, layer, head) decisions")
    assert n_checked >= 10, (tag, n_checked, "too few well-defined decisions to be a meaningful test")
    assert 2 * n_checked >= n_total, (tag, n_checked, n_total, "the stability probe left out more than half of the decisions")


# ---- decode steps ---------------------------------------------------------------------------------------------------------------------
# budget + 25 steps from a 5-row prompt: every cache length from 5 to budget + 1, so odd lengths (half a wave-load at two rows per
# load) and lengths on either side of every RW = 16 and RW * NW = 64 / 128 boundary.  one_launch: None = the step moves from the
# one-launch kernel to the split path as the cache grows past one key range of 128 rows (n_split = 0 with few heads, and an explicit
# n_split > 1, whose ranges are at least 128 rows); both paths must have been visited
DECODE_CASES = [
    # id, rep, H, L, budget, n_split, policy, one_launch, seed
    ("mha_roco_fused4", 1, 4, 2, 140, 1, "roco", True, 1),
    ("gqa2_h2o_split2", 2, 2, 2, 160, 2, "h2o_head", None, 2),
    ("gqa3_roco_fused4", 3, 2, 2, 75, 1, "roco", True, 3),
    ("gqa4_tova_split3", 4, 2, 2, 200, 3, "tova", None, 4),
    ("gqa7_roco_auto", 7, 2, 2, 150, 0, "roco", None, 5),
    ("gqa8_h2o_fused4", 8, 1, 3, 60, 1, "h2o_head", True, 6),
    ("gqa8_recency_auto", 8, 2, 2, 60, 0, "recency", None, 7),
    ("gqa12_roco_groups_of_8", 12, 1, 3, 70, 0, "roco", False, 8),
    ("mha_tova_fused8_256_heads", 1, 16, 16, 60, 0, "tova", True, 9),
]


def run_decode_case(name, rep, H, L, budget, n_split, policy, one_launch, seed, oracle_only=False):
    from oracle import easykv_oracle as O
    Hq, P = H * rep, 5
    steps = budget + 25
    g = torch.Generator().manual_seed(25600 + seed)
    qs, ks, vs = _mk(L, Hq, P + steps, g), _mk(L, H, P + steps, g), _mk(L, H, P + steps, g)
    bank = None
    if not oracle_only:
        from easykv_amd import KVBank, StepPlan
        bank = KVBank(L, Hq, H, D, cap=P + budget + 1)
        bank.load_rows(ks[:, :, :P].cuda(), vs[:, :, :P].cuda())
        bank.state_init(budget + 1, 0)
    sts = []
    for l in range(L):
        st = O.LayerState(k=ks[l:l + 1, :, :P].float(), v=vs[l:l + 1, :, :P].float())
        st.s, st.q, st.c = O.init_state_decoding((H,), budget)
        sts.append(st)
    alive = torch.ones(L, H, dtype=torch.bool)
    probe = Probe()
    O.SELECT_HOOK = probe
    n_checked = n_total = n_fused = 0
    scored = policy != "recency"
    try:
        for i in range(steps):
            t = P + i
            T_prev = P + i if i <= budget else P + budget      # slots before this step's append
            evict = (T_prev + 1 - P) > budget
            rs = (P + (i % 7)) if (policy == "recency" and evict) else -1
            kw = dict(policy=policy, phase="decode", evict=evict, score_off=P, budget=budget, range_start=rs)
            if bank is not None:
                assert bank.n_slots[0] == T_prev
                plan = StepPlan(n_split=n_split, **kw)
                fused = bool(bank.step_info(plan, 1)["fused"])
                if one_launch is not None:
                    assert fused == one_launch, (name, i, bank.step_info(plan, 1))      # no silent fall-back to the other path
                n_fused += fused
                out, ids = bank.attend(plan, qs[:, :, t:t + 1].cuda().contiguous(), ks[:, :, t:t + 1].cuda().contiguous(),
                                       vs[:, :, t:t + 1].cuda().contiguous())
            for l in range(L):
                if scored and not bool(alive[l].any()):
                    continue
                o_ref, ids_ref = O.layer_step(sts[l], qs[l:l + 1, :, t:t + 1].float(), ks[l:l + 1, :, t:t + 1].float(), vs[l:l + 1, :, t:t + 1].float(),
                                              O.StepPlan(**kw))
                if not scored:      # recency: the host's range, every head alike; the output is compared at every step
                    if bank is not None:
                        assert out_close(out[l].float().cpu(), o_ref[0]), (name, i, l, float((out[l].float().cpu() - o_ref[0]).abs().max()))
                        if evict:
                            assert bool((ids[l].cpu().long() == rs).all()), (name, i, l)
                    n_checked += H if evict else 0
                    n_total += H if evict else 0
                    continue
                if bank is not None:
                    # a head that left the oracle's trajectory keeps other K/V rows from then on: its outputs are no longer comparable
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
        if one_launch is None and scored:
            assert 0 < n_fused < steps, (name, n_fused)      # both paths were visited
        assert bank.n_slots == [P + budget] * L
        _permutation(bank)
    _enough(name, n_checked, n_total)
    return n_checked, n_total


@pytest.mark.parametrize("name,rep,H,L,budget,n_split,policy,one_launch,seed", DECODE_CASES, ids=[c[0] for c in DECODE_CASES])
def test_decode_steps_at_head_dim_256(name, rep, H, L, budget, n_split, policy, one_launch, seed):
    run_decode_case(name, rep, H, L, budget, n_split, policy, one_launch, seed)


def test_decode_steps_on_the_slot_indexed_layout():
    """A whole-cache decode step (score_off = 0) of 256 heads: the 8-wave one-launch build on the slot-indexed score rows, which the
    planner's rule admits at head_dim 256 as at any other.  The bank must report the layout in use."""
    from easykv_amd import KVBank, StepPlan
    from oracle import easykv_oracle as O
    L, H, budget, steps = 32, 8, 70, 12
    T = budget + 1
    g = torch.Generator().manual_seed(25616)
    k0, v0 = _mk(L, H, budget, g), _mk(L, H, budget, g)
    warm = torch.rand(L, H, T, generator=g) * 1e-3
    bank = KVBank(L, H, H, D, cap=T + 63)
    bank.load_rows(k0.cuda(), v0.cuda())
    bank.state_init(T, 0)
    bank.score_sum[:, :, :T] += warm.cuda()
    bank.score_sq[:, :, :T] += (warm ** 2).cuda()
    sts = []
    for l in range(L):
        st = O.LayerState(k=k0[l:l + 1].float(), v=v0[l:l + 1].float())
        st.s, st.q, st.c = O.init_state_decoding((H,), budget)
        st.s += warm[l]
        st.q += warm[l] ** 2
        sts.append(st)
    plan = StepPlan(policy="roco", phase="decode", evict=True, budget=budget)
    info = bank.step_info(plan, 1)
    assert info["fused"] == 1 and info["n_launches"] == 1, info
    alive = torch.ones(L, H, dtype=torch.bool)
    probe = Probe()
    O.SELECT_HOOK = probe
    n_checked = n_total = n_slot = 0
    try:
        for i in range(steps):
            q, k, v = _mk(L, H, 1, g), _mk(L, H, 1, g), _mk(L, H, 1, g)
            out, ids = bank.attend(plan, q.cuda(), k.cuda(), v.cuda())
            n_slot += int(all(bank._slot_rows))
            for l in range(L):
                o_ref, ids_ref = O.layer_step(sts[l], q[l:l + 1].float(), k[l:l + 1].float(), v[l:l + 1].float(),
                                              O.StepPlan(policy="roco", phase="decode", evict=True, budget=budget))
                got_o = out[l].float().cpu()
                assert out_close(got_o[alive[l]], o_ref[0][alive[l]]), (i, l)
                ok = ~probe.last_unstable
                same = ids[l, :, 0].cpu().long() == ids_ref[:, 0]
                assert bool(same[ok & alive[l]].all()), (i, l)
                n_total += H
                n_checked += int((ok & alive[l]).sum())
                alive[l] &= ok & same
    finally:
        O.SELECT_HOOK = None
    assert n_slot == steps, n_slot      # every step ran on the slot-indexed layout
    _enough("slot_rows_fused8", n_checked, n_total)
    _permutation(bank)


def test_decode_steps_bf16():
    """bf16 rows, 256 heads in the launch: the 8-wave one-launch build on the slot-indexed layout, and the split path with the fold,
    under the bf16 bar of tests/test_hip_bf16.py."""
    import tests.test_hip_bf16 as TBF
    TBF.test_decode_against_the_oracle("d256 fused 32 layers roco", 32, 8, 8, D, 48, "roco", 0, False, (1, True, False))
    TBF.test_decode_against_the_oracle("d256 split + fold tova GQA3", 2, 24, 8, D, 600, "tova", 4, False, (0, False, True))


# ---- chunk steps ----------------------------------------------------------------------------------------------------------------------
CHUNK_CASES = [
    # id, rep, H, stride, idx, policy, two_pass, n_split, seed
    ("mha_s3_tova", 1, 3, 3, 120, "tova", 0, 0, 1),
    ("gqa2_s8_roco", 2, 2, 8, 210, "roco", 0, 0, 2),
    ("gqa3_s16_h2o_two_blocks", 3, 2, 16, 300, "h2o_head", 0, 0, 3),          # 48 folded rows: two blocks of 10 queries x 3 heads, one pass
    ("gqa4_s16_roco_two_pass_auto", 4, 2, 16, 330, "roco", 0, 0, 4),           # 64 folded rows: the planner's two passes, two blocks
    ("mha_s64_roco_two_pass", 1, 2, 64, 500, "roco", 1, 0, 5),
    ("mha_s64_roco_one_pass", 1, 2, 64, 500, "roco", -1, 0, 5),
    ("mha_s130_tova_five_blocks", 1, 2, 130, 700, "tova", 0, 0, 6),
    ("gqa2_s8_roco_forced_split", 2, 2, 8, 400, "roco", 0, 2, 7),
    ("mha_s16_h2o_forced_split_two_pass", 1, 3, 16, 640, "h2o_head", 1, 3, 8),
]


class _ProbeAndCapture:
    """oracle.SELECT_HOOK: the stability probe plus the rows the selection saw (tests/select_rule.py)."""

    def __init__(self):
        from tests.select_rule import Capture
        self.probe, self.cap = Probe(), Capture()

    def __call__(self, *args):
        self.probe(*args)
        self.cap(*args)


def run_chunk_case(name, rep, H, s, idx, policy, two_pass, n_split, seed, oracle_only=False):
    """Evicting chunk steps of the encoding rule (easykv/easykv.py:443-499) from a cache of `idx` slots; a decision is compared exactly
    where the probe calls it stable and roco's feasible set does not cut through a tied class (tests/select_rule.py)."""
    from oracle import easykv_oracle as O
    from tests.select_rule import feasible_classes, valid_victims
    Hq, L, n_steps = H * rep, 2, 4
    budget_p, recent, sink = idx + s // 2, int(idx * 0.2), 4
    g = torch.Generator().manual_seed(25700 + seed)
    k0, v0 = _mk(L, H, idx, g), _mk(L, H, idx, g)
    bank = None
    if not oracle_only:
        from easykv_amd import KVBank, StepPlan
        bank = KVBank(L, Hq, H, D, cap=idx + s)
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
    try:
        for step in range(n_steps):
            q, k, v = _mk(L, Hq, s, g), _mk(L, H, s, g), _mk(L, H, s, g)
            kw = dict(policy=policy, phase="prefill", accumulate=True, evict=True, budget=budget_p, recent=recent, sink=sink, stride=s,
                      tova_head_mean=False)
            if bank is not None:
                plan = StepPlan(two_pass=two_pass, n_split=n_split, **kw)
                info = bank.step_info(plan, s)
                assert info["wide"] == 0 and info["qb_rows"] * rep <= 32 and info["n_qblocks"] == -(-s // info["qb_rows"]), (name, info)
                assert two_pass == 0 or info["two_pass"] == (1 if two_pass == 1 else 0), (name, info)
                assert n_split == 0 or (info["n_split"] == n_split and not info["fused"]), (name, info)
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
                        alive[l, h] = False      # (a valid outcome, but not necessarily torch's: the trajectories part here)
                        continue
                    if bank is not None:
                        assert bool((got[h] == ref[h]).all()), (name, step, l, h, got[h].tolist(), ref[h].tolist())
                    n_checked += 1
    finally:
        O.SELECT_HOOK = None
    if bank is not None:
        assert bank.n_slots == [idx] * L
        _permutation(bank)
    _enough(name, n_checked, n_steps * L * H)
    return n_checked, n_steps * L * H


@pytest.mark.parametrize("name,rep,H,s,idx,policy,two_pass,n_split,seed", CHUNK_CASES, ids=[c[0] for c in CHUNK_CASES])
def test_chunk_steps_at_head_dim_256(name, rep, H, s, idx, policy, two_pass, n_split, seed):
    run_chunk_case(name, rep, H, s, idx, policy, two_pass, n_split, seed)


def test_chunk_steps_bf16():
    import tests.test_hip_bf16 as TBF
    TBF.test_chunk_step_against_the_oracle("d256 16x16 two pass", 2, 8, 8, D, 480, 48, "h2o_head", 1, dict(wide=0, two_pass=1))
    TBF.test_chunk_step_against_the_oracle("d256 16x16 one pass, scorer tail", 2, 8, 8, D, 496, 16, "roco", -1, dict(wide=0, two_pass=0))


# ---- the drivers ------------------------------------------------------------------------------------------------------------------------
DRIVER_SEED = 41
DRIVER_CASES = [
    # mode, stride, prompt length, generation_config
    ("decoding", 8, 200, dict(budget=40, kv_policy="roco", max_new_tokens=70)),
    ("encoding", 8, 300, dict(budget=0.5, kv_policy="roco", max_new_tokens=12)),
    ("auto", 8, 300, dict(budget=120, kv_policy="roco", max_new_tokens=24, recent_ratio=0.3)),
    # keep_attention: the dense prefix is scored in query blocks — the column-sum pass of the two-pass scheme over the prefix
    ("encoding", 8, 260, dict(budget=0.5, kv_policy="h2o_head", keep_attention=True, max_new_tokens=8)),
]


def _streams(max_pos, seed=DRIVER_SEED, hq=4, h=2):
    from oracle.fake_model import make_streams
    return make_streams(2, hq, h, D, max_pos, seed=seed)


def _oracle_events(tr, shape_of):
    from tests.golden_util import trace_events
    kinds, ph, rg = trace_events(tr)
    ref = []
    for kind in kinds:
        if kind == 0:
            ref.append(ph.pop(0))
        else:
            lo, hi = rg.pop(0)
            ref.append(np.broadcast_to(np.arange(lo, hi, dtype=np.int32), shape_of(len(ref))))
    return ref


@pytest.mark.parametrize("mode,stride,length,cfg", DRIVER_CASES, ids=[c[0] + ("_keep_attention" if c[3].get("keep_attention") else "") for c in DRIVER_CASES])
def test_generate_equals_the_oracles_run(mode, stride, length, cfg):
    """easykv_amd.generate over a head_dim-256 fake model: the dense prefix, the strided prefill, state_init and the decode loop.  Every
    evicted id, the text and the printed budget line are the oracle's."""
    from tests.test_hip_generate_batch import _evictions, _run_oracle, _run_solo
    streams = _streams(length + cfg["max_new_tokens"] + 8)
    model, res, cache, line = _run_solo(streams, dict(cfg, _record_evictions=True), mode, stride, length)
    tr = _run_oracle(streams, cfg, mode, stride, length)
    ours = _evictions(cache.evictions)
    ref = _oracle_events(tr, lambda i: ours[i].shape)
    assert len(ours) == len(ref) > 0, (len(ours), len(ref))
    for step, (a, b) in enumerate(zip(ours, ref)):
        assert np.array_equal(a, b), (mode, f"eviction ids differ at eviction {step}")
    ref_text = tr.result if isinstance(tr.result, str) else " ".join(str(t) for t in tr.result)
    assert res == ref_text and line == tr.report.strip(), (res, ref_text, line, tr.report)
    assert cache.bank.head_dim == D


def test_generate_batch_equals_the_solo_runs():
    """Three prompts of different lengths decoded in one batched attend per layer: each sequence equals its solo run and the oracle's."""
    from tests.test_hip_generate_batch import _check_batch
    cfg = dict(budget=40, kv_policy="roco", max_new_tokens=60)
    model, cache, n_sel = _check_batch(_streams(200), cfg, "decoding", 1, (33, 48, 75))
    assert min(n_sel) > 0 and model.n_batched_forwards == cfg["max_new_tokens"]


# ---- batches ----------------------------------------------------------------------------------------------------------------------------
UNIFORM = [
    # id, Hq, H, B, rows, policy, dtype, n_split, one launch?
    ("fused8_roco", 8, 8, 32, 200, "roco", torch.float16, 0, True),             # B * H = 256: the 8-wave one-launch build
    ("fused4_gqa4_tova_bf16", 8, 2, 4, 300, "tova", torch.bfloat16, 1, True),   # explicit n_split = 1: the 4-wave build
    ("split_gqa3_roco", 6, 2, 3, 500, "roco", torch.float16, 4, False),         # split path + fast scorer
    ("split_recency_bf16", 8, 2, 2, 400, "recency", torch.bfloat16, 0, False),  # in-kernel fold + range compaction
]


@pytest.mark.parametrize("name,Hq,H,B,rows,policy,dtype,n_split,one_launch", UNIFORM, ids=[c[0] for c in UNIFORM])
def test_uniform_batch_is_the_multi_layer_step_bit_for_bit(name, Hq, H, B, rows, policy, dtype, n_split, one_launch):
    """Outputs, ids, slot maps, score rows and K/V of a uniform batch equal the multi-layer step it spells out, bit for bit."""
    import tests.test_hip_batch as TB
    TB.test_uniform_batch_is_the_multi_layer_step_bit_for_bit("d256_" + name, D, Hq, H, B, rows, policy, dtype, n_split, one_launch)


RAGGED_T = (2, 17, 130, 300)


@pytest.mark.parametrize("policy", ["roco", "h2o_head", "recency"])
@pytest.mark.parametrize("n_split", [1, 3], ids=["one_launch", "split"])
def test_ragged_batch_against_the_oracle(policy, n_split):
    """One table with T from 2 to 300, evicting and non-evicting entries mixed, against the oracle per entry."""
    import tests.test_hip_batch as TB
    from easykv_amd import KVBankBatch, StepPlan
    from oracle import easykv_oracle as O
    from tests.test_hip_lockstep import Hook
    Hq, H, B = 4, 2, len(RAGGED_T)
    g = torch.Generator().manual_seed(25631)
    bat = KVBankBatch(B, 1, Hq, H, D, cap=300 + 40)
    offs = {2: 0, 17: 5, 130: 0, 300: 21}
    evicts = {2: False, 17: False, 130: True, 300: True}
    plans, oplans, widths = [], [], []
    for i, T in enumerate(RAGGED_T):
        W = T - offs[T]
        TB._fill(bat.bank, i, T - 1, g, W)
        kw = dict(policy=policy, phase="decode", evict=evicts[T], score_off=offs[T], budget=W - 1,
                  range_start=T // 3 if (policy == "recency" and evicts[T]) else -1)
        plans.append(StepPlan(**kw))
        oplans.append(O.StepPlan(**kw))
        widths.append(W)
    info = bat.step_info(plans, 0, None, n_split)
    assert bool(info["fused"]) == (n_split == 1) and (n_split == 1 or info["n_split"] == 3), info
    seqs = [bat.sequence(i) for i in range(B)]
    hook = Hook()
    n_dec = n_class = 0
    O.SELECT_HOOK = hook
    try:
        for step in range(2):
            states = [TB._oracle_state(seqs[i], widths[i]) for i in range(B)]
            q, k, v = (_mk(B, hh, 1, g) for hh in (Hq, H, H))
            out, ids = bat.attend(plans, q.cuda(), k.cuda(), v.cuda(), 0, n_split=n_split)
            torch.cuda.synchronize()
            assert int(bat.bank.arrive.abs().sum()) == 0
            for i, T in enumerate(RAGGED_T):
                o_ref, ids_ref = O.layer_step(states[i], q[i:i + 1].float(), k[i:i + 1].float(), v[i:i + 1].float(), oplans[i])
                got = (ids[i] - (offs[T] if ids_ref is not None else 0)) if evicts[T] else None
                nd, nc = TB._check_entry(("d256", policy, n_split, step, T), hook, policy, o_ref, ids_ref, out[i], got, seqs[i], states[i], widths[i],
                                         evicts[T], plans[i].range_start)
                n_dec += nd
                n_class += nc
                assert bat.n_slots(i) == (T - 1 if evicts[T] else T + step), (T, step, bat.n_slots(i))
            for i, T in enumerate(RAGGED_T):
                if not evicts[T]:
                    widths[i] += 1
                    kw = dict(policy=policy, phase="decode", evict=False, score_off=offs[T], budget=widths[i] - 1, range_start=-1)
                    plans[i], oplans[i] = StepPlan(**kw), O.StepPlan(**kw)
    finally:
        O.SELECT_HOOK = None
    assert n_dec == 2 * 2 * H
    print(f"[d256] ragged batched step {policy} n_split={n_split}: {n_dec - n_class} exact + {n_class} in the tolerance class of {n_dec}")


# ---- the long family ------------------------------------------------------------------------------------------------------------------
def test_long_rows_chunk_step_is_the_plain_step_bit_for_bit():
    """Twin banks, plain and long_rows=True: a chunk step of stride 16 whose heads are split over two key ranges, so the plain plan ends
    in the generic scorer and the long plan in the long-row scorer.  Outputs, victims, slot maps and score rows are bit-identical."""
    import tests.test_hip_long_rows as TL
    from easykv_amd import StepPlan
    H, hq, idx, s = 2, 4, 608, 16
    g = torch.Generator().manual_seed(25640)
    k0, v0 = _mk(1, H, idx, g), _mk(1, H, idx, g)
    plain, long = banks = TL._twins(1, hq, H, D, idx + s)
    for b in banks:
        b.load_rows(k0.cuda(), v0.cuda())
        b.state_init(idx + s, 2, s)
    for policy, two_pass in (("roco", -1), ("h2o_head", 1)):
        kw = dict(policy=policy, phase="prefill", accumulate=True, evict=True, budget=idx, recent=int(idx * 0.1), sink=4, stride=s, n_split=2,
                  two_pass=two_pass)
        ip, il = TL._ends_in_the_two_scorers(plain, long, StepPlan(**kw), s)
        assert ip["n_split"] == 2 and ip["wide"] == 0, ip
        for step in range(2):
            q, k, v = (_mk(1, n_h, s, g).cuda() for n_h in (hq, H, H))
            _, ids = TL._step_both(plain, long, StepPlan(**kw), q, k, v, (policy, two_pass, step))
            assert ids.shape == (1, H, s)
    assert long.n_slots == [idx]
    _permutation(long)


# ---- the HF seam ------------------------------------------------------------------------------------------------------------------------
class _Tok:
    eos_token_id = -1

    def decode(self, ids, skip_special_tokens=True):
        return " ".join(str(i) for i in ids)


def _tiny_hf(kind, heads, kv_heads, seed):
    import transformers
    torch.manual_seed(seed)
    common = dict(vocab_size=97, hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=heads,
                  num_key_value_heads=kv_heads, head_dim=D, max_position_embeddings=512, attn_implementation="eager")
    if kind == "gemma":
        model = transformers.GemmaForCausalLM(transformers.GemmaConfig(**common))
    else:
        model = transformers.LlamaForCausalLM(transformers.LlamaConfig(**common))
    return model.half().cuda().eval()


@pytest.mark.parametrize("kind,heads,kv_heads", [("gemma", 4, 1), ("gemma", 2, 2), ("llama", 4, 2)], ids=["gemma-gqa4", "gemma-mha", "llama-gqa2"])
def test_stock_hf_models_of_head_dim_256_through_the_seam(kind, heads, kv_heads):
    """A stock GemmaForCausalLM (every Gemma model has head_dim 256; scaling = 1 / sqrt(256)) and a Llama of head_dim 256 through
    hf.patch_model + enable_fixed_kv.  At full budget: the logits of the patched forward against the model's own eager attention
    (atol = rtol = 3e-2, the bar of tests/test_hip_hf_adapter.py) and the greedy tokens against HF's own generate.  Under half the
    prompt as budget with roco in auto mode (the mode takes an integer budget): the run completes with the reference's budget line and
    the cache length the geometry gives."""
    import easykv_amd
    from easykv_amd import hf
    model = _tiny_hf(kind, heads, kv_heads, seed=heads * 10 + kv_heads)
    assert model.model.layers[0].self_attn.scaling == 0.0625 and model.config.head_dim == D
    ids = torch.randint(0, 97, (1, 40), device="cuda")
    with torch.inference_mode():
        ref_logits = model(input_ids=ids).logits.float()
        ref_tokens = model.generate(ids, max_new_tokens=8, do_sample=False)[0, 40:].tolist()
    hf.patch_model(model)
    easykv_amd.enable_fixed_kv(model, _Tok(), mode="decoding", stride=1)
    cache = easykv_amd.BudgetedKVCache(2, heads, kv_heads, D, 64, torch.device("cuda"))
    with torch.inference_mode(), cache.active(easykv_amd.StepPlan(policy="full", phase="prefill", accumulate=False)):
        got = model(input_ids=ids, past_key_values=cache, position_ids=torch.arange(40, device="cuda").view(1, -1), use_cache=True).logits.float()
    assert torch.allclose(got, ref_logits, atol=3e-2, rtol=3e-2), float((got - ref_logits).abs().max())
    with contextlib.redirect_stdout(io.StringIO()):
        out = model.easykv_generate(input_ids=ids, generation_config=dict(temperature=1e-6, kv_policy="full", budget=200, max_new_tokens=8, eos_token_ids=[-1]))
    assert [int(t) for t in out.split()] == ref_tokens
    # eviction: auto mode at half the prompt, stride 8
    ids2 = torch.randint(0, 97, (1, 120), device="cuda")
    gc = dict(budget=60, kv_policy="roco", max_new_tokens=6, recent_ratio=0.3, eos_token_ids=[-1], temperature=1e-6)
    easykv_amd.enable_fixed_kv(model, _Tok(), mode="auto", stride=8)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        out, cache = model.easykv_generate(input_ids=ids2, generation_config=gc, return_cache=True)
    bp, idx, _ = easykv_amd.geometry("auto", 120, 60, 8)
    assert len(out.split()) == 6 and cache.get_seq_length() == idx
    line = buf.getvalue().strip()      # (easykv/easykv.py:751: the whole cache over prompt + generated tokens)
    assert line.startswith("KV Cache Budget ratio") and line.endswith(f"[{idx}/(120+6)]") and "\n" not in line, line
    with pytest.raises(ValueError, match="256"):
        model.easykv_generate(input_ids=ids2, generation_config=dict(gc, streaming=True))


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_at_head_dim_256_raise_before_any_launch():
    import easykv_amd
    from easykv_amd import KVBank, KVBankBatch
    from easykv_amd._lib import EkvError
    from oracle import easykv_oracle as O
    from tests.native_fake_model import NativeFakeModel
    g = torch.Generator().manual_seed(3)
    bank = KVBank(1, 2, 2, D, cap=64)
    bank.load_rows(_mk(1, 2, 20, g).cuda(), _mk(1, 2, 20, g).cuda())
    k_before = bank.k.clone()
    with pytest.raises(EkvError, match="256"):
        bank.set_rope(*O.rope_tables(64, D))
    for name in ("quantize_fp8", "quantize_mxfp4", "quantize_mxfp6", "quantize_fp8_mxfp4", "quantize_k16_mxfp4"):
        with pytest.raises(EkvError, match="256"):
            getattr(bank, name)()
    assert torch.equal(bank.k, k_before) and bank.n_slots == [20]
    for kind in ("fp8", "mxfp4", "mxfp6", "fp8_mxfp4", "k16_mxfp4"):
        with pytest.raises(EkvError, match="256"):
            KVBank(1, 2, 2, D, cap=64, kv_quant=kind)
        with pytest.raises(EkvError, match="256"):
            KVBankBatch(2, 1, 2, 2, D, cap=64, kv_quant=kind)
    model = NativeFakeModel(*_streams(64, hq=2, h=2))
    ids = torch.arange(24).view(1, -1) % 16
    with pytest.raises(ValueError, match="256"):
        easykv_amd.generate(model, ids, dict(budget=8, kv_policy="roco", max_new_tokens=4, streaming=True), kv_mode="decoding", stride=1)
    with pytest.raises(ValueError, match="256"):
        easykv_amd.generate(model, ids, dict(budget=8, kv_policy="roco", max_new_tokens=4, kv_quant="fp8"), kv_mode="decoding", stride=1)
    assert model.outputs_log == []      # no forward ran
