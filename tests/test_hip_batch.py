"""Batched decode steps (include/easykv_hip.h, ekv_seq; easykv_amd.KVBankBatch) on the GPU.

  * a UNIFORM batch is the existing multi-layer step, bit for bit: outputs, evicted ids, slot maps and score rows (the batch
    instances of the kernels are the uniform kernels with the per-step fields read from the table);
  * a RAGGED batch — entries from 2 to 2049 slots in one launch, evicting and non-evicting entries mixed, per-entry score offset and
    roco window — against the oracle on each entry's own rows, on the one-launch kernel and on the split path (where the key-range
    splits past a short entry's end are empty);
  * 96 consecutive ragged steps of five sequences with different prompt lengths and budgets, one of them retired half-way, every
    step of every sequence re-seeded and compared as tests/test_hip_lockstep.py does for one sequence, and the survivors' victims
    equal to those of a run the retired sequence never took part in.

  * a sequence prefilled and stepped ALONE through ``KVBankBatch.sequence(i)`` (the single-sequence calls, which move its layers to
    the slot-indexed score-row layout) and then served by the batched call: the layout bookkeeping is the shared bank's.

  * the ragged edges again in bf16, head_dim 96, GQA 3, on the 8-wave one-launch build.

``generate_batch`` and the HF seam: tests/test_hip_generate_batch.py."""
import pytest
import torch

from tests.golden_util import out_close
from tests.test_hip_lockstep import Hook

pytestmark = pytest.mark.gpu


def _fill(bank, layer, n_rows, g, width, warm=True):
    """Rows in a scattered slot map (a bank whose rows have been recycled for many steps) + a warm decoding score state."""
    h, d = bank.n_kv_heads, bank.head_dim
    k0, v0 = (torch.randn(1, h, n_rows, d, generator=g).to(bank.dtype) for _ in range(2))
    bank.load_rows(k0.cuda(), v0.cuda(), layer_begin=layer)
    perm = torch.argsort(torch.rand(h, n_rows, generator=g), dim=-1).int().cuda()
    idx = perm.long().unsqueeze(-1).expand(-1, -1, d)
    kk, vv = bank.k[layer, :, :n_rows].clone(), bank.v[layer, :, :n_rows].clone()
    bank.k[layer, :, :n_rows].scatter_(1, idx, kk)
    bank.v[layer, :, :n_rows].scatter_(1, idx, vv)
    bank.slot_of_pos[layer, :, :n_rows] = perm
    bank.state_init(width, 0, layer_begin=layer, layer_count=1)
    live = max(0, min(width - 1, n_rows))      # (the column the next token takes starts at zero, as the reference appends it)
    if warm and bank.score_sum is not None and live > 0:
        w = torch.rand(h, live, generator=g) * 1e-3
        bank.score_sum[layer, :, :live] += w.cuda()
        bank.score_sq[layer, :, :live] += (w ** 2).cuda()


def _copy_layer(src, ls, dst, ld):
    for name in ("k", "v", "slot_of_pos", "score_sum", "score_sq", "score_cnt"):
        getattr(dst, name)[ld].copy_(getattr(src, name)[ls])
    dst.n_slots[ld], dst.extent[ld] = src.n_slots[ls], src.extent[ls]


UNIFORM = [
    # id, D, Hq, H, B, rows, policy, dtype, n_split, one launch?
    ("fused8_d128_roco", 128, 32, 32, 8, 300, "roco", torch.float16, 0, True),            # B * H = 256: the 8-wave one-launch build
    ("fused4_d64_gqa4_tova_bf16", 64, 8, 2, 4, 700, "tova", torch.bfloat16, 1, True),      # explicit n_split = 1: the 4-wave build
    ("fused4_1024heads_h2o", 64, 32, 32, 32, 130, "h2o_head", torch.float16, 0, True),     # B * H = 1024: the 4-wave build by itself
    ("fused8_d96_gqa3_roco_bf16", 96, 24, 8, 32, 200, "roco", torch.bfloat16, 0, True),    # head_dim 96, GQA 3, B * H = 256
    ("split_d96_gqa3_roco", 96, 24, 8, 3, 700, "roco", torch.float16, 4, False),           # split path + fast scorer
    ("split_d128_h2o_bf16", 128, 32, 32, 2, 2048, "h2o_head", torch.bfloat16, 0, False),
    ("split_d64_gqa4_tova", 64, 8, 2, 5, 1300, "tova", torch.float16, 3, False),
    ("split_d128_recency_bf16", 128, 32, 8, 2, 500, "recency", torch.bfloat16, 0, False),  # in-kernel fold + range compaction
    ("split_d32_full", 32, 4, 4, 3, 400, "full", torch.float16, 2, False),                 # nothing scored: the in-kernel fold alone
]


@pytest.mark.parametrize("name,D,Hq,H,B,rows,policy,dtype,n_split,one_launch", UNIFORM, ids=[c[0] for c in UNIFORM])
def test_uniform_batch_is_the_multi_layer_step_bit_for_bit(name, D, Hq, H, B, rows, policy, dtype, n_split, one_launch):
    from easykv_amd import KVBank, KVBankBatch, StepPlan
    g = torch.Generator().manual_seed(1000 + rows + B)
    T = rows + 1
    ref = KVBank(B, Hq, H, D, cap=T + 6, dtype=dtype)
    ref.use_slot_rows = False      # like against like: a batch runs the ordered score-row layout
    ref.k.zero_(), ref.v.zero_()   # (whole layers are compared below: no uninitialised rows)
    for l in range(B):
        _fill(ref, l, rows, g, T)
    LPS, layer = 3, 1      # the batch bank: [sequence][layer], the call serves model layer 1 of every sequence, in permuted order
    bat = KVBankBatch(B, LPS, Hq, H, D, cap=T + 6, dtype=dtype)
    order = [(5 * i + 2) % B for i in range(B)] if B % 5 else list(reversed(range(B)))
    assert sorted(order) == list(range(B))
    for i, s in enumerate(order):
        _copy_layer(ref, i, bat.bank, s * LPS + layer)
    budget = rows - 3
    plan = StepPlan(policy=policy, phase="decode", evict=policy != "full", score_off=0, budget=budget, n_split=n_split,
                    range_start=7 if policy == "recency" else -1)
    info = bat.step_info([plan] * B, layer, order, n_split)
    assert info == ref.step_info(plan, 1, 0, B), (info, ref.step_info(plan, 1, 0, B))
    assert bool(info["fused"]) == one_launch, info
    for step in range(3):
        q, k, v = (torch.randn(B, hh, 1, D, generator=g).to(dtype).cuda() for hh in (Hq, H, H))
        o1, ids1 = ref.attend(plan, q, k, v)
        o2, ids2 = bat.attend([plan] * B, q, k, v, layer, active=order, n_split=n_split)
        torch.cuda.synchronize()
        assert torch.equal(o1, o2), (name, step, float((o1.float() - o2.float()).abs().max()))
        if policy == "full":
            assert ids1 is None and ids2 is None
        else:
            assert torch.equal(ids1, ids2), (name, step)
        for i, s in enumerate(order):
            lb = s * LPS + layer
            assert bat.bank.n_slots[lb] == ref.n_slots[i] and bat.bank.extent[lb] == ref.extent[i]
            for arr in ("slot_of_pos", "score_sum", "score_sq", "score_cnt", "k", "v"):
                assert torch.equal(getattr(bat.bank, arr)[lb], getattr(ref, arr)[i]), (name, step, i, arr)
        assert int(bat.bank.arrive.abs().sum()) == 0      # the arrival counters of the in-kernel fold are left at zero
    # the other layers of the batch bank were never touched
    assert all(bat.bank.n_slots[s * LPS + l] == 0 for s in range(B) for l in (0, 2))


def _oracle_state(seq, W):
    """Oracle layer state = the sequence's own one-layer bank (ordered rows in birth order, score rows of width W)."""
    from oracle import easykv_oracle as O
    kk, vv = seq.ordered_kv()
    st = O.LayerState(k=kk[0:1].float().cpu(), v=vv[0:1].float().cpu())
    st.s, st.q, st.c = (getattr(seq, a)[0, :, :W].cpu().clone() for a in ("score_sum", "score_sq", "score_cnt"))
    return st


def _check_entry(tag, hook, policy, o_ref, ids_ref, out_i, ids_i, seq, st, W, evict, range_start=-1, check_out=None):
    """One entry of a batched step against the oracle's step from the same state: output, decision (equal, or one of the oracle's own
    answers under +-2e-5), score rows of the heads that took the oracle's decision."""
    if check_out is not None:      # (bf16 banks: the project's bf16 bar, tests/test_hip_bf16.py)
        check_out(out_i, o_ref[0])
    else:
        assert out_close(out_i.float().cpu(), o_ref[0]), (tag, float((out_i.float().cpu() - o_ref[0]).abs().max()))
    h = ids_i.shape[0] if ids_i is not None else 0
    n_class = 0
    same = torch.ones(st.s.shape[0], dtype=torch.bool)
    if evict and ids_ref is not None:
        got = ids_i[:, 0].cpu().long()
        same = got == ids_ref[:, 0]
        for hh in (~same).nonzero().flatten().tolist():
            assert hook.in_tolerance_class(hh, got[hh:hh + 1]), (tag, hh, "not one of the oracle's answers under +-2e-5")
            n_class += 1
    if evict and ids_ref is None:      # recency / random: the host-chosen range, every head alike
        assert bool((ids_i[:, 0].cpu() == range_start).all()), (tag, ids_i[:, 0].tolist(), range_start)
    # the cache after the step, in birth order: the appended row is there and the victim's slot is gone
    kk, vv = seq.ordered_kv()
    assert torch.equal(kk[0].cpu()[same], st.k[0].to(kk.dtype)[same]) and torch.equal(vv[0].cpu()[same], st.v[0].to(vv.dtype)[same]), tag
    w = W - (1 if evict else 0)
    S2 = seq.score_sum[0, :, :w].cpu()
    assert torch.allclose(S2[same], st.s[:, :w][same], rtol=2e-5, atol=1e-9), tag
    if policy == "roco":
        assert torch.allclose(seq.score_sq[0, :, :w].cpu()[same], st.q[:, :w][same], rtol=2e-5, atol=1e-12), tag
        assert torch.equal(seq.score_cnt[0, :, :w].cpu()[same], st.c[:, :w][same]), tag
    return h, n_class


RAGGED_T = (2, 17, 130, 700, 1301, 2049)



@pytest.mark.parametrize("policy", ["roco", "h2o_head", "recency", "full"])
@pytest.mark.parametrize("n_split", [1, 8], ids=["one_launch", "split"])
@pytest.mark.parametrize("draw", [0, 1], ids=["short_first", "short_last"])
def test_ragged_step_against_the_oracle(policy, n_split, draw):
    from easykv_amd import KVBankBatch, StepPlan
    from oracle import easykv_oracle as O
    Hq, H, D, B = 8, 4, 128, len(RAGGED_T)
    g = torch.Generator().manual_seed(31 + draw)
    bat = KVBankBatch(B, 1, Hq, H, D, cap=2049 + 40)
    lens = list(RAGGED_T) if draw == 0 else [2049, 1301, 700, 130, 17, 2]
    # per entry: the score rows start at its own offset (decoding mode: the prompt length), and it evicts only when its own length
    # has passed its own budget — entries with and without a victim share the launch
    offs = {2: 0, 17: 5, 130: 0, 700: 321, 1301: 7, 2049: 0}
    evicts = {2: False, 17: False, 130: True, 700: False, 1301: True, 2049: True}
    plans, oplans, widths = [], [], []
    for i, T in enumerate(lens):
        W = T - offs[T]
        _fill(bat.bank, i, T - 1, g, W)
        if policy == "full":
            evicts[T] = False
        kw = dict(policy=policy, phase="decode", evict=evicts[T], score_off=offs[T], budget=W - 1,
                  range_start=T // 3 if (policy == "recency" and evicts[T]) else -1)
        plans.append(StepPlan(**kw))
        oplans.append(O.StepPlan(**kw))
        widths.append(W)
    info = bat.step_info(plans, 0, None, n_split)
    assert bool(info["fused"]) == (n_split == 1) and (n_split == 1 or info["n_split"] >= 4), info      # (split: ranges past T = 2 .. 1301 are empty)
    seqs = [bat.sequence(i) for i in range(B)]
    hook = Hook()
    n_dec = n_class = 0
    O.SELECT_HOOK = hook
    try:
        for step in range(2):
            states = [_oracle_state(seqs[i], widths[i]) for i in range(B)]
            q, k, v = (torch.randn(B, hh, 1, D, generator=g).half() for hh in (Hq, H, H))
            out, ids = bat.attend(plans, q.cuda(), k.cuda(), v.cuda(), 0, n_split=n_split)
            torch.cuda.synchronize()
            assert int(bat.bank.arrive.abs().sum()) == 0
            for i, T in enumerate(lens):
                o_ref, ids_ref = O.layer_step(states[i], q[i:i + 1].float(), k[i:i + 1].float(), v[i:i + 1].float(), oplans[i])
                # (the oracle's ids are relative to the score rows; the library reports cache positions — a range is one already)
                got = (ids[i] - (offs[T] if ids_ref is not None else 0)) if evicts[T] else None
                nd, nc = _check_entry((policy, n_split, draw, step, T), hook, policy, o_ref, ids_ref, out[i], got, seqs[i], states[i], widths[i],
                                      evicts[T], plans[i].range_start)
                n_dec += nd
                n_class += nc
                # the entry's length after the step: it grew by the token unless it evicted
                assert bat.n_slots(i) == (T - 1 if evicts[T] else T + step), (T, step, bat.n_slots(i))
            for i, T in enumerate(lens):      # entries that do not evict grow: their score rows and budget follow (as a decode loop's would)
                if not evicts[T]:
                    widths[i] += 1
                    kw = dict(policy=policy, phase="decode", evict=False, score_off=offs[T], budget=widths[i] - 1, range_start=-1)
                    plans[i], oplans[i] = StepPlan(**kw), O.StepPlan(**kw)
    finally:
        O.SELECT_HOOK = None
    assert n_dec == (0 if policy == "full" else 2 * 3 * H)
    print(f"[bound-fraction] ragged batched step {policy} n_split={n_split} draw={draw}: {n_dec - n_class} exact + {n_class} in the tolerance class of {n_dec}")


def _run_lockstep(prompts, budgets, steps, retire, g_seed, check):
    """`steps` batched decode steps over the sequences (prompt length, budget), sequence `retire[0]` leaving after step `retire[1]`.
    Streams are drawn per sequence from its own generator, so a run without a sequence sees the same tokens for the others.
    Returns {sequence: [victims per evicting step]}."""
    from easykv_amd import KVBankBatch, StepPlan
    from oracle import easykv_oracle as O
    Hq, H, D = 4, 4, 64
    B = len(prompts)
    bat = KVBankBatch(B, 1, Hq, H, D, cap=max(p + b for p, b in zip(prompts.values(), budgets.values())) + 8)
    names = list(prompts)
    gens = {s: torch.Generator().manual_seed(g_seed + 17 * s) for s in names}
    for i, s in enumerate(names):
        _fill(bat.bank, i, prompts[s], gens[s], budgets[s] + 1, warm=False)
    seqs = {s: bat.sequence(i) for i, s in enumerate(names)}
    victims = {s: [] for s in names}
    hook = Hook()
    n_dec = n_class = n_mixed = 0
    O.SELECT_HOOK = hook if check else None
    try:
        for step in range(steps):
            live = [i for i, s in enumerate(names) if not (retire and s == retire[0] and step > retire[1])]
            plans, oplans, toks = [], [], []
            for i in live:
                s = names[i]
                P, bud = prompts[s], budgets[s]
                evict = (bat.n_slots(i) + 1 - P) > bud      # as the decode loop decides: ITS length against ITS budget
                kw = dict(policy="roco", phase="decode", evict=evict, score_off=P, budget=bud)
                plans.append(StepPlan(**kw))
                oplans.append(O.StepPlan(**kw))
                toks.append([torch.randn(1, hh, 1, D, generator=gens[s]).half() for hh in (Hq, H, H)])
            n_mixed += len({p.evict for p in plans}) == 2
            states = [_oracle_state(seqs[names[i]], budgets[names[i]] + 1) for i in live] if check else None
            q, k, v = (torch.cat([t[j] for t in toks]).cuda() for j in range(3))
            out, ids = bat.attend(plans, q, k, v, 0, active=live)
            for row, i in enumerate(live):
                s = names[i]
                if plans[row].evict:
                    victims[s].append(ids[row, :, 0].cpu().clone())
                if check:
                    o_ref, ids_ref = O.layer_step(states[row], *(t.float() for t in toks[row]), oplans[row])
                    got = ids[row] - prompts[s] if plans[row].evict else None
                    nd, nc = _check_entry((step, s), hook, "roco", o_ref, ids_ref, out[row], got, seqs[s], states[row], budgets[s] + 1, plans[row].evict)
                    n_dec += nd
                    n_class += nc
    finally:
        O.SELECT_HOOK = None
    return victims, n_dec, n_class, n_mixed, bat


def test_ragged_lockstep_with_a_retirement():
    prompts = {0: 12, 1: 20, 2: 33, 3: 47, 4: 64}
    # the sequences start evicting at steps 30 / 70 / 36 / 90 / 50.  No budget below 30: roco's feasible set (budget - int(0.3 * budget)
    # entries of smallest std) then reaches into the 10 newest entries, whose std is the same 1e9 sentinel for all of them
    # (easykv/easykv.py:318-321) — which of those equal keys a top-k returns is the implementation's choice, in the oracle as in any
    # kernel, and no +-2e-5 perturbation of the scores moves it
    budgets = {0: 30, 1: 70, 2: 36, 3: 90, 4: 50}
    steps, retire = 96, (2, 47)
    victims, n_dec, n_class, n_mixed, bat = _run_lockstep(prompts, budgets, steps, retire, 5, check=True)
    assert n_mixed >= 55, n_mixed      # launches that mix evicting and non-evicting sequences
    assert n_dec == 4 * sum(len(v) for v in victims.values()) and n_dec > 4 * 120, n_dec
    assert len(victims[2]) == 48 - 36 and len(victims[0]) == steps - 30, {s: len(v) for s, v in victims.items()}
    assert bat.n_calls == steps
    print(f"[bound-fraction] ragged batched lockstep: {n_dec - n_class} exact + {n_class} in the tolerance class of {n_dec} decisions, {n_mixed} mixed launches")
    # the neighbours of the retired sequence: the same victims as in a run it never took part in
    solo = {s: p for s, p in prompts.items() if s != 2}
    twin, _, _, _, _ = _run_lockstep(solo, {s: budgets[s] for s in solo}, steps, None, 5, check=False)
    for s in solo:
        assert len(twin[s]) == len(victims[s]) and all(torch.equal(a, b) for a, b in zip(twin[s], victims[s])), s


def test_solo_steps_through_a_sequence_view_then_the_batch():
    """Sequence 0 is prefilled and decoded alone through its view — one-launch steps, which put its layers on the slot-indexed score
    rows — while sequence 1 waits; the batched call that follows finds those layers, brings them back to the ordered layout and
    decides as a twin bank that never left it."""
    from easykv_amd import KVBank, KVBankBatch, StepPlan
    L, Hq, H, D, rows = 2, 8, 8, 64, 300
    T = rows + 1
    g = torch.Generator().manual_seed(9)
    bat = KVBankBatch(2, L, Hq, H, D, cap=T + 8)
    twin = KVBank(2 * L, Hq, H, D, cap=T + 8)
    twin.use_slot_rows = False
    k0, v0 = (torch.randn(2 * L, H, rows, D, generator=g).half().cuda() for _ in range(2))
    for s in range(2):      # the prefill of each sequence, alone, through its own view
        seq = bat.sequence(s)
        seq.load_rows(k0[s * L:(s + 1) * L], v0[s * L:(s + 1) * L])
        seq.state_init(T, 0)
        assert seq.n_slots == (rows,) * L and bat.bank.n_slots[s * L:(s + 1) * L] == [rows] * L
    twin.load_rows(k0, v0)
    twin.state_init(T, 0)
    plan = StepPlan(policy="roco", phase="decode", evict=True, score_off=0, budget=rows, n_split=1)
    seq0 = bat.sequence(0)
    for step in range(3):      # sequence 0 alone: both of its layers per call, the one-launch step
        q, k, v = (torch.randn(L, hh, 1, D, generator=g).half().cuda() for hh in (Hq, H, H))
        o1, i1 = seq0.attend(plan, q, k, v)
        o2, i2 = twin.attend(plan, q, k, v, layer_begin=0)
        assert torch.equal(o1, o2) and torch.equal(i1, i2), step
    assert bat.bank._slot_rows == [True, True, False, False]      # the solo steps ran on the slot-indexed layout, behind no one's back
    try:      # the view is the sequence's bank and nothing more
        seq0.attend(plan, q, k, v, layer_begin=1)
    except ValueError:
        pass
    else:
        raise AssertionError("a view served layers outside its sequence")
    for step in range(3):
        for layer in range(L):
            q, k, v = (torch.randn(2, hh, 1, D, generator=g).half().cuda() for hh in (Hq, H, H))
            o1, i1 = bat.attend([plan, plan], q, k, v, layer, n_split=1)
            assert not bat.bank._slot_rows[layer] and not bat.bank._slot_rows[L + layer]
            for row, s in enumerate((0, 1)):
                o2, i2 = twin.attend(plan, q[row:row + 1], k[row:row + 1], v[row:row + 1], layer_begin=s * L + layer)
                assert torch.equal(o1[row], o2[0]) and torch.equal(i1[row], i2[0]), (step, layer, s)
    for arr in ("slot_of_pos", "score_cnt"):
        assert torch.equal(getattr(bat.bank, arr), getattr(twin, arr)), arr
    assert torch.allclose(bat.bank.score_sum, twin.score_sum, rtol=2e-5, atol=1e-9)


@pytest.mark.parametrize("policy", ["roco", "tova"])
def test_ragged_step_bf16_d96_gqa3_on_the_8_wave_build(policy):
    """The ragged edges on the other instantiation axes: bf16 rows, head_dim 96 (padded lanes), GQA 3 (padding heads), and 32 entries
    x 8 KV heads = 256 workgroup rows, which the planner gives the 8-wave one-launch build; lengths from 2 to 1301, every third entry
    not evicting, per-entry score offsets.  Outputs to the bf16 bar of tests/test_hip_bf16.py, decisions and score rows as above."""
    from easykv_amd import KVBankBatch, StepPlan
    from oracle import easykv_oracle as O
    from tests.test_hip_bf16 import _check_out, _pv
    Hq, H, D, B = 24, 8, 96, 32
    g = torch.Generator().manual_seed(77)
    bat = KVBankBatch(B, 1, Hq, H, D, cap=1301 + 40, dtype=torch.bfloat16)
    base = (1301, 2, 130, 700, 17, 333, 64, 1024)
    lens = [base[i % 8] + (i // 8) * 3 for i in range(B)]
    plans, oplans, widths, evicts = [], [], [], []
    for i, T in enumerate(lens):
        off = 0 if (T < 100 or i % 2) else 11 + i
        W = T - off
        ev = T >= 64 and i % 3 != 0
        _fill(bat.bank, i, T - 1, g, W)
        kw = dict(policy=policy, phase="decode", evict=ev, score_off=off, budget=W - 1)
        plans.append(StepPlan(**kw)), oplans.append(O.StepPlan(**kw)), widths.append(W), evicts.append(ev)
    info = bat.step_info(plans, 0)
    assert info["fused"] == 1 and info["n_launches"] == 1, info
    assert {True, False} <= set(evicts)
    seqs = [bat.sequence(i) for i in range(B)]
    states = [_oracle_state(seqs[i], widths[i]) for i in range(B)]
    q, k, v = (torch.randn(B, hh, 1, D, generator=g).to(torch.bfloat16) for hh in (Hq, H, H))
    out, ids = bat.attend(plans, q.cuda(), k.cuda(), v.cuda(), 0)
    hook = Hook()
    n_dec = n_class = 0
    O.SELECT_HOOK = hook
    try:
        for i, T in enumerate(lens):
            # p.|V| over the T rows the query attends (the bank's rows before the step + the appended one): the bf16 bar's scale
            pv = _pv(q[i].float(), torch.cat((states[i].k[0], k[i].float()), dim=1), torch.cat((states[i].v[0], v[i].float()), dim=1), T - 1)
            o_ref, ids_ref = O.layer_step(states[i], q[i:i + 1].float(), k[i:i + 1].float(), v[i:i + 1].float(), oplans[i])
            got = (ids[i] - plans[i].score_off) if evicts[i] else None
            nd, nc = _check_entry((policy, i, T), hook, policy, o_ref, ids_ref, out[i], got, seqs[i], states[i], widths[i], evicts[i],
                                  check_out=lambda o, r, pv=pv, i=i: _check_out(o, r, pv, (policy, i)))
            n_dec += nd
            n_class += nc
    finally:
        O.SELECT_HOOK = None
    assert n_dec == H * sum(evicts)
    print(f"[bound-fraction] ragged batched step bf16 d96 gqa3 8-wave {policy}: {n_dec - n_class} exact + {n_class} in the tolerance class of {n_dec}")
