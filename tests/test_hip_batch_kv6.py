"""Ragged decode batches on MXFP6 K/V rows (include/easykv_hip.h, "kv6 batches"; KVBankBatch.quantize_mxfp6) on the GPU.

  (a) a UNIFORM MXFP6 batch is the MXFP6 multi-layer step, bit for bit: outputs, evicted ids, slot maps, score rows, code planes and
      exponent planes, on the 8-wave and the 4-wave one-launch builds (GQA x 4 in bf16, the padded GQA x 3 build), the split path with
      its in-kernel fold, the range compaction and `full`;
  (b) a RAGGED MXFP6 batch — entries of 2 .. 2049 slots whose ends fall inside the kv6 stream's 16-row wave-loads, evicting and
      non-evicting entries mixed, per-entry score offsets — against the oracle ON THE BANK'S OWN dequantised contents
      (tests/test_hip_kv6.py): outputs under tests.golden_util.out_close, the appended row's codes and exponents under
      tests.kv6_ref.check_rows at the row the free list named, victims identical wherever tests.test_hip_fullsize.Probe calls the
      decision well defined (at most 10 % of a case's decisions may be ill defined; tests/test_batch_kv6_cpu.py verifies on the
      reference side that the seeded inputs allow it), lengths and extents as planned;
  (c) 32 consecutive ragged MXFP6 steps of four sequences, one retired half-way, checked as (b) every step; the survivors' victims equal
      those of a run the retired sequence never joined;
  (d) the engine: quantize_mxfp6 of a populated batch bank, adopt of quantised banks, an MXFP6-only batch bank, the refusals;
  (e) the seam: one decode forward through api.BudgetedKVCacheBatch over a kv6 batch is one batched MXFP6 attend per layer;
  (f) generate_batch(kv_quant='mxfp6') on the fake model: every sequence equals its solo generate(kv_quant='mxfp6') run."""
import contextlib
import io

import numpy as np
import pytest
import torch

from tests import batch_kv6_cases as cases
from tests import kv6_ref as R
from tests.golden_util import out_close
from tests.test_hip_fullsize import Probe

pytestmark = pytest.mark.gpu
BF, F16 = torch.bfloat16, torch.float16
PLANES = ("k6", "v6", "k_exp", "v_exp")


# ---- (a) uniform --------------------------------------------------------------------------------------------------------------------
UNIFORM = [
    # id, Hq, H, B, rows, policy, dtype, n_split, one launch?   (head_dim 128 throughout)
    ("fused8_roco", 32, 32, 8, 300, "roco", F16, 0, True),                  # B * H = 256: the 8-wave one-launch build
    ("fused4_gqa4_tova_bf16", 8, 2, 4, 700, "tova", BF, 1, True),           # explicit n_split = 1: the 4-wave build, GQA x 4
    ("fused4_gqa3_h2o", 6, 2, 3, 200, "h2o_head", F16, 1, True),            # the padded GQA x 3 build
    ("split_h2o_fold", 4, 4, 3, 700, "h2o_head", F16, 4, False),            # split path, in-kernel fold, fast scorer
    ("recency", 4, 4, 2, 500, "recency", F16, 0, False),                    # range compaction
    ("full", 4, 4, 3, 400, "full", F16, 2, False),                          # nothing scored
]


@pytest.mark.parametrize("name,Hq,H,B,rows,policy,dtype,n_split,one_launch", UNIFORM, ids=[c[0] for c in UNIFORM])
def test_uniform_mxfp6_batch_is_the_mxfp6_multi_layer_step_bit_for_bit(name, Hq, H, B, rows, policy, dtype, n_split, one_launch):
    from easykv_amd import KVBank, KVBankBatch, StepPlan
    from tests.test_hip_batch import _copy_layer, _fill
    D = 128
    g = torch.Generator().manual_seed(4000 + rows + B)
    T = rows + 1
    ref = KVBank(B, Hq, H, D, cap=T + 6, dtype=dtype)
    ref.use_slot_rows = False      # like against like: a batch runs the ordered score-row layout
    ref.k.zero_(), ref.v.zero_()   # (whole planes are compared below: no uninitialised rows)
    for l in range(B):
        _fill(ref, l, rows, g, T)
    LPS, layer = 3, 1      # [sequence][layer]; the call serves model layer 1 of every sequence, in permuted, non-contiguous order
    bat = KVBankBatch(B, LPS, Hq, H, D, cap=T + 6, dtype=dtype)
    bat.bank.k.zero_(), bat.bank.v.zero_()
    order = [(5 * i + 2) % B for i in range(B)] if B % 5 else list(reversed(range(B)))
    assert sorted(order) == list(range(B))
    for i, s in enumerate(order):
        _copy_layer(ref, i, bat.bank, s * LPS + layer)
    ref.quantize_mxfp6()
    assert bat.quantize_mxfp6() is bat and bat.kv_quant == "mxfp6"
    budget = rows - 3
    plan = StepPlan(policy=policy, phase="decode", evict=policy != "full", score_off=0, budget=budget, n_split=n_split,
                    range_start=7 if policy == "recency" else -1)
    info = bat.step_info([plan] * B, layer, order, n_split)
    assert info == ref.step_info(plan, 1, 0, B), (info, ref.step_info(plan, 1, 0, B))
    assert bool(info["fused"]) == one_launch and info["n_launches"] >= 1 and info["fused_order"] == 0, info
    if n_split > 1:      # (the planner rounds a split's key range up, so fewer than the asked-for splits may remain: 700 rows / 4 -> 3)
        assert info["n_split"] > 1, info
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
            for arr in ("slot_of_pos", "score_sum", "score_sq", "score_cnt") + PLANES:
                assert torch.equal(getattr(bat.bank, arr)[lb], getattr(ref, arr)[i]), (name, step, i, arr)
        assert int(bat.bank.arrive.abs().sum()) == 0      # the arrival counters of the in-kernel fold are left at zero
    # the other layers of the [sequence][layer] bank were never touched: no rows, zero codes, exponent bytes as allocated
    for s in range(B):
        for l in (0, 2):
            lb = s * LPS + l
            assert bat.bank.n_slots[lb] == 0
            assert not bool(bat.bank.k6[lb].any()) and not bool(bat.bank.v6[lb].any())
            assert bool((bat.bank.k_exp[lb] == 127).all()) and bool((bat.bank.v_exp[lb] == 127).all())


# ---- (b), (c): one batched MXFP6 step against the oracle on the bank's own contents --------------------------------------------------
def _oracle_states(bank, wanted):
    """{layer: LayerState} of the layers in `wanted` ({layer: score-row width}) from the bank as it stands: dequantised rows gathered
    through the slot map into position order (ordered_kv is refused on quantised banks) + the ordered score rows."""
    from oracle import easykv_oracle as O
    slot = bank.slot_of_pos.cpu().long()
    S, Q, Cn = bank.score_sum.cpu(), bank.score_sq.cpu(), bank.score_cnt.cpu()
    out = {}
    for l, W in wanted.items():
        kd, vd = (x.cpu() for x in bank.dequantized_rows(l))
        t = bank.n_slots[l]
        idx = slot[l, :, :t].unsqueeze(-1).expand(-1, -1, kd.shape[-1])
        st = O.LayerState(k=torch.gather(kd, 1, idx).unsqueeze(0), v=torch.gather(vd, 1, idx).unsqueeze(0))
        st.s, st.q, st.c = S[l, :, :W].clone(), Q[l, :, :W].clone(), Cn[l, :, :W].clone()
        out[l] = st
    return out


class _Check:
    """Runs batched MXFP6 steps and holds every entry to the checks of case (b).  The oracle's state of an entry is carried from step
    to step and re-seeded from the bank when asked (`fresh`) or after an ill-defined decision that went the other way."""

    def __init__(self, bat):
        self.bat, self.bank = bat, bat.bank
        self.states = {}
        self.probe = Probe()
        self.n_dec = self.n_stable = self.n_reseed = 0
        self.worst = 0.0

    def step(self, tag, layers, plans, oplans, widths, q, k, v, n_split=0, fresh=()):
        """layers[row]: the bank layer (LPS = 1: the sequence) of table row `row`; q / k / v: CPU tensors of the table."""
        from oracle import easykv_oracle as O
        bat, bank = self.bat, self.bank
        H, D = bank.n_kv_heads, bank.head_dim
        rows = torch.arange(H)
        need = {l: widths[r] for r, l in enumerate(layers) if l not in self.states or l in fresh}
        self.states.update(_oracle_states(bank, need))
        before = [(bank.n_slots[l], bank.extent[l]) for l in layers]
        # the row each entry appends to: the front of its free list
        new_row = torch.stack([bank._slot_of_pos[l, :, bank.n_slots[l]] for l in layers]).cpu().long()
        out, ids = bat.attend(plans, q.cuda(), k.cuda(), v.cuda(), 0, active=layers, n_split=n_split)
        torch.cuda.synchronize()
        assert out.dtype == bank.dtype and int(bank.arrive.abs().sum()) == 0
        O.SELECT_HOOK = self.probe
        try:
            for r, l in enumerate(layers):
                plan = plans[r]
                # the appended row: quantised by the kernel as the rule says, at the row the free list named
                for given, codes, ex in ((k[r, :, 0], bank.k6[l], bank.k_exp[l]), (v[r, :, 0], bank.v6[l], bank.v_exp[l])):
                    R.check_rows(given, codes[rows, new_row[r]], ex[rows, new_row[r]], (tag, l))
                kd, vd = bank.dequantized_rows(l)
                kq, vq = kd[rows, new_row[r]].cpu().view(1, H, 1, D), vd[rows, new_row[r]].cpu().view(1, H, 1, D)
                o_ref, ids_ref = O.layer_step(self.states[l], q[r:r + 1].float(), kq, vq, oplans[r])
                err = float((out[r].float().cpu() - o_ref[0]).abs().max())
                self.worst = max(self.worst, err)
                assert out_close(out[r].float().cpu(), o_ref[0]), (tag, l, err)
                T, ext = before[r][0] + 1, before[r][1]
                if plan.evict:
                    unstable = self.probe.last_unstable
                    got = ids[r, :, 0].cpu().long() - plan.score_off      # (the library reports cache positions)
                    same = got == ids_ref[:, 0]
                    self.n_dec += H
                    self.n_stable += int((~unstable).sum())
                    assert bool(same[~unstable].all()), (tag, l, got.tolist(), ids_ref[:, 0].tolist())      # well defined: identical
                    if not bool(same.all()):      # an ill-defined decision went the other way: the oracle follows the bank from here
                        self.states.pop(l)
                        self.n_reseed += 1
                # lengths and extents advance as the plan says
                assert bank.n_slots[l] == (T - 1 if plan.evict else T) and bank.extent[l] == max(ext, T), (tag, l, bank.n_slots[l], bank.extent[l])
                assert int(new_row[r].max()) < bank.extent[l]
        finally:
            O.SELECT_HOOK = None
        return out, ids


@pytest.mark.parametrize("policy", cases.POLICIES)
@pytest.mark.parametrize("n_split", [1, 8], ids=["one_launch", "split"])
@pytest.mark.parametrize("draw", [0, 1], ids=["short_first", "short_last"])
@pytest.mark.parametrize("shape", list(cases.SHAPES))
def test_ragged_mxfp6_step_against_the_oracle(shape, draw, n_split, policy):
    from easykv_amd import KVBankBatch, StepPlan
    from oracle import easykv_oracle as O
    D, Hq, H, dtype = cases.SHAPES[shape]
    entries, tokens = cases.inputs(shape, draw)
    B = len(entries)
    bat = KVBankBatch(B, 1, Hq, H, D, cap=2049 + 40, dtype=dtype)
    for i, e in enumerate(entries):
        cases.fill_entry(bat.bank, i, e)
    bat.quantize_mxfp6()
    widths = [e["W"] for e in entries]
    plans = [StepPlan(**cases.plan_kw(e, policy)) for e in entries]
    oplans = [O.StepPlan(**cases.plan_kw(e, policy)) for e in entries]
    info = bat.step_info(plans, 0, None, n_split)
    assert bool(info["fused"]) == (n_split == 1) and (n_split == 1 or info["n_split"] >= 4), info      # (split: ranges past the short entries are empty)
    assert {p.evict for p in plans} == {True, False} and any(p.score_off for p in plans)
    chk = _Check(bat)
    layers = list(range(B))
    for step, (q, k, v) in enumerate(tokens):
        # entries that keep everything grow: their score rows are read at the new width (as a decode loop's plan would say)
        grown = [i for i, e in enumerate(entries) if not e["evict"]]
        chk.step((shape, draw, n_split, policy, step), layers, plans, oplans, widths, q, k, v, n_split=n_split, fresh=grown if step else ())
        for i in grown:
            widths[i] += 1
            plans[i], oplans[i] = StepPlan(**cases.plan_kw(entries[i], policy, widths[i])), O.StepPlan(**cases.plan_kw(entries[i], policy, widths[i]))
        for i, e in enumerate(entries):
            assert bat.n_slots(i) == (e["T"] - 1 if e["evict"] else e["T"] + step), (e["T"], step, bat.n_slots(i))
    assert chk.n_dec == cases.STEPS * H * sum(e["evict"] for e in entries)
    print(f"[kv6-batch] ragged {shape} draw {draw} n_split {n_split} {policy}: {chk.n_stable} of {chk.n_dec} decisions well defined, "
          f"{chk.n_reseed} re-seeds, largest |out - oracle| {chk.worst:.3g}")
    assert chk.n_stable >= 0.9 * chk.n_dec, (chk.n_stable, chk.n_dec)      # the cap: at most 10 % ill defined


def _run_lockstep(names, retire, check):
    """cases.LOCK_STEPS batched MXFP6 decode steps over the sequences `names` of cases.LOCK, sequence retire[0] leaving after step
    retire[1].  Returns ({sequence: [victims per evicting step]}, the checker, mixed launches, the batch)."""
    from easykv_amd import KVBankBatch, StepPlan
    from oracle import easykv_oracle as O
    Hq, H, D = cases.LOCK_SHAPE
    P, Bud = cases.LOCK["prompts"], cases.LOCK["budgets"]
    bat = KVBankBatch(len(names), 1, Hq, H, D, cap=max(P[s] + Bud[s] for s in names) + 8)
    toks = {}
    for i, s in enumerate(names):
        entry, toks[s] = cases.lockstep_inputs(s)
        cases.fill_entry(bat.bank, i, entry)
    bat.quantize_mxfp6()
    victims = {s: [] for s in names}
    chk = _Check(bat)
    n_mixed = 0
    for step in range(cases.LOCK_STEPS):
        live = [i for i, s in enumerate(names) if not (retire and s == retire[0] and step > retire[1])]
        plans, oplans, widths = [], [], []
        for i in live:
            s = names[i]
            evict = (bat.n_slots(i) + 1 - P[s]) > Bud[s]      # as the decode loop decides: ITS length against ITS budget
            assert evict == cases.lockstep_evicts(s, step)
            kw = dict(policy="roco", phase="decode", evict=evict, score_off=P[s], budget=Bud[s])
            plans.append(StepPlan(**kw)), oplans.append(O.StepPlan(**kw)), widths.append(Bud[s] + 1)
        n_mixed += len({p.evict for p in plans}) == 2
        q, k, v = (torch.cat([toks[names[i]][step][j] for i in live]) for j in range(3))
        if check:
            _, ids = chk.step(("lockstep", step), live, plans, oplans, widths, q, k, v)
        else:
            _, ids = bat.attend(plans, q.cuda(), k.cuda(), v.cuda(), 0, active=live)
        for row, i in enumerate(live):
            if plans[row].evict:
                victims[names[i]].append(ids[row, :, 0].cpu().clone())
    return victims, chk, n_mixed, bat


def test_ragged_mxfp6_lockstep_with_a_retirement():
    steps, retire = cases.LOCK_STEPS, cases.LOCK_RETIRE
    victims, chk, n_mixed, bat = _run_lockstep([0, 1, 2, 3], retire, check=True)
    # sequences 0 .. 3 start evicting at steps 10 / 6 / 4 / 30; sequence 2 leaves after step 15
    assert [len(victims[s]) for s in range(4)] == [steps - 10, steps - 6, 16 - 4, steps - 30], {s: len(v) for s, v in victims.items()}
    assert n_mixed >= 20 and bat.n_calls == steps, (n_mixed, bat.n_calls)
    assert chk.n_dec == 4 * sum(len(v) for v in victims.values())
    print(f"[kv6-batch] lockstep: {chk.n_stable} of {chk.n_dec} decisions well defined, {chk.n_reseed} re-seeds, {n_mixed} mixed launches, "
          f"largest |out - oracle| {chk.worst:.3g}")
    assert chk.n_stable >= 0.9 * chk.n_dec, (chk.n_stable, chk.n_dec)
    # the neighbours of the retired sequence: the same victims as in a run it never took part in
    twin, _, _, _ = _run_lockstep([0, 1, 3], None, check=False)
    for s in (0, 1, 3):
        assert len(twin[s]) == len(victims[s]) and all(torch.equal(a, b) for a, b in zip(twin[s], victims[s])), s


# ---- (d) engine --------------------------------------------------------------------------------------------------------------------
def _solo_bank(L, Hq, H, D, rows, cap, g, dtype=F16):
    from easykv_amd import KVBank
    from tests.test_hip_batch import _fill
    b = KVBank(L, Hq, H, D, cap=cap, dtype=dtype)
    b.k.zero_(), b.v.zero_()
    for l in range(L):
        _fill(b, l, rows, g, rows + 1)
    return b


def test_quantize_mxfp6_of_a_populated_ragged_batch_bank():
    from easykv_amd import KVBankBatch, StepPlan
    from easykv_amd._lib import EkvError
    from tests.test_hip_batch import _fill
    Hq, H, D, lens = 4, 2, 128, (5, 130, 64)
    g = torch.Generator().manual_seed(4)
    bat = KVBankBatch(len(lens), 2, Hq, H, D, cap=200)
    bat.bank.k.zero_(), bat.bank.v.zero_()
    for s, n in enumerate(lens):
        for l in range(2):
            _fill(bat.bank, s * 2 + l, n, g, n + 1)
    maps, k16, v16 = bat.bank.slot_of_pos.clone(), bat.bank.k.clone(), bat.bank.v.clone()
    sums = bat.bank.score_sum.clone()
    rows = bat.bank.n_layers * H * bat.cap
    assert bat.kv_quant is None and bat.kv_bytes() == rows * 4 * D
    assert bat.quantize_mxfp6() is bat
    assert bat.kv_quant == "mxfp6" and bat.bank.k is None and bat.bank.v is None      # the 16-bit tensors are released
    assert bat.kv_bytes() == rows * (3 * D // 2 + D // 16) == rows * 200
    assert torch.equal(bat.bank.slot_of_pos, maps) and torch.equal(bat.bank.score_sum, sums)
    assert [bat.n_slots(s, l) for s in range(3) for l in range(2)] == [n for n in lens for _ in range(2)]
    assert bat.bank.extent == [n for n in lens for _ in range(2)]
    ext = max(lens)
    for x, codes, ex in ((k16, bat.bank.k6, bat.bank.k_exp), (v16, bat.bank.v6, bat.bank.v_exp)):
        R.check_rows(x[:, :, :ext], codes[:, :, :ext], ex[:, :, :ext], "batch bank")
        assert not bool(codes[:, :, ext:].any()) and bool((ex[:, :, ext:] == 127).all())      # rows >= the largest extent: as allocated
    # a sequence of a quantised batch is a quantised bank: decode steps only
    seq = bat.sequence(1)
    with pytest.raises(EkvError, match="row move"):
        seq.ordered_kv()
    with pytest.raises(EkvError, match="load_rows"):
        seq.load_rows(k16[:2, :, :4], v16[:2, :, :4])
    q, k, v = (torch.randn(2, hh, 8, D, generator=g).half().cuda() for hh in (Hq, H, H))
    with pytest.raises(EkvError, match="chunk step"):
        seq.attend(StepPlan(policy="full", phase="prefill", accumulate=False), q, k, v)
    with pytest.raises(EkvError, match="quantised already"):
        bat.quantize_mxfp6()
    with pytest.raises(EkvError, match="MXFP6 already"):
        bat.quantize_fp8()


def test_adopt_of_quantised_banks_and_an_mxfp6_only_batch(monkeypatch):
    from easykv_amd import KVBankBatch, StepPlan, engine
    from easykv_amd._lib import EkvError
    monkeypatch.setattr(engine.KVBank, "use_slot_rows", False)
    L, Hq, H, D, rows = 2, 4, 4, 128, 90
    g = torch.Generator().manual_seed(6)
    # a batch created MXFP6-only never holds a 16-bit K/V tensor: not as an attribute, and not in the allocator's peak
    n_seq, cap = 4, 1024
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    bat = KVBankBatch(n_seq, L, Hq, H, D, cap=cap, kv_quant="mxfp6")
    assert bat.bank.k is None and bat.bank.v is None and bat.kv_quant == "mxfp6"
    n_rows = n_seq * L * H * bat.cap
    assert bat.kv_bytes() == n_rows * 200
    peak = torch.cuda.max_memory_allocated() - base
    assert peak < n_rows * 4 * D, (peak, n_rows * 4 * D)      # (planes 200 B + slot map, score rows and births 24 B per row: 0.44 x the 16-bit rows alone)
    assert not bool(bat.bank.k6.any()) and not bool(bat.bank.v6.any()) and bool((bat.bank.k_exp == 127).all()) and bool((bat.bank.v_exp == 127).all())
    solo = [_solo_bank(L, Hq, H, D, rows + 7 * i, 200, g) for i in range(2)]
    fp8 = _solo_bank(L, Hq, H, D, rows, 200, g).quantize_fp8()
    with pytest.raises(ValueError, match="kv_quant"):      # 16-bit rows into an MXFP6 batch
        bat.adopt(0, solo[0])
    with pytest.raises(ValueError, match="kv_quant"):      # FP8 rows into an MXFP6 batch
        bat.adopt(0, fp8)
    for b in solo:
        b.quantize_mxfp6()
    with pytest.raises(ValueError, match="kv_quant"):      # MXFP6 rows into a 16-bit batch
        KVBankBatch(2, L, Hq, H, D, cap=256).adopt(0, solo[0])
    with pytest.raises(ValueError, match="kv_quant"):      # MXFP6 rows into an FP8 batch
        KVBankBatch(2, L, Hq, H, D, cap=256, kv_quant="fp8").adopt(0, solo[0])
    for i, b in ((2, solo[0]), (0, solo[1])):
        bat.adopt(i, b)
        l0, c = i * L, b.cap
        for arr in PLANES + ("slot_of_pos", "score_sum", "score_sq", "score_cnt"):      # the same physical rows
            assert torch.equal(getattr(bat.bank, arr)[l0:l0 + L, :, :c], getattr(b, arr)), (i, arr)
        assert bat.bank.n_slots[l0:l0 + L] == b.n_slots and bat.bank.extent[l0:l0 + L] == b.extent
    assert bat.bank.k is None and bat.bank.v is None
    # sequence(i) keeps the single-sequence kv6 behaviour: an immediate decode step is the solo bank's, bit for bit
    plan = StepPlan(policy="roco", phase="decode", evict=True, score_off=0, budget=rows, n_split=1)
    q, k, v = (torch.randn(L, hh, 1, D, generator=g).half().cuda() for hh in (Hq, H, H))
    o1, i1 = bat.sequence(2).attend(plan, q, k, v)
    o2, i2 = solo[0].attend(plan, q, k, v)
    assert torch.equal(o1, o2) and torch.equal(i1, i2)
    seq = bat.sequence(2)
    with pytest.raises(EkvError, match="row move"):
        seq.ordered_kv()
    with pytest.raises(EkvError, match="load_rows"):
        seq.load_rows(k, v)
    with pytest.raises(EkvError, match="chunk step"):
        seq.attend(StepPlan(policy="full", phase="prefill", accumulate=False), q.expand(-1, -1, 8, -1).contiguous(), k.expand(-1, -1, 8, -1).contiguous(),
                   v.expand(-1, -1, 8, -1).contiguous())
    # ... and the batched call serves the adopted sequences from the MXFP6 planes: each row is its sequence's own solo step
    plans = [StepPlan(policy="roco", phase="decode", evict=True, score_off=0, budget=bat.n_slots(s), n_split=1) for s in (0, 2)]
    q, k, v = (torch.randn(2, hh, 1, D, generator=g).half().cuda() for hh in (Hq, H, H))
    ob, ib = bat.attend(plans, q, k, v, 1, active=[0, 2], n_split=1)
    for row, (s, b) in enumerate(((0, solo[1]), (2, solo[0]))):
        if s == 2:      # (layer 1 of solo[0] took the step above; solo[1] did not)
            continue
        o2, i2 = b.attend(plans[row], q[row:row + 1], k[row:row + 1], v[row:row + 1], layer_begin=1)
        assert torch.equal(ob[row], o2[0]) and torch.equal(ib[row], i2[0])
    # what KVBank(kv_quant='mxfp6') refuses: the shapes quantize_mxfp6() refuses, with its errors
    with pytest.raises(EkvError, match="head_dim 128"):
        KVBankBatch(2, L, Hq, H, 64, cap=256, kv_quant="mxfp6")
    with pytest.raises(EkvError, match="GQA factors up to 4"):
        KVBankBatch(2, L, 16, 2, D, cap=256, kv_quant="mxfp6")


# ---- (e) the seam -----------------------------------------------------------------------------------------------------------------
def test_seam_one_batched_mxfp6_attend_per_layer(monkeypatch):
    """One decode forward of the batched fake model through api.BudgetedKVCacheBatch over a kv6 batch: exactly one batched attend per
    layer, each on MXFP6 rows, and every sequence one row longer afterwards."""
    from easykv_amd import KVBankBatch, StepPlan, api, engine
    from oracle.fake_model import make_streams
    from tests.batch_fake_model import BatchFakeModel
    from tests.test_hip_batch import _fill
    L, Hq, H, D, lens = 2, 4, 2, 128, (40, 17, 65)
    model = BatchFakeModel(*make_streams(L, Hq, H, D, 128, seed=5))
    model.logs = [[] for _ in lens]      # (generate_batch's prefills open these; here the sequences are filled directly)
    g = torch.Generator().manual_seed(8)
    bat = KVBankBatch(len(lens), L, Hq, H, D, cap=128)
    for s, n in enumerate(lens):
        for l in range(L):
            _fill(bat.bank, s * L + l, n, g, n + 1)
    bat.quantize_mxfp6()
    calls = []
    orig = engine.KVBankBatch.attend
    monkeypatch.setattr(engine.KVBankBatch, "attend", lambda self, *a, **k: (calls.append((a[4], self.kv_quant)), orig(self, *a, **k))[1])
    cache = api.BudgetedKVCacheBatch(bat)
    evicts = (True, False, False)      # a mixed launch: sequence 0 is at its budget, the others still grow
    plans = [StepPlan(policy="roco", phase="decode", evict=ev, score_off=0, budget=n) for n, ev in zip(lens, evicts)]
    live = [0, 1, 2]
    ids = torch.tensor([[3], [5], [7]], device="cuda")
    positions = torch.tensor([[n] for n in lens], device="cuda")
    with cache.active(plans, live, positions):
        model(input_ids=ids, past_key_values=cache, position_ids=positions)
    torch.cuda.synchronize()
    assert calls == [(l, "mxfp6") for l in range(L)] and cache.n_attend == L and bat.n_calls == L
    assert [bat.n_slots(s, l) for s in range(3) for l in range(L)] == [n + (not ev) for n, ev in zip(lens, evicts) for _ in range(L)]
    assert bat.bank.k is None and bat.bank.v is None
    assert all(len(model.logs[s]) == 1 and bool(torch.isfinite(model.logs[s][0]).all()) for s in live)


# ---- (f) generate_batch(kv_quant='mxfp6') ---------------------------------------------------------------------------------------------
def _evictions(ev):
    return [np.sort(torch.stack(list(e)).cpu().numpy(), axis=-1) for e in ev]


def _ids(length):
    return torch.arange(length).view(1, -1) % 16


def test_generate_batch_mxfp6_equals_the_solo_mxfp6_runs(monkeypatch):
    """The twin of tests/test_hip_batch_kv8.py's FP8 case at head_dim 128: five prompts of different lengths through generate_batch on
    MXFP6 rows (each bank quantised after its own prefill, adopted into an MXFP6-only batch bank, one batched MXFP6 step per layer and
    token), each against its solo generate(kv_quant='mxfp6') on deterministic logits: budget line, text, evicted ids, final length and
    the attention outputs of every forward."""
    import easykv_amd
    from easykv_amd import engine
    from oracle.fake_model import make_streams
    from tests.batch_fake_model import BatchFakeModel
    from tests.native_fake_model import NativeFakeModel
    streams = make_streams(2, 4, 2, 128, 400, seed=11)      # head_dim 128, GQA x 2
    cfg = dict(budget=40, kv_policy="roco", max_new_tokens=60, kv_quant="mxfp6", _record_evictions=True)
    lengths = (16, 33, 48, 64, 97)

    def solo(n):
        model = NativeFakeModel(*streams)
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            res, cache = easykv_amd.generate(model, _ids(n), cfg, kv_mode="decoding", stride=1, return_cache=True)
        return model, res, cache, buf.getvalue().strip()

    model = BatchFakeModel(*streams)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        res, cache = easykv_amd.generate_batch(model, [_ids(n) for n in lengths], cfg, kv_mode="decoding", stride=1, return_cache=True)
    lines = buf.getvalue().strip().split("\n")
    bat = cache.bat
    assert bat.kv_quant == "mxfp6" and bat.bank.k is None and bat.bank.v is None and len(res) == len(lines) == len(lengths)
    assert bat.kv_bytes() == bat.bank.n_layers * bat.n_kv_heads * bat.cap * 200
    assert model.n_batched_forwards == cfg["max_new_tokens"] and bat.n_calls == model.n_batched_forwards * 2
    for i, n in enumerate(lengths):
        smodel, sres, scache, sline = solo(n)
        assert scache.kv_quant == "mxfp6"
        solo_ev = _evictions(scache.evictions)
        # the precondition: the solo run again on the ordered score-row layout (another summation order) decides the same, so a
        # differing id below is never a near-tie
        monkeypatch.setattr(engine.KVBank, "use_slot_rows", False)
        _, sres2, scache2, sline2 = solo(n)
        monkeypatch.undo()
        ev2 = _evictions(scache2.evictions)
        assert sres2 == sres and sline2 == sline and len(ev2) == len(solo_ev) and all(np.array_equal(a, b) for a, b in zip(ev2, solo_ev)), (i, n, "precondition")
        assert res[i] == sres and lines[i] == sline, (i, n, res[i], sres, lines[i], sline)
        ours = _evictions(cache.evictions[i])
        assert len(ours) == len(solo_ev) > 0 and all(np.array_equal(a, b) for a, b in zip(ours, solo_ev)), (i, n, len(ours), len(solo_ev))
        assert bat.n_slots(i) == scache.get_seq_length(), (i, bat.n_slots(i), scache.get_seq_length())
        assert len(model.logs[i]) == len(smodel.outputs_log)
        for f, (a, b) in enumerate(zip(model.logs[i], smodel.outputs_log)):
            assert a.shape == b.shape and out_close(a, b, 1e-3), (i, f, float((a - b).abs().max()))


def test_generate_batch_mxfp6_refusals():
    """What generate_batch refuses with kv_quant='mxfp6', before any bank exists: the refusals of the other formats."""
    import easykv_amd
    from oracle.fake_model import make_streams
    from tests.batch_fake_model import BatchFakeModel
    ids = [_ids(16), _ids(20)]
    gen = dict(budget=8, kv_policy="roco", max_new_tokens=4, kv_quant="mxfp6")
    model = BatchFakeModel(*make_streams(2, 4, 2, 128, 64, seed=1))
    for extra, mode, match in ((dict(streaming=True), "decoding", "streaming"), ({}, "ppl", "ppl"), (dict(hipgraph=True), "decoding", "hipgraph")):
        with pytest.raises(ValueError, match=match):
            easykv_amd.generate_batch(model, ids, dict(gen, **extra), kv_mode=mode)
    with pytest.raises(ValueError, match="needs head_dim 128"):
        easykv_amd.generate_batch(BatchFakeModel(*make_streams(2, 4, 2, 64, 64, seed=1)), ids, gen, kv_mode="decoding")
    with pytest.raises(ValueError, match="GQA factor of at most 4"):
        easykv_amd.generate_batch(BatchFakeModel(*make_streams(2, 16, 2, 128, 64, seed=1)), ids, gen, kv_mode="decoding")
    with pytest.raises(ValueError, match="mxfp4"):      # (the batch driver's own MXFP4 refusal stays)
        easykv_amd.generate_batch(model, ids, dict(gen, kv_quant="mxfp4"), kv_mode="decoding")
