"""The geometry edges of the chunk step on FP8 rows (ekv_attn_chunk8.inc; the ekv_kv8_chunk_* calls): one table of named cases, the
seeded inputs of a case, and a CPU restatement of it.  tests/test_kv8_chunk_edges_cpu.py holds every case to what it claims to reach —
from the planner's dry run and the kernel's own rules, restated below — and tests/test_hip_kv8_chunk_edges.py runs the cases on the GPU.

Both draw the same rows, slot maps, score state and tokens from `draw`.  A bank is built as `_bank` of tests/test_hip_kv8_chunk.py
builds it (T0 + 3 rows loaded, three positions compacted out, an outlier K row, an outlier V row and an all-zero row among the cache
rows, an all-zero row among the new ones, a warm score state) and then, once quantised, has its physical rows permuted per head
(`scatter_rows`): ekv_compact_inplace moves rows and leaves the slot map the identity, under which a kernel that took a position for a
physical row would go unnoticed.  bf16 cases draw V at 1/4 scale, clamped to |v| <= 0.24, as that module's docstring explains.

`restate` rebuilds a case's bank on the CPU by the quantisation rule (tests/kv8_ref.py) and runs the float64 oracle step on it: which
heads the stability probe accepts and which heads roco's feasible set leaves uncut is what decides whether the GPU test can compare
victims exactly.  Seeds are picked with it (tests/test_kv8_chunk_edges_cpu.py), on the CPU, until every evicting case has such a head."""
from collections import namedtuple

import torch

from tests import kv8_ref as R

BF, F16 = torch.bfloat16, torch.float16
POLICY_CODES = dict(full=0, h2o_head=1, roco=2, tova=3)
SINK = 4
KT = 64      # positions per super-tile of the kernel, and the unit of rows_per_split
WS_BYTES = 8 << 20      # more than any case's step asks for (the largest, three deferred layers of empty-pairs, stays below 2 MiB)

# n_split: the forced split count (0: the planner's choice, which is 1 at these sizes); expect: (n_split, n_qblocks, qb_rows) of the plan;
# reaches: the edges (see `edges`) the case is in the table for
Case = namedtuple("Case", "name D rep H L dtype T0 n n_split policy seed expect reaches layer_begin")


def _c(name, D, rep, T0, n, n_split, policy, seed, expect, reaches, H=2, L=1, dtype=F16, layer_begin=0):
    return Case(name, D, rep, H, L, dtype, T0, n, n_split, policy, seed, expect, tuple(reaches.split()), layer_begin)


CASES = [
    # new rows 120..135 lie on both sides of rows_per_split = 128
    _c("straddle", 128, 1, 120, 16, 2, "roco", 1, (2, 1, 16), "straddle idle_wave"),
    # rows_per_split = 64 inside the chunk 60..67, 32 folded rows
    _c("straddle-d64-gqa", 64, 4, 60, 8, 2, "h2o_head", 2, (2, 1, 8), "straddle"),
    # blocks of 32, 32, 32, 4 queries; block 0's causal bound 52 < 64: (split 1, block 0) is empty; the last block leaves wave 1 idle
    _c("empty-pairs", 64, 1, 20, 100, 2, "roco", 3, (2, 4, 32), "straddle empty_pair short_block idle_wave"),
    # a bank created quantised: every row is the launch's own; 10 blocks of 16 queries (the last of 6), blocks 0..7 end at or below 128
    _c("dense-prefix", 128, 2, 0, 150, 2, "full", 4, (2, 10, 16), "straddle empty_pair short_block idle_wave"),
    # GQA factors that do not divide 32: two full blocks of 30 / 30 / 28 rows and a one-query block
    _c("rep3", 128, 3, 70, 21, 0, "h2o_head", 5, (1, 3, 10), "ragged_rows short_block idle_wave"),
    _c("rep5", 64, 5, 70, 13, 0, "roco", 6, (1, 3, 6), "ragged_rows short_block idle_wave"),
    _c("rep7", 128, 7, 70, 9, 0, "h2o_head", 7, (1, 3, 4), "ragged_rows short_block idle_wave"),
    # one query per block / two queries per block
    # (rep32 with h2o_head: at T0 = 40 roco's k1 = 32 exceeds the 29 columns outside its sink and tail sentinels, so its feasible set always
    #  cuts the tied sentinel class and no head could be compared exactly)
    _c("rep32", 64, 32, 40, 3, 0, "h2o_head", 8, (1, 3, 1), "one_query_blocks", H=1),
    # (seed 101: under seeds 9 and 100 the probe calls the one head's roco decision unstable; picked on the CPU restatement)
    _c("rep16", 128, 16, 62, 5, 0, "roco", 101, (1, 3, 2), "short_block idle_wave crosses_tile", H=1),
    # odd-n: a second block of one query; a chunk that starts exactly on a tile boundary
    _c("odd-n-33", 64, 1, 31, 33, 0, "roco", 10, (1, 2, 32), "short_block idle_wave one_query_blocks"),
    _c("odd-n-3", 64, 1, 64, 3, 0, "h2o_head", 11, (1, 1, 3), "starts_on_tile idle_wave fused_tail"),
    # layers 1 and 2 of 3 step, layer 0 does not; split, so that the partials are indexed by the launch's layer too
    _c("layers", 128, 2, 70, 8, 2, "roco", 12, (2, 1, 8), "layer_offset", L=3, layer_begin=1),
]
# unsplit one-block steps (the fused scorer tail) whose range ends on or next to a 32- or 64-position boundary
CASES += [_c(f"boundaries-{T}", 128, 1, T - 8, 8, 0, ("roco", "h2o_head")[i % 2], 20 + i, (1, 1, 8), "ends_near_32 fused_tail idle_wave")
          for i, T in enumerate((95, 96, 97, 127, 128, 129))]
CASES += [_c("straddle-bf16", 128, 1, 120, 16, 2, "roco", 31, (2, 1, 16), "straddle idle_wave", dtype=BF),
          _c("empty-pairs-bf16", 64, 1, 20, 100, 2, "roco", 32, (2, 4, 32), "straddle empty_pair short_block idle_wave", dtype=BF),
          _c("rep5-bf16", 64, 5, 70, 13, 0, "roco", 33, (1, 3, 6), "ragged_rows short_block idle_wave", dtype=BF)]
BY_NAME = {c.name: c for c in CASES}
NON_EVICTING = ("empty-pairs", "straddle", "rep3")      # also run as accumulate=True, evict=False: every head's score rows are compared
VIEWS = ("straddle", "empty-pairs", "rep5", "boundaries-96")      # views against dense copies, immediate and deferred (L = 3)
TWO_STEPS = ("straddle", "empty-pairs")


def with_layers(case, L):
    return case._replace(L=L, layer_begin=0)


def cap_of(case):
    return (case.T0 + case.n + 16 + 63) // 64 * 64      # (whole multiples of 64, as KVBank rounds it)


def plan_kw(case, evict=True):
    """StepPlan keywords (easykv_amd.StepPlan and the oracle's alike) without n_split; `evict=False`: the accumulate-only form."""
    scored = case.policy != "full"
    return dict(policy=case.policy, phase="prefill", accumulate=scored, evict=scored and evict, budget=case.T0, recent=case.T0 // 10, sink=SINK,
                stride=case.n, tova_head_mean=False)


def step_fields(case, evict=True, n_split=None):
    """The ekv_step of the case's call as KVBank.make_step fills it, as keywords of tests/test_dispatch_table._case."""
    kw = plan_kw(case, evict)
    n_evict = case.n if kw["evict"] else 0
    win = dict(win_lo=kw["sink"], win_tail=kw["recent"], roco_k1=max(kw["budget"] - kw["recent"] - kw["sink"], n_evict)) if n_evict else \
        dict(win_lo=0, win_tail=0, roco_k1=0)
    return dict(head_dim=case.D, hq=case.H * case.rep, h=case.H, n_layers=case.L, cap=cap_of(case), layer_begin=case.layer_begin,
                layer_count=case.L - case.layer_begin, q_len=case.n, n_slots=case.T0 + case.n, policy=POLICY_CODES[case.policy],
                accumulate=int(kw["accumulate"]), n_evict=n_evict, count_add2=2 * case.n, n_split=case.n_split if n_split is None else n_split,
                phys_extent=cap_of(case), **win)


# ---- the kernel's geometry, restated: ekv_plan.cpp (rows_per_split) and ekv_attn_chunk8.inc (t0, t1, the append rule) ----------------------
def geometry(case, n_split, qb_rows):
    """Every (split, query block) workgroup of one head: its queries [i0, i0 + nb), its key range [t0, t1) (empty when t0 >= t1), the
    new positions [j_lo, j_hi) whose rows it stores, and the folded rows NR = rep * nb of its block."""
    T, n = case.T0 + case.n, case.n
    ceil = lambda a, b: -(-a // b)
    rps = ceil(ceil(T, max(n_split, 1)), KT) * KT      # align64(ceil(T / n_split))
    wgs = []
    for split in range(ceil(T, rps)):
        for i0 in range(0, n, qb_rows):
            nb = min(qb_rows, n - i0)
            t0 = split * rps
            t1 = min(T, t0 + rps, T - n + i0 + nb)
            j_lo, j_hi = max(T - n + i0, t0), min(T - n + i0 + nb, t1)
            wgs.append(dict(split=split, i0=i0, nb=nb, t0=t0, t1=t1, j_lo=j_lo, j_hi=max(j_hi, j_lo), NR=case.rep * nb))
    return rps, wgs


def edges(case, n_split, qb_rows):
    """The names of the edges the case reaches under the plan (n_split, qb_rows)."""
    T, n, t_new = case.T0 + case.n, case.n, case.T0
    rps, wgs = geometry(case, n_split, qb_rows)
    got = set()
    stores = [0] * n      # how many workgroups store each new row: the append rule says exactly one
    for w in wgs:
        for j in range(w["j_lo"], w["j_hi"]):
            stores[j - t_new] += 1
    assert stores == [1] * n, (case.name, stores)
    if any(t_new < b < T for b in range(rps, T, rps)):
        got.add("straddle")          # new rows on both sides of a split boundary: two workgroups each store their part
    if any(w["t0"] >= w["t1"] for w in wgs):
        got.add("empty_pair")        # a workgroup with nothing to stage: partial (-inf, 0, 0), its whole logits range filled with -inf
    if any(w["nb"] < qb_rows for w in wgs):
        got.add("short_block")
    if any(w["NR"] <= 16 for w in wgs):
        got.add("idle_wave")         # query wave 1 returns from consume() and still takes every barrier
    if any(w["NR"] % 16 for w in wgs) and case.rep not in (1, 2, 4, 8, 16, 32):
        got.add("ragged_rows")       # trailing lanes of a query tile are not rows; row % rep, row / rep for a rep that is no power of two
    if qb_rows == 1 or any(w["nb"] == 1 for w in wgs):
        got.add("one_query_blocks")
    if any(w["t0"] < w["t1"] and min(abs(w["t1"] - b) for b in range(0, T + 64, 32)) <= 1 for w in wgs):
        got.add("ends_near_32")      # consume() works in 32-key halves, fill_lo rounds up to 32, tile_mixed decides per 64
    if t_new % KT == 0:
        got.add("starts_on_tile")
    if t_new // KT != (T - 1) // KT and t_new % KT:
        got.add("crosses_tile")
    if n_split == 1 and len(wgs) == 1 and case.policy != "full":
        got.add("fused_tail")        # one launch: the scorer runs as the kernel's tail
    if case.layer_begin > 0 and case.layer_begin + 1 < case.L:
        got.add("layer_offset")      # head_row uses layer_begin + ll; q, k_new, logits and partials use ll
    return got


# ---- seeded inputs --------------------------------------------------------------------------------------------------------------------
def evicted_positions(case):
    """The three positions compacted out after loading (`_bank` of tests/test_hip_kv8_chunk.py: 2, 11, 30; T0 < 31: the last row instead of 30)."""
    return (2, 11, 30) if case.T0 >= 31 else (2, 11, case.T0 + 2)


def draw(case, steps=1):
    """The CPU tensors of a case: k0 / v0 [L, H, T0 + 3, D] (None for an empty bank) in the case's dtype, warm [L, H, T0], perm [L, H, cap]
    (the physical row every slot-map entry is moved to) and, per step, (q, k, v) of the layers that step."""
    L, H, D, T0, n, dtype = case.L, case.H, case.D, case.T0, case.n, case.dtype
    g = torch.Generator().manual_seed(case.seed)
    vs = 0.25 if dtype is BF else 1.0
    d = dict(vs=vs, k0=None, v0=None, warm=None)
    if T0:
        k0, v0 = torch.randn(L, H, T0 + 3, D, generator=g), torch.randn(L, H, T0 + 3, D, generator=g) * vs
        if dtype is BF:
            v0.clamp_(-0.24, 0.24)
        k0[:, :, 5, 3], v0[:, :, 9, 1] = 300.0, (80.0 if dtype is F16 else 0.24)
        k0[:, :, 7], v0[:, :, 7] = 0.0, 0.0
        d.update(k0=k0.to(dtype), v0=v0.to(dtype), warm=torch.rand(L, H, T0, generator=g) * 1e-3)
    d["perm"] = torch.stack([torch.randperm(cap_of(case), generator=g) for _ in range(L * H)]).view(L, H, -1)
    lc = L - case.layer_begin
    d["tokens"] = []
    for _ in range(steps):
        q, k = torch.randn(lc, H * case.rep, n, D, generator=g).to(dtype), torch.randn(lc, H, n, D, generator=g).to(dtype)
        v = (torch.randn(lc, H, n, D, generator=g) * vs).clamp_(-80 * vs, 0.96 * vs).to(dtype)
        k[:, :, n // 2], v[:, :, n // 2] = 0, 0      # an all-zero new row
        d["tokens"].append((q, k, v))
    return d


def build_bank(case, d):
    """The case's quantised bank on the GPU, physical rows scattered by d['perm']."""
    from easykv_amd import KVBank
    L, H, T0, n = case.L, case.H, case.T0, case.n
    if not T0:
        bank = KVBank(L, H * case.rep, H, case.D, cap=cap_of(case), dtype=case.dtype, kv_quant="fp8", quant_chunks=True)
    else:
        bank = KVBank(L, H * case.rep, H, case.D, cap=cap_of(case), dtype=case.dtype)
        bank.load_rows(d["k0"].cuda(), d["v0"].cuda())
        bank.compact_inplace(torch.tensor(evicted_positions(case), dtype=torch.int32).expand(L, H, 3).contiguous())
        bank.state_init(T0 + n, 2, n)
        bank.score_sum[:, :, :T0] += d["warm"].cuda()
        bank.score_sq[:, :, :T0] += (d["warm"] ** 2).cuda()
        bank.quantize_fp8(chunks=True)
    assert bank.cap == cap_of(case)
    scatter_rows(bank, d["perm"].cuda())
    # the step's workspace, filled with a finite value (fp32 0.0115): a logit, partial or row statistic that a kernel leaves unwritten and
    # a later one reads is then a wrong number, not whatever an earlier test of the same geometry left in the allocator's block
    bank._workspace(WS_BYTES).fill_(0x3C)
    return bank


def scatter_rows(bank, perm):
    """Move physical row r of every head to perm[r] (codes and scales) and send the slot map, free list included, after it."""
    for name in ("k8", "v8", "k_scale", "v_scale"):
        plane = getattr(bank, name)
        idx = perm if plane.dim() == 3 else perm.unsqueeze(-1).expand_as(plane)
        plane.copy_(torch.empty_like(plane).scatter_(2, idx, plane))
    bank.slot_of_pos.copy_(torch.gather(perm, 2, bank.slot_of_pos.long()).int())
    bank.extent = [bank.cap] * bank.n_layers      # (live rows anywhere below cap)


# ---- the CPU restatement ----------------------------------------------------------------------------------------------------------------
def restate(case, d, step=0):
    """The float64 oracle step of every stepping layer on the rule's restatement of the bank.  Returns per layer (o_ref, ids_ref, exact):
    exact = the heads whose decision the probe calls stable and whose roco feasible set cuts no tied class."""
    from oracle import easykv_oracle as O
    from tests.select_rule import feasible_classes
    from tests.test_hip_d256 import _ProbeAndCapture
    from tests.test_hip_kv8_chunk import _f64
    assert step == 0, "later steps depend on the victims of the earlier ones: the GPU test re-seeds the oracle from the bank"
    L, H, T0, n = case.L, case.H, case.T0, case.n
    kw = plan_kw(case)
    q, k, v = d["tokens"][0]
    kq, vq = (R.dequant(*R.quantize(x)).double() for x in (k, v))
    keep = [p for p in range(T0 + 3) if p not in evicted_positions(case)]
    out = []
    for ll, l in enumerate(range(case.layer_begin, L)):
        if T0:
            st = O.LayerState(k=R.dequant(*R.quantize(d["k0"][l:l + 1, :, keep])), v=R.dequant(*R.quantize(d["v0"][l:l + 1, :, keep])))
            st.s, st.q, st.c = O.init_state_prefill((H,), T0, n, False)
            st.s[:, :T0] += d["warm"][l]
            st.q[:, :T0] += d["warm"][l] ** 2
        else:
            st = O.LayerState(k=torch.zeros(1, H, 0, case.D), v=torch.zeros(1, H, 0, case.D))
        hook = _ProbeAndCapture()
        O.SELECT_HOOK = hook
        try:
            o_ref, ids_ref = O.layer_step(_f64(st), q[ll:ll + 1].double(), kq[ll:ll + 1], vq[ll:ll + 1], O.StepPlan(**kw))
        finally:
            O.SELECT_HOOK = None
        exact = []
        if ids_ref is not None:
            k1 = max(T0 - kw["recent"] - SINK, n)
            for h in range(H):
                if bool(hook.probe.last_unstable[h]):
                    continue
                if case.policy == "roco":
                    c = hook.cap
                    _, pool, need = feasible_classes(O.roco_std(c.s, c.q, c.c, SINK)[h], k1)
                    if len(pool) != need:
                        continue
                exact.append(h)
        out.append((o_ref, ids_ref, exact))
    return out
