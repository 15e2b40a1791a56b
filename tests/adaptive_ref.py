"""Adaptive head budgets (include/easykv_hip.h, "adaptive head budgets"), composed from tests/oneshot_ref.py (`observation_step`, whose
ranking rows are `pooled_slice` of the oracle's accumulated score rows) and the oracle's primitives (`drop_columns`, `drop_kv_slots`).

The rule, on the ranking rows rank [H, W] of one layer, candidates R = [sink, W - obs), C = |R|: a head's elements are ordered by
(value, j), NaN largest; its evict_min smallest are FORCED, its C - evict_max largest PROTECTED, the rest FREE; the layer evicts all forced
elements and the H * (n_evict - evict_min) smallest free ones in the order (value, head, j); k_h is head h's share, and its victims are
its own k_h smallest.

The tolerance class.  It is tests/oneshot_ref.py's `row_class` with one theta per LAYER — the value of the last free element taken —
plus two boundary thetas per head, the evict_min-th and the evict_max-th smallest value of the head.  With tol(theta) = ATOL + RTOL *
|theta| (the same RTOL / ATOL), a candidate of value x is
    a decided victim   if x < theta_min_h - tol (forced), or x < theta_max_h - tol and x < theta - tol (free, below the layer's threshold);
    a decided keeper   if x > theta_max_h + tol (protected), or x > theta_min_h + tol and x > theta + tol;
    undecided          otherwise.
A boundary that does not exist (evict_min = 0, evict_max = C, nothing or everything free taken) decides nothing against anybody.  An
answer is valid if every head's victims hold its decided victims and no decided keeper, every head's count lies within the bounds, and
the counts sum to H * n_evict.  A layer is a comparison only if at least 90 % of its candidates are decided and every head has at least
10 decided victims (`meets_cap`)."""
import math

import torch

from oracle import easykv_oracle as O
from tests import oneshot_ref as R

RTOL, ATOL = R.RTOL, R.ATOL


def _order(vals):
    """vals [C] -> indices in the order (value, j), NaN largest (a stable sort; torch sorts NaN last)."""
    return torch.sort(vals, stable=True).indices


def allot(rank, n_evict, evict_min, evict_max, sink, obs):
    """rank [H, W] -> (k [H] ints, victims: list of H ascending index tensors into the row), exactly by the rule."""
    H, W = rank.shape
    C = W - obs - sink
    assert 0 <= evict_min <= n_evict <= evict_max <= C
    orders = [_order(rank[h, sink:W - obs]) for h in range(H)]
    free = []      # (value as an orderable key, head, j)
    for h in range(H):
        vals = rank[h, sink:W - obs]
        for j in orders[h][evict_min:evict_max].tolist():
            x = float(vals[j])
            free.append((math.inf if x != x else x, x != x, h, j))      # NaN behind +inf
    free.sort()
    k = [evict_min] * H
    for _, _, h, _ in free[:H * (n_evict - evict_min)]:
        k[h] += 1
    victims = [torch.sort(orders[h][:k[h]]).values + sink for h in range(H)]
    return k, victims


def thetas(rank, n_evict, evict_min, evict_max, sink, obs):
    """(theta of the layer or None, [theta_min_h or None], [theta_max_h or None]) in float64."""
    H, W = rank.shape
    C = W - obs - sink
    vals = rank[:, sink:W - obs].double()
    srt = torch.sort(vals, dim=-1).values
    t_min = [srt[h, evict_min - 1].item() if evict_min > 0 else None for h in range(H)]
    t_max = [srt[h, evict_max - 1].item() if evict_max < C else None for h in range(H)]
    m = H * (n_evict - evict_min)
    theta = None
    if 0 < m < H * (evict_max - evict_min):
        theta = torch.sort(srt[:, evict_min:evict_max].flatten()).values[m - 1].item()
    return theta, t_min, t_max, m


def layer_class(rank, n_evict, evict_min, evict_max, sink, obs):
    """Per head: (must: decided victims, maybe: undecided candidates) as sets of row indices, and the number of candidates."""
    H, W = rank.shape
    theta, t_min, t_max, m = thetas(rank, n_evict, evict_min, evict_max, sink, obs)
    tol = lambda t: ATOL + RTOL * abs(t)
    all_free_taken = m > 0 and theta is None
    out = []
    for h in range(H):
        x = rank[h, sink:W - obs].double()
        true, false = torch.ones_like(x, dtype=torch.bool), torch.zeros_like(x, dtype=torch.bool)
        forced = x < t_min[h] - tol(t_min[h]) if t_min[h] is not None else false
        not_forced = x > t_min[h] + tol(t_min[h]) if t_min[h] is not None else true
        protected = x > t_max[h] + tol(t_max[h]) if t_max[h] is not None else false
        not_protected = x < t_max[h] - tol(t_max[h]) if t_max[h] is not None else true
        if theta is not None:
            below, above = x < theta - tol(theta), x > theta + tol(theta)
        else:
            below, above = (true, false) if all_free_taken else (false, true)
        victim = forced | (not_protected & below)
        keeper = protected | (not_forced & above)
        must = set((torch.nonzero(victim).flatten() + sink).tolist())
        maybe = set((torch.nonzero(~victim & ~keeper).flatten() + sink).tolist())
        out.append((must, maybe))
    return out, W - obs - sink


def meets_cap(rank, n_evict, evict_min, evict_max, sink, obs):
    cls, C = layer_class(rank, n_evict, evict_min, evict_max, sink, obs)
    return sum(len(maybe) for _, maybe in cls) <= 0.1 * C * len(cls) and all(len(must) >= 10 for must, _ in cls)


def valid(victims, rank, n_evict, evict_min, evict_max, sink, obs):
    """victims: H sequences of row indices.  Is it an answer of the class?"""
    cls, _ = layer_class(rank, n_evict, evict_min, evict_max, sink, obs)
    total = 0
    for (must, maybe), v in zip(cls, victims):
        s = set(int(x) for x in v)
        if len(s) != len(list(v)) or not (evict_min <= len(s) <= evict_max) or not (must <= s <= (must | maybe)):
            return False
        total += len(s)
    return total == len(cls) * n_evict


def compact_heads(st, victims, policy):
    """Per-head states after compaction: head h loses victims[h] (order-preserving; the score rows get the count tail of tests/
    oneshot_ref.py's `compact`).  Returns a list of H dicts(k, v [T_h, D], s, q, c [W]) — the heads no longer share a length."""
    heads = []
    for h, ids in enumerate(victims):
        ids = torch.as_tensor(ids, dtype=torch.long).reshape(1, -1)
        kk = ids.shape[-1]
        one = lambda x: x[h:h + 1]
        heads.append(dict(k=O.drop_kv_slots(st.k[:, h:h + 1], ids)[0, 0], v=O.drop_kv_slots(st.v[:, h:h + 1], ids)[0, 0],
                          s=O.drop_columns(one(st.s), ids, torch.zeros(kk))[0], q=O.drop_columns(one(st.q), ids, torch.zeros(kk))[0],
                          c=O.drop_columns(one(st.c), ids, -torch.arange(kk, dtype=torch.float32))[0]))
    return heads


def observation_step(st, qn, kn, vn, policy, n_evict, evict_min, evict_max, sink, pool=1, op="max"):
    """Forward B of one layer with adaptive head budgets: tests/oneshot_ref.py's step (accumulate, pool), then the rule above.  Returns
    (o [1, Hq, obs, D], k [H], victims [H] index tensors, the ranking rows [H, n]); `st` is left accumulated, NOT compacted."""
    o, _, rank = R.observation_step(st, qn, kn, vn, policy, n_evict, sink, pool, op)
    k, victims = allot(rank, n_evict, evict_min, evict_max, sink, qn.shape[2])
    return o, k, victims, rank


def budget_bounds(n, budget, obs, sink, floor=0.2, ceil=2.0):
    """(n_evict, evict_min, evict_max) the driver derives for a prompt of n tokens cut to `budget`: fractions of the uniform candidate
    keep K = C - n_evict."""
    C, n_evict = n - obs - sink, n - budget
    K = C - n_evict
    return n_evict, max(0, C - math.ceil(ceil * K)), C - math.floor(floor * K)


def generate(qs, ks, vs, n, cfg, mode, follow=None, on_decode=None, vocab=16):
    """tests/oneshot_ref.py's test-side driver with adaptive head budgets: forward A, forward B with the rule above, per-head states
    after compaction, decode by the mode's rule head by head (a head of a layer is a layer of one KV head to the oracle).  cfg as there,
    plus head_budget_floor / head_budget_ceil.  `follow(layer, victims_ref [H] tensors, rank [H, n], bounds)` -> the victims to compact
    with; `on_decode(layer, step, head, ids_ref [1, 1])` after every evicting decode step of auto mode.  Returns dict(tokens, printed,
    positions [L][H] lists, rank [L], k [L] lists, bounds)."""
    L, hq, h = qs.shape[0], qs.shape[1], ks.shape[1]
    rep = hq // h
    B, policy, sink = cfg["budget"], cfg["kv_policy"], cfg.get("temp_length", 4)
    obs, pool, op, m = cfg.get("obs_window", 32), cfg.get("score_pool", 7), cfg.get("score_pool_op", "max"), cfg.get("max_new_tokens", 8)
    ne, lo, hi = budget_bounds(n, B, obs, sink, cfg.get("head_budget_floor", 0.2), cfg.get("head_budget_ceil", 2.0))
    sl = slice(n - obs, n)
    heads, positions, ranks, counts = [], [], [], []
    for l in range(L):
        st = R.prompt_state(ks, vs, l, n, obs)
        _, k, victims, rank = observation_step(st, qs[l][:, sl].unsqueeze(0).float(), ks[l][:, sl].unsqueeze(0).float(),
                                               vs[l][:, sl].unsqueeze(0).float(), policy, ne, lo, hi, sink, pool, op)
        use = victims if follow is None else follow(l, victims, rank, (ne, lo, hi))
        heads.append(compact_heads(st, use, policy))
        positions.append([[p for p in range(n) if p not in set(int(x) for x in use[hh])] for hh in range(h)])
        ranks.append(rank), counts.append([len(u) for u in use])
    tokens = [(n + i) % vocab for i in range(m)]
    if mode == "encoding":
        printed = f"KV cache budget ratio: {B / n * 100:.2f}%({B}/{n})"
        for l in range(L):
            for hh in range(h):
                positions[l][hh] += list(range(n, n + m))
    else:      # auto: the decode policy over each head's whole cache, one victim per head and step, on the score rows forward B left
        plan = O.StepPlan(policy=policy, phase="decode", accumulate=True, evict=True, score_off=0, budget=B)
        for l in range(L):
            for hh in range(h):
                hd = heads[l][hh]
                t = hd["k"].shape[0]
                st = O.LayerState(k=hd["k"][None, None], v=hd["v"][None, None])
                st.s, st.q, st.c = hd["s"][None, :t + 1].clone(), hd["q"][None, :t + 1].clone(), hd["c"][None, :t + 1].clone()
                for i in range(m):
                    p = n + i
                    _, ids = O.layer_step(st, qs[l][hh * rep:(hh + 1) * rep, p:p + 1].unsqueeze(0).float(), ks[l][hh:hh + 1, p:p + 1].unsqueeze(0).float(),
                                          vs[l][hh:hh + 1, p:p + 1].unsqueeze(0).float(), plan)
                    if on_decode is not None:
                        on_decode(l, i, hh, ids)
                    positions[l][hh].append(p)
                    del positions[l][hh][int(ids[0, 0])]
        printed = f"KV Cache Budget ratio {B / (n + m) * 100:.2f}%[{B}/({n}+{m})]"
    return dict(tokens=" ".join(str(t) for t in tokens), printed=printed, positions=positions, rank=ranks, k=counts, bounds=(ne, lo, hi))
