"""One-shot prompt compression with pooled observation-window scores, composed from the oracle's primitives (include/easykv_hip.h,
"pooled selection" and "one-shot prefill"): `attention_core`, `causal_chunk_mask`, `gqa_fold`, `accumulate_chunk`, `_select_prefill`
called with k = n_evict, `drop_columns`, `drop_kv_slots`; the pooling is `torch.nn.functional.{max,avg}_pool1d` on the slice s[R] ahead of
the oracle's `topk(largest=False)`.  For a sink or window model, swap `oracle.easykv_oracle.attention_core` (tests/sink_ref.py,
tests/window_ref.py: `patched(...)`) around the call, as those tests do.

The tolerance class.  Many-victim selection over pooled values produces exact ties (max) and near-ties (avg), and topk promises no order
among them.  With theta the n_evict-th smallest reference pooled value of a row, a column is DECIDED if its pooled value differs from
theta by more than rtol 2e-5, atol 1e-7 (the project's tolerance for score rows, tests/test_hip_window.py).  Every decided column must
match the reference (below theta: a victim; above: kept); the undecided ones must bring the victim count to exactly n_evict.  A row is
only a meaningful comparison if at least 90 % of its candidate columns and at least 10 of its victims are decided (`row_class`)."""
import torch
import torch.nn.functional as F

from oracle import easykv_oracle as O

RTOL, ATOL = 2e-5, 1e-7


def pooled_slice(s, sink, obs, pool, op):
    """s [..., W] -> the ranking values of the candidate range R = [sink, W - obs): what torch computes on s[R], nothing else."""
    r = s[..., sink:s.shape[-1] - obs]
    if pool == 1:
        return r.clone()
    x = r.reshape(-1, 1, r.shape[-1])
    y = F.max_pool1d(x, pool, stride=1, padding=pool // 2) if op == "max" else F.avg_pool1d(x, pool, stride=1, padding=pool // 2)
    return y.reshape(r.shape)


def ranking_rows(policy, s, sink, obs, pool, op):
    """The rows `_select_prefill` ranks: s with its candidate range replaced by the pooled values (roco is never pooled)."""
    if pool == 1 or policy == "roco":
        return s
    rank = s.clone()
    rank[..., sink:s.shape[-1] - obs] = pooled_slice(s, sink, obs, pool, op)
    return rank


def observation_step(st, qn, kn, vn, policy, n_evict, sink, pool=1, op="max", tova_head_mean=False):
    """Forward B of one layer: the last `obs` tokens as one chunk step over all n keys, scored, pooled, selected once.  `st`: the
    oracle's LayerState with the n - obs cached rows and score rows of n columns (O.init_state_prefill((H,), n - obs, obs, False)).
    Returns (o [1, Hq, obs, D], ids [H, n_evict], the ranking rows [H, n] the selection saw); `st` is left accumulated, NOT compacted
    (`compact` does that, with the victims of whoever's choice is being followed)."""
    h, obs = kn.shape[1], qn.shape[2]
    rep = qn.shape[1] // h
    st.k, st.v = torch.cat((st.k, kn), dim=2), torch.cat((st.v, vn), dim=2)
    t = st.k.shape[2]
    o, p = O.attention_core(qn, st.k, st.v, O.causal_chunk_mask(obs, t, qn.dtype))
    O.accumulate_chunk(policy, st.s, st.q, O.gqa_fold(p, h, rep)[0], tova_head_mean)
    st.c += float(obs)
    rank = ranking_rows(policy, st.s, sink, obs, pool, op)
    ids = O._select_prefill(policy, rank, st.q, st.c, t, obs, sink, n_evict)
    return o, ids, rank


def compact(st, ids, policy):
    """Order-preserving removal of `ids` [H, k] from the rows and the score rows, the count tail as the strided prefill leaves it."""
    k = ids.shape[-1]
    st.k, st.v = O.drop_kv_slots(st.k, ids), O.drop_kv_slots(st.v, ids)
    st.s = O.drop_columns(st.s, ids, torch.zeros(k))
    st.q = O.drop_columns(st.q, ids, torch.zeros(k))
    st.c = O.drop_columns(st.c, ids, -torch.arange(k, dtype=torch.float32))


def row_class(rank_row, n_evict, sink, obs):
    """One ranking row [W] -> (must: columns every valid answer evicts, free: the undecided columns, n_candidates)."""
    w = rank_row.shape[-1]
    vals = rank_row[sink:w - obs].double()
    theta = torch.kthvalue(vals, n_evict).values
    tol = ATOL + RTOL * theta.abs()
    must = torch.nonzero(vals < theta - tol).flatten() + sink
    free = torch.nonzero((vals - theta).abs() <= tol).flatten() + sink
    return set(must.tolist()), set(free.tolist()), vals.numel()


def meets_cap(rank_row, n_evict, sink, obs):
    must, free, n_cand = row_class(rank_row, n_evict, sink, obs)
    return len(free) <= 0.1 * n_cand and len(must) >= 10


def valid(victims, rank_row, n_evict, sink, obs):
    """Is `victims` (n_evict column indices) an answer of the class: distinct, every decided victim in, no decided keeper in?"""
    must, free, _ = row_class(rank_row, n_evict, sink, obs)
    v = set(int(x) for x in victims)
    return len(v) == n_evict == len(list(victims)) and must <= v and v <= (must | free)


def prompt_state(ks, vs, layer, n, obs):
    """LayerState of `layer` after forward A and state_init(n, mode 2): the first n - obs rows of the fp16 streams, widened."""
    st = O.LayerState(k=ks[layer][:, :n - obs].unsqueeze(0).float(), v=vs[layer][:, :n - obs].unsqueeze(0).float())
    st.s, st.q, st.c = O.init_state_prefill((ks.shape[1],), n - obs, obs, False)
    return st


def generate(qs, ks, vs, n, cfg, mode, follow=None, on_decode=None, vocab=16):
    """The test-side driver over the streams of oracle.fake_model (q / k / v of the token at position t are rows t): forward A, forward
    B, hand-over, decode by the mode's rule.  cfg: budget (int), kv_policy, temp_length, obs_window, score_pool, score_pool_op,
    max_new_tokens.  `follow`: optional callable (layer, ids_ref [H, k], rank [H, n]) -> ids to compact with — the device's victims,
    once the caller has held them to the class — so that later steps compare like with like; `on_decode(layer, step, ids_ref [H, 1])`
    is called after every evicting decode step of auto mode (with oracle.SELECT_HOOK set by the caller, a stability probe has just seen
    the decision).  Returns dict(tokens, printed, positions
    [L][H] lists of the retained token positions, rank [L] rows, ids [L])."""
    L, hq, h = qs.shape[0], qs.shape[1], ks.shape[1]
    B, policy, sink = cfg["budget"], cfg["kv_policy"], cfg.get("temp_length", 4)
    obs, pool, op, m = cfg.get("obs_window", 32), cfg.get("score_pool", 7), cfg.get("score_pool_op", "max"), cfg.get("max_new_tokens", 8)
    states, positions, ranks, all_ids = [], [], [], []
    sl = slice(n - obs, n)
    for l in range(L):
        st = prompt_state(ks, vs, l, n, obs)
        _, ids, rank = observation_step(st, qs[l][:, sl].unsqueeze(0).float(), ks[l][:, sl].unsqueeze(0).float(), vs[l][:, sl].unsqueeze(0).float(),
                                        policy, n - B, sink, pool, op, tova_head_mean=(mode == "encoding"))
        use = ids if follow is None else follow(l, ids, rank)
        compact(st, use, policy)
        pos = [[p for p in range(n) if p not in set(use[hh].tolist())] for hh in range(h)]
        states.append(st), positions.append(pos), ranks.append(rank), all_ids.append(ids)
    tokens = [(n + i) % vocab for i in range(m)]
    if mode == "encoding":
        printed = f"KV cache budget ratio: {B / n * 100:.2f}%({B}/{n})"
        for l in range(L):
            for hh in range(h):
                positions[l][hh] += list(range(n, n + m))
    else:      # auto: the decode policy over the whole cache with budget B, on the score rows forward B left (their first B + 1 columns)
        plan = O.StepPlan(policy=policy, phase="decode", accumulate=True, evict=True, score_off=0, budget=B)
        for l in range(L):
            st = states[l]
            st.s, st.q, st.c = st.s[:, :B + 1].clone(), st.q[:, :B + 1].clone(), st.c[:, :B + 1].clone()
            for i in range(m):
                p = n + i
                _, ids = O.layer_step(st, qs[l][:, p:p + 1].unsqueeze(0).float(), ks[l][:, p:p + 1].unsqueeze(0).float(),
                                      vs[l][:, p:p + 1].unsqueeze(0).float(), plan)
                if on_decode is not None:
                    on_decode(l, i, ids)
                for hh in range(h):
                    positions[l][hh].append(p)
                    del positions[l][hh][int(ids[hh, 0])]
        printed = f"KV Cache Budget ratio {B / (n + m) * 100:.2f}%[{B}/({n}+{m})]"
    return dict(tokens=" ".join(str(t) for t in tokens), printed=printed, positions=positions, rank=ranks, ids=all_ids)
