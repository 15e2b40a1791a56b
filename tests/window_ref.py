"""The attention of a model with per-layer sliding windows, as the oracle's `attention_core` (in the manner of tests/sink_ref.py): HF
transformers' `sliding_window_overlay` (masking_utils.py: a key is attended iff kv_idx > q_idx - sliding_window) over TOKEN positions,

    masked(h, i, j)  iff  W > 0  and  q_pos[i] - key_pos[h][j] >= W

added to the logits as `finfo.min` before the softmax, per KV head (eviction is per head: the retained token positions differ), optionally
with gpt-oss's attention sinks (the extra softmax column of tests/sink_ref.py, never masked).

The oracle keeps no token positions: the TEST holds, for every head, the list of token positions of the retained keys and deletes the
oracle's `ids_ref` from it after every evicting step.  `patched(window, key_pos, q_pos, sinks)` swaps `oracle.easykv_oracle.attention_core`
for the duration of one layer's step, where `key_pos` is [H, T] — the retained positions with the step's own appended behind them — and
`q_pos` the positions of the step's n queries; `model_core(windows, sinks)` is the `core` hook of oracle.fake_model.FakeAttnModel for
`generate`, which recovers the positions from the rows themselves.  With window = 0 the replacement IS the oracle's own function (sinks=None) or the sink
core.  `track`: the replacement also evaluates the full (unwindowed) attention on the same rows and keeps the largest |o - o_full| it saw:
how far the model under test is from the one that ignores the window."""
import contextlib
import math

import torch

from tests import sink_ref


def make_core(window=0, key_pos=None, q_pos=None, sinks=None, track=None):
    """window: int >= 0; key_pos: int [H, T]; q_pos: int [n]; sinks: [Hq] (fp32) or None."""
    if not window:
        if sinks is None:
            from oracle import easykv_oracle as O
            return O.attention_core
        return sink_ref.make_core(sinks)
    key_pos = torch.as_tensor(key_pos).long()
    q_pos = torch.as_tensor(q_pos).long().reshape(-1)

    def core(q, k, v, mask=None):
        hq, h = q.shape[1], k.shape[1]
        rep = hq // h
        assert tuple(key_pos.shape) == (h, k.shape[2]) and q_pos.numel() == q.shape[2], (key_pos.shape, k.shape, q_pos.shape)
        if rep > 1:
            k = k[:, :, None].expand(1, h, rep, k.shape[2], k.shape[3]).reshape(1, hq, k.shape[2], k.shape[3])
            v = v[:, :, None].expand(1, h, rep, v.shape[2], v.shape[3]).reshape(1, hq, v.shape[2], v.shape[3])
        w = torch.matmul(q, k.transpose(2, 3)) / math.sqrt(q.shape[-1])
        if mask is not None:
            w = w + mask
        out_of_window = (q_pos[None, :, None] - key_pos[:, None, :]) >= window      # [H, n, T]
        overlay = torch.zeros(out_of_window.shape, dtype=w.dtype).masked_fill(out_of_window, torch.finfo(w.dtype).min)
        ww = w + overlay.repeat_interleave(rep, dim=0)[None]

        def soft(x):
            if sinks is None:
                return torch.softmax(x, dim=-1, dtype=torch.float32).to(q.dtype)
            col = sinks.to(x.dtype).reshape(1, hq, 1, 1).expand(1, hq, x.shape[2], 1)
            combined = torch.cat([x, col], dim=-1)
            combined = combined - combined.max(dim=-1, keepdim=True).values
            return torch.softmax(combined, dim=-1, dtype=torch.float32)[..., :-1].to(q.dtype)
        p = soft(ww)
        o = torch.matmul(p, v)
        if track is not None:
            track[0] = max(track[0], float((o - torch.matmul(soft(w), v)).abs().max()))
        return o, p
    return core


@contextlib.contextmanager
def patched(window=0, key_pos=None, q_pos=None, sinks=None, track=None):
    """oracle.easykv_oracle.attention_core = the windowed attention of one layer's step, for the duration of the block."""
    from oracle import easykv_oracle as O
    saved = O.attention_core
    O.attention_core = make_core(window, key_pos, q_pos, sinks, track)
    try:
        yield
    finally:
        O.attention_core = saved


def model_core(windows, sinks=None, track=None):
    """The `core` hook of oracle.fake_model.FakeAttnModel: layer `layer` attends under windows[layer], with sinks[layer] ([L, Hq]) where
    given.  The oracle stores K verbatim and the fake model's rows are random, hence distinct: the token position of a retained key (and
    of a query) is recovered by matching its row against the rows of the layer's stream."""
    def where(rows, stream):      # rows [T, D], stream [P, D] -> the index in the stream of every row
        hit = (rows[:, None, :] == stream[None, :, :]).all(-1)
        assert bool((hit.sum(-1) == 1).all()), "a row of the cache is not exactly one row of the stream"
        return hit.float().argmax(-1)

    def core(model, q, k, v, mask, layer):
        sk = None if sinks is None else sinks[layer].float()
        if not windows[layer]:
            return make_core(0, sinks=sk)(q, k, v, mask)
        key_pos = torch.stack([where(k[0, h], model.ks[layer][h]) for h in range(k.shape[1])])
        q_pos = where(q[0, 0], model.qs[layer][0])
        return make_core(windows[layer], key_pos, q_pos, sk, track)(q, k, v, mask)
    return core


def drop_positions(pos, ids):
    """pos: list (per head) of lists of token positions, in cache order; ids [H, k]: the oracle's evicted cache indices.  In place."""
    for h, row in enumerate(pos):
        for j in sorted((int(x) for x in ids[h]), reverse=True):
            del row[j]
