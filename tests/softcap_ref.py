"""The attention of a soft-capped / freely scaled model, as the oracle's `attention_core`: a restatement of the eager attention forward
of HF transformers' Gemma 2 (`eager_attention_forward`, modeling_gemma2.py):

    w = matmul(q, k^T) * scaling;  if softcap is not None: w = w / softcap; w = tanh(w); w = w * softcap;  w = w + mask;
    p = softmax(w, dim=-1, dtype=float32).to(q.dtype);  o = matmul(p, v)

`oracle.easykv_oracle.layer_step` and `generate` look `attention_core` up in the module's globals at call time, so `patched(...)`
swaps it for the duration of a test and nothing under oracle/ changes.  With cap=None and scale=None the replacement IS the oracle's
own function (the division by sqrt(head_dim) included).  `track`: the replacement also evaluates the uncapped, standard-scale attention
on the same rows and keeps the largest |o - o_plain| it saw — how far the model under test is from the one the library served before."""
import contextlib
import math

import torch


def make_core(cap=None, scale=None, track=None):
    def core(q, k, v, mask=None):
        hq, h = q.shape[1], k.shape[1]
        rep = hq // h
        if rep > 1:
            k = k[:, :, None].expand(1, h, rep, k.shape[2], k.shape[3]).reshape(1, hq, k.shape[2], k.shape[3])
            v = v[:, :, None].expand(1, h, rep, v.shape[2], v.shape[3]).reshape(1, hq, v.shape[2], v.shape[3])
        raw = torch.matmul(q, k.transpose(2, 3))
        w = raw / math.sqrt(q.shape[-1]) if scale is None else raw * scale
        if cap is not None:
            w = w / cap
            w = torch.tanh(w)
            w = w * cap
        if mask is not None:
            w = w + mask
        p = torch.softmax(w, dim=-1, dtype=torch.float32).to(q.dtype)
        o = torch.matmul(p, v)
        if track is not None:
            w0 = raw / math.sqrt(q.shape[-1])
            if mask is not None:
                w0 = w0 + mask
            o0 = torch.matmul(torch.softmax(w0, dim=-1, dtype=torch.float32).to(q.dtype), v)
            track[0] = max(track[0], float((o - o0).abs().max()))
        return o, p
    return core


@contextlib.contextmanager
def patched(cap=None, scale=None, track=None):
    """oracle.easykv_oracle.attention_core = the capped / scaled attention, for the duration of the block."""
    from oracle import easykv_oracle as O
    saved = O.attention_core
    O.attention_core = make_core(cap, scale, track)
    try:
        yield
    finally:
        O.attention_core = saved
