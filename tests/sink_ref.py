"""The attention of a model with learned attention sinks, as the oracle's `attention_core`: a restatement of the eager attention forward of
HF transformers' gpt-oss (`eager_attention_forward`, modeling_gpt_oss.py):

    w = matmul(q, k^T) * scaling + mask;  combined = cat([w, sinks], -1);  combined = combined - combined.max(-1)
    p = softmax(combined, dim=-1)[..., :-1];  o = matmul(p, v)

`sinks` is one logit per query head ([Hq]); it joins every softmax of that head as an extra column, which is then dropped: the
probabilities of the real keys no longer sum to 1.  `p` — what the oracle's scorers accumulate — is the truncated matrix.

`oracle.easykv_oracle.layer_step` looks `attention_core` up in the module's globals at call time, so `patched(sinks_of_the_layer)` swaps
it for the duration of one layer's step and nothing under oracle/ changes; `model_core(sinks)` is the `core(model, q, k, v, mask,
layer)` hook of `oracle.fake_model.FakeAttnModel` for `generate`, where the layer picks the row of `sinks` ([L, Hq]).  With sinks=None the
replacement IS the oracle's own function.  `track`: the replacement also evaluates the sink-free attention on the same rows and keeps
the largest |o - o_plain| it saw — how far the model under test is from the one the library served before."""
import contextlib
import math

import torch


def make_core(sinks=None, track=None):
    """sinks: [Hq] (fp32), or None."""
    def core(q, k, v, mask=None):
        hq, h = q.shape[1], k.shape[1]
        rep = hq // h
        if rep > 1:
            k = k[:, :, None].expand(1, h, rep, k.shape[2], k.shape[3]).reshape(1, hq, k.shape[2], k.shape[3])
            v = v[:, :, None].expand(1, h, rep, v.shape[2], v.shape[3]).reshape(1, hq, v.shape[2], v.shape[3])
        w = torch.matmul(q, k.transpose(2, 3)) / math.sqrt(q.shape[-1])
        if mask is not None:
            w = w + mask
        if sinks is None:
            p = torch.softmax(w, dim=-1, dtype=torch.float32).to(q.dtype)
        else:
            col = sinks.to(w.dtype).reshape(1, hq, 1, 1).expand(1, hq, w.shape[2], 1)
            combined = torch.cat([w, col], dim=-1)
            combined = combined - combined.max(dim=-1, keepdim=True).values
            p = torch.softmax(combined, dim=-1, dtype=torch.float32)[..., :-1].to(q.dtype)
        o = torch.matmul(p, v)
        if track is not None:
            o0 = torch.matmul(torch.softmax(w, dim=-1, dtype=torch.float32).to(q.dtype), v)
            track[0] = max(track[0], float((o - o0).abs().max()))
        return o, p
    return core


@contextlib.contextmanager
def patched(sinks=None, track=None):
    """oracle.easykv_oracle.attention_core = the attention with these sinks ([Hq]: one layer's), for the duration of the block."""
    from oracle import easykv_oracle as O
    saved = O.attention_core
    O.attention_core = make_core(sinks, track)
    try:
        yield
    finally:
        O.attention_core = saved


def model_core(sinks, track=None):
    """The `core` hook of oracle.fake_model.FakeAttnModel: layer `layer` attends with sinks[layer] ([L, Hq])."""
    cores = [make_core(sinks[l].float(), track) for l in range(sinks.shape[0])]

    def core(model, q, k, v, mask, layer):
        return cores[layer](q, k, v, mask)
    return core
