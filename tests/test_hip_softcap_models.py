"""Soft-capped models end to end on the GPU: the drivers over fake models whose config carries attn_logit_softcapping (and, once, a
non-standard query_pre_attn_scalar) against the oracle's own run with HF's eager Gemma 2 attention (tests/softcap_ref.py), and a tiny
stock Gemma2ForCausalLM through hf.patch_model + enable_fixed_kv against its own eager forward.

The HF models: hidden 64, 2 layers, 4 / 2 heads, attn_logit_softcapping = 2.0, query_pre_attn_scalar = 64, initializer_range = 0.25 —
the default init (0.02, cap 50) makes the cap invisible (removing it moves the logits by 3e-7).  With this config, on the CPU in
fp32 over the 40-token prompt, removing the cap moves HF's eager logits by 5.9 (head_dim 256) / 5.4 (head_dim 128) and forcing the scale
back to 1 / sqrt(head_dim) by 1.1 / 0.46, against the seam bar of 3e-2; HF's own fp16 forward is within 1.1e-2 of its fp32 forward, so
initializer_range stays at 0.25.  The test checks both conditions again on the model it runs (each at least ten times the bar).
Prompts are shorter than sliding_window, so HF's eager result on the local layers is full attention."""
import contextlib
import io

import numpy as np
import pytest
import torch

from tests.softcap_ref import patched
from tests.test_hip_fullsize import Probe

pytestmark = pytest.mark.gpu
BAR = 3e-2      # the seam's logit bar (tests/test_hip_hf_adapter.py, tests/test_hip_d256.py)


# ---- (d) the drivers ----------------------------------------------------------------------------------------------------------------------
class _EventProbe(Probe):
    """The stability probe, one mask [L, H] per eviction event of oracle.generate."""

    def __init__(self):
        super().__init__()
        self.events = []

    def __call__(self, *args):
        super().__call__(*args)
        self.events.append(self.last_unstable.clone())


DRIVER_CASES = [
    # mode, stride, head_dim, policy, query_pre_attn_scalar
    ("decoding", 1, 128, "roco", None), ("decoding", 1, 256, "h2o_head", None), ("decoding", 1, 128, "h2o_head", 144),
    ("auto", 8, 128, "roco", None), ("auto", 8, 256, "roco", 224),
]


@pytest.mark.parametrize("mode,stride,D,policy,qpas", DRIVER_CASES, ids=[f"{c[0]}-d{c[2]}-{c[3]}" + (f"-qpas{c[4]}" if c[4] else "") for c in DRIVER_CASES])
def test_generate_on_a_capped_model_equals_the_capped_oracles_run(mode, stride, D, policy, qpas):
    import easykv_amd
    from oracle import easykv_oracle as O
    from oracle.fake_model import FakeAttnModel, make_streams
    from tests.golden_util import trace_events
    from tests.native_fake_model import NativeFakeModel
    from tests.test_hip_generate_batch import _evictions, _ids
    cap, length = 2.0, 120
    cfg = dict(budget=60, kv_policy=policy, max_new_tokens=24, recent_ratio=0.3)
    if mode == "decoding":
        cfg = dict(budget=60, kv_policy=policy, max_new_tokens=84)
    streams = make_streams(2, 4, 2, D, length + cfg["max_new_tokens"] + 8, seed=43)
    model = NativeFakeModel(*streams)
    model.config.attn_logit_softcapping = cap
    if qpas is not None:
        model.config.query_pre_attn_scalar = qpas
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        res, cache = easykv_amd.generate(model, _ids(length), dict(cfg, _record_evictions=True), kv_mode=mode, stride=stride, return_cache=True)
    line = buf.getvalue().strip()
    assert cache.logit_cap == cap and cache.bank.logit_cap == cap
    assert cache.sm_scale == (None if qpas is None else qpas ** -0.5) and cache.bank.sm_scale == cache.sm_scale
    probe, dist = _EventProbe(), [0.0]
    O.SELECT_HOOK = probe
    try:
        with patched(cap, None if qpas is None else qpas ** -0.5, dist):
            tr = O.generate(FakeAttnModel(*streams), _ids(length), cfg, kv_mode=mode, stride=stride)
    finally:
        O.SELECT_HOOK = None
    ours = _evictions(cache.evictions)
    kinds, ref, _ = trace_events(tr)
    assert len(ours) == len(ref) == len(probe.events) > 0 and not kinds.any(), (len(ours), len(ref), len(probe.events))
    alive = np.ones(ours[0].shape[:2], dtype=bool)
    n_checked = n_total = 0
    for e, (a, b) in enumerate(zip(ours, ref)):
        stable = ~probe.events[e].numpy()
        same = (a == b).all(-1)
        assert same[alive & stable].all(), (mode, D, policy, f"eviction ids differ at eviction {e}")
        n_total += alive.size
        n_checked += int((alive & stable).sum())
        alive &= stable & same
    print(f"[softcap] generate {mode} d{D} {policy}: compared {n_checked} of {n_total} decisions; max |o_capped - o_uncapped| = {dist[0]:.3e}")
    assert n_checked >= 10 and 2 * n_checked >= n_total and dist[0] >= 1e-2
    ref_text = tr.result if isinstance(tr.result, str) else " ".join(str(t) for t in tr.result)
    assert res == ref_text and line == tr.report.strip(), (res, ref_text, line, tr.report)


# ---- (e) the HF seam ----------------------------------------------------------------------------------------------------------------------
class _Tok:
    eos_token_id = -1

    def decode(self, ids, skip_special_tokens=True):
        return " ".join(str(i) for i in ids)


def _tiny_gemma2(D, cap=2.0, qpas=64, seed=0):
    import transformers
    torch.manual_seed(seed)
    cfg = transformers.Gemma2Config(vocab_size=97, hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=4,
                                    num_key_value_heads=2, head_dim=D, max_position_embeddings=512, attn_implementation="eager",
                                    attn_logit_softcapping=cap, query_pre_attn_scalar=qpas, initializer_range=0.25, sliding_window=256)
    return transformers.Gemma2ForCausalLM(cfg).half().cuda().eval()


@contextlib.contextmanager
def _attn(model, **attrs):
    """The attention modules of `model` with some attributes replaced (what HF's eager forward then computes)."""
    mods = [l.self_attn for l in model.model.layers]
    saved = [{k: getattr(m, k) for k in attrs} for m in mods]
    for m in mods:
        for k, v in attrs.items():
            setattr(m, k, v)
    try:
        yield
    finally:
        for m, s in zip(mods, saved):
            for k, v in s.items():
                setattr(m, k, v)


@pytest.mark.parametrize("D", [256, 128])
def test_stock_gemma2_through_the_seam(D):
    import easykv_amd
    from easykv_amd import hf
    model = _tiny_gemma2(D)
    attn = model.model.layers[0].self_attn
    assert type(model).__name__ == "Gemma2ForCausalLM" and attn.attn_logit_softcapping == 2.0 and attn.scaling == 0.125 and model.config.head_dim == D
    ids = torch.randint(0, 97, (1, 40), device="cuda", generator=torch.Generator("cuda").manual_seed(5))
    with torch.inference_mode():
        ref_logits = model(input_ids=ids).logits.float()
        ref_tokens = model.generate(ids, max_new_tokens=8, do_sample=False)[0, 40:].tolist()
        with _attn(model, attn_logit_softcapping=None):
            uncapped = model(input_ids=ids).logits.float()
        with _attn(model, scaling=D ** -0.5):
            rescaled = model(input_ids=ids).logits.float()
    moves = float((uncapped - ref_logits).abs().max()), float((rescaled - ref_logits).abs().max())
    print(f"[softcap] Gemma2 d{D}: removing the cap moves HF's eager logits by {moves[0]:.3f}, the standard scale by {moves[1]:.3f} (bar {BAR})")
    assert min(moves) >= 10 * BAR, moves      # the model is one the old seam would have computed wrongly (or refused)
    hf.patch_model(model)
    easykv_amd.enable_fixed_kv(model, _Tok(), mode="decoding", stride=1)
    cache = easykv_amd.BudgetedKVCache(2, 4, 2, D, 64, torch.device("cuda"), logit_cap=2.0, sm_scale=0.125)
    with torch.inference_mode(), cache.active(easykv_amd.StepPlan(policy="full", phase="prefill", accumulate=False)):
        got = model(input_ids=ids, past_key_values=cache, position_ids=torch.arange(40, device="cuda").view(1, -1), use_cache=True).logits.float()
    assert torch.allclose(got, ref_logits, atol=BAR, rtol=BAR), float((got - ref_logits).abs().max())
    # the module's arithmetic is held against the cache's: a cache without the cap, or with another scale, raises instead of computing another model
    for kw in (dict(sm_scale=0.125), dict(logit_cap=2.0), dict(logit_cap=50.0, sm_scale=0.125), dict(logit_cap=2.0, sm_scale=0.125 * 1.01)):
        wrong = easykv_amd.BudgetedKVCache(2, 4, 2, D, 64, torch.device("cuda"), **kw)
        with torch.inference_mode(), wrong.active(easykv_amd.StepPlan(policy="full", phase="prefill", accumulate=False)):
            with pytest.raises(ValueError, match="easykv_amd attention"):
                model(input_ids=ids, past_key_values=wrong, position_ids=torch.arange(40, device="cuda").view(1, -1), use_cache=True)
    with contextlib.redirect_stdout(io.StringIO()):
        out, cache = model.easykv_generate(input_ids=ids, generation_config=dict(temperature=1e-6, kv_policy="full", budget=200, max_new_tokens=8, eos_token_ids=[-1]),
                                           return_cache=True)
    assert [int(t) for t in out.split()] == ref_tokens
    assert cache.logit_cap == 2.0 and abs(cache.sm_scale - 0.125) < 1e-12      # read from the model's config by the driver
    # eviction: auto mode at half the prompt, stride 8
    ids2 = torch.randint(0, 97, (1, 120), device="cuda", generator=torch.Generator("cuda").manual_seed(6))
    gc = dict(budget=60, kv_policy="roco", max_new_tokens=6, recent_ratio=0.3, eos_token_ids=[-1], temperature=1e-6)
    easykv_amd.enable_fixed_kv(model, _Tok(), mode="auto", stride=8)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        out, cache = model.easykv_generate(input_ids=ids2, generation_config=gc, return_cache=True)
    bp, idx, _ = easykv_amd.geometry("auto", 120, 60, 8)
    assert len(out.split()) == 6 and cache.get_seq_length() == idx
    line = buf.getvalue().strip()
    assert line.startswith("KV Cache Budget ratio") and line.endswith(f"[{idx}/(120+6)]") and "\n" not in line, line
    for extra, match in ((dict(streaming=True), "streaming"), (dict(kv_quant="fp8"), "kv_quant"), (dict(long_rows=True), "long_rows")):
        with pytest.raises(ValueError, match=match):
            model.easykv_generate(input_ids=ids2, generation_config=dict(gc, **extra))
    with pytest.raises(ValueError, match="attn_logit_softcapping"):
        model.easykv_generate_batch(input_ids_list=[ids2, ids2], generation_config=gc)


def test_stock_gemma_with_a_free_scale_through_the_seam():
    """A GemmaForCausalLM-style uncapped model whose attention scale is not 1 / sqrt(head_dim) (query_pre_attn_scalar): before, the
    seam raised.  Its logits against its own eager attention, and the greedy tokens against the model's own eager forward run greedily
    (one full forward per token, no cache: HF's `generate` does not go through the replaced `scaling` attribute consistently — its step
    scores differ from the model's own forward on the same tokens by more than 2 here — so it is no reference for this model) — token
    by token for as long as the reference's top-2 logit gap exceeds twice the seam's logit bar (below that, two correct fp16 paths may
    pick either token, and the sequences part from there); at least the first three tokens are bound that way."""
    import easykv_amd
    import transformers
    from easykv_amd import hf
    D, qpas = 128, 144
    torch.manual_seed(1)
    cfg = transformers.GemmaConfig(vocab_size=97, hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=4,
                                   num_key_value_heads=2, head_dim=D, max_position_embeddings=512, attn_implementation="eager", initializer_range=0.25)
    model = transformers.GemmaForCausalLM(cfg).half().cuda().eval()
    model.config.query_pre_attn_scalar = qpas
    ids = torch.randint(0, 97, (1, 40), device="cuda", generator=torch.Generator("cuda").manual_seed(7))
    with torch.inference_mode(), _attn(model, scaling=qpas ** -0.5):
        ref_logits = model(input_ids=ids).logits.float()
        seq, ref_tokens, gaps = ids, [], []
        for _ in range(8):
            last = model(input_ids=seq).logits[0, -1].float()
            top2 = torch.topk(last, 2)
            ref_tokens.append(int(top2.indices[0]))
            gaps.append(float(top2.values[0] - top2.values[1]))
            seq = torch.cat([seq, top2.indices[:1].view(1, 1)], dim=1)
    with torch.inference_mode():
        standard = model(input_ids=ids).logits.float()
    assert float((standard - ref_logits).abs().max()) >= 10 * BAR
    for m in (l.self_attn for l in model.model.layers):
        m.scaling = qpas ** -0.5
    hf.patch_model(model)
    easykv_amd.enable_fixed_kv(model, _Tok(), mode="decoding", stride=1)
    plain = easykv_amd.BudgetedKVCache(2, 4, 2, D, 64, torch.device("cuda"))
    with torch.inference_mode(), plain.active(easykv_amd.StepPlan(policy="full", phase="prefill", accumulate=False)):
        with pytest.raises(ValueError, match="standard 1/sqrt"):      # a cache without a scale keeps the old check and the old message
            model(input_ids=ids, past_key_values=plain, position_ids=torch.arange(40, device="cuda").view(1, -1), use_cache=True)
    cache = easykv_amd.BudgetedKVCache(2, 4, 2, D, 64, torch.device("cuda"), sm_scale=qpas ** -0.5)
    with torch.inference_mode(), cache.active(easykv_amd.StepPlan(policy="full", phase="prefill", accumulate=False)):
        got = model(input_ids=ids, past_key_values=cache, position_ids=torch.arange(40, device="cuda").view(1, -1), use_cache=True).logits.float()
    assert torch.allclose(got, ref_logits, atol=BAR, rtol=BAR), float((got - ref_logits).abs().max())
    with contextlib.redirect_stdout(io.StringIO()):
        out, cache = model.easykv_generate(input_ids=ids, generation_config=dict(temperature=1e-6, kv_policy="full", budget=200, max_new_tokens=8, eos_token_ids=[-1]),
                                           return_cache=True)
    assert cache.logit_cap is None and abs(cache.sm_scale - qpas ** -0.5) < 1e-12      # read from the model's config by the driver
    toks, bound = [int(t) for t in out.split()], 0
    for t, r, gap in zip(toks, ref_tokens, gaps):
        if gap < 2 * BAR:
            break
        assert t == r, (bound, toks, ref_tokens, gaps)
        bound += 1
    print(f"[softcap] Gemma with query_pre_attn_scalar {qpas}: {bound} of 8 greedy tokens bound (the reference's top-2 gaps {[round(g, 3) for g in gaps]})")
    assert bound >= 3, (bound, gaps)
