"""easykv_amd.generate_batch end to end: prompts of different lengths prefilled alone, decoded in ONE forward per token.

  * on the reference's goldens (a batched fake model, tests/batch_fake_model.py): each batch takes one golden's streams and config
    and runs its prompt next to longer prompts over the same streams.  Sequence 0 must reproduce the golden of the real reference
    (every evicted id, text, printed line); every other sequence must equal the oracle's run on that prompt and its own solo
    ``easykv_amd.generate`` run (ids, text, printed line, attention outputs of every forward);
  * an EOS case: sequences stop where their solo runs stop, and the survivors are unaffected;
  * the HF seam on tiny Llama / Mistral models: one batched attend per layer and decode forward, tokens equal to the solo runs up to
    the logit-gap bar;
  * the refusals of generate_batch come before any bank exists."""
import contextlib
import io

import numpy as np
import pytest
import torch

from tests.golden_util import load_golden, out_close, split_ids, trace_events

pytestmark = pytest.mark.gpu


def _evictions(ev):
    return [np.sort(torch.stack(e).cpu().numpy(), axis=-1) for e in ev]


def _ids(length):
    return torch.arange(length).view(1, -1) % 16


def _run_batch(streams, cfg, mode, stride, lengths, vocab=16, arch="LlamaForCausalLM"):
    import easykv_amd
    from tests.batch_fake_model import BatchFakeModel
    model = BatchFakeModel(*streams, arch=arch, vocab=vocab)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        res, cache = easykv_amd.generate_batch(model, [_ids(n) for n in lengths], cfg, kv_mode=mode, stride=stride, return_cache=True)
    return model, res, cache, buf.getvalue().strip().split("\n")


def _run_solo(streams, cfg, mode, stride, length, vocab=16, arch="LlamaForCausalLM"):
    import easykv_amd
    from tests.native_fake_model import NativeFakeModel
    model = NativeFakeModel(*streams, arch=arch, vocab=vocab)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        res, cache = easykv_amd.generate(model, _ids(length), cfg, kv_mode=mode, stride=stride, return_cache=True)
    return model, res, cache, buf.getvalue().strip()


def _run_oracle(streams, cfg, mode, stride, length, vocab=16, arch="LlamaForCausalLM"):
    from oracle import easykv_oracle as O
    from oracle.fake_model import FakeAttnModel
    model = FakeAttnModel(*streams, arch=arch, vocab=vocab)
    return O.generate(model, _ids(length), {k: v for k, v in cfg.items() if not k.startswith("_")}, kv_mode=mode, stride=stride)


def _check_batch(streams, cfg, mode, stride, lengths, golden=None, vocab=16):
    """Every sequence of the batch against its solo run and the oracle; sequence 0 against `golden` when given."""
    cfg = dict(cfg, _record_evictions=True)
    model, res, cache, lines = _run_batch(streams, cfg, mode, stride, lengths, vocab)
    assert len(res) == len(lines) == len(lengths), (res, lines)
    n_sel = []
    for i, n in enumerate(lengths):
        smodel, sres, scache, sline = _run_solo(streams, cfg, mode, stride, n, vocab)
        assert res[i] == sres and lines[i] == sline, (i, n, res[i], sres, lines[i], sline)
        ours, solo = _evictions(cache.evictions[i]), _evictions(scache.evictions)
        assert len(ours) == len(solo) and all(np.array_equal(a, b) for a, b in zip(ours, solo)), (i, n, len(ours), len(solo))
        assert len(model.logs[i]) == len(smodel.outputs_log), (i, len(model.logs[i]), len(smodel.outputs_log))
        for f, (a, b) in enumerate(zip(model.logs[i], smodel.outputs_log)):
            assert a.shape == b.shape and out_close(a, b, 1e-3), (i, f, float((a - b).abs().max()))
        # the oracle's own run on this prompt
        tr = _run_oracle(streams, cfg, mode, stride, n, vocab)
        kinds, ph, rg = trace_events(tr)
        ref = []
        for kind in kinds:
            if kind == 0:
                ref.append(ph.pop(0))
            else:
                lo, hi = rg.pop(0)
                ref.append(np.broadcast_to(np.arange(lo, hi, dtype=np.int32), ours[len(ref)].shape))
        assert len(ours) == len(ref) and all(np.array_equal(a, b) for a, b in zip(ours, ref)), (i, n, "oracle")
        ref_text = tr.result if isinstance(tr.result, str) else " ".join(str(t) for t in tr.result)      # (the oracle keeps the ids)
        assert res[i] == ref_text and lines[i] == tr.report.strip(), (i, res[i], ref_text, lines[i], tr.report)
        n_sel.append(len(ours))
    if golden is not None:      # sequence 0 IS the golden's prompt: the real reference's ids, text and printed line
        m = golden["meta"]
        assert lengths[0] == m["length"] and res[0] == m["result"] and lines[0] == m["printed"]
        ours = _evictions(cache.evictions[0])
        ref_ph, ref_rg, ref = split_ids(golden), golden["ranges"].tolist(), []
        for kind in golden["kinds"]:
            if kind == 0:
                ref.append(ref_ph.pop(0))
            else:
                lo, hi = ref_rg.pop(0)
                ref.append(np.broadcast_to(np.arange(lo, hi, dtype=np.int32), ours[len(ref)].shape))
        assert len(ours) == len(ref) and all(np.array_equal(a, b) for a, b in zip(ours, ref))
    return model, cache, n_sel


GOLDEN_BATCHES = [("dec_roco", (16, 19, 22, 24)), ("dec_h2o_head", (16, 19, 22, 24)), ("dec_tova", (16, 19, 22, 24)),
                  ("dec_roco_gqa", (16, 19, 22, 24)), ("dec_recency", (16, 19, 22, 24)), ("dec_roco_d128", (8, 11, 13, 15, 16)),
                  ("auto_to_decoding", (20, 24, 28)), ("auto_roco_s4", (96, 100, 104))]


@pytest.mark.parametrize("name,lengths", GOLDEN_BATCHES, ids=[c[0] for c in GOLDEN_BATCHES])
def test_batch_on_the_goldens(name, lengths):
    g = load_golden(name)
    m = g["meta"]
    model, cache, n_sel = _check_batch(g["streams"], m["config"], m["mode"], m["stride"], lengths, golden=g, vocab=m.get("vocab", 16))
    # one forward per token for all sequences: every decode forward was a batched one, with one attend per layer
    assert model.n_batched_forwards == m["config"]["max_new_tokens"]
    assert cache.bat.n_calls == model.n_batched_forwards * model.config.num_hidden_layers
    print(f"[batch-golden] {name} lengths {lengths}: selections per sequence {n_sel}")


def test_batch_of_eight_lengths_in_one_launch():
    """T from 17 to 350 in one launch: eight prompts over seeded streams, the config of dec_roco."""
    from oracle.fake_model import make_streams
    cfg = load_golden("dec_roco")["meta"]["config"]
    lengths = (16, 33, 48, 64, 97, 130, 200, 260)
    _check_batch(make_streams(2, 4, 4, 32, 400, seed=11), cfg, "decoding", 1, lengths)


def test_batch_eos_retires_sequences_where_their_solo_runs_stop():
    g = load_golden("dec_roco_eos_mid")
    m = g["meta"]
    cfg = dict(m["config"], eos_token_ids=m["eos_token_ids"])
    lengths = (16, 19, 22, 24)
    model, cache, _ = _check_batch(g["streams"], cfg, m["mode"], m["stride"], lengths, golden=g, vocab=m["vocab"])
    # sequence 0 took the golden's forwards (its prefill + 57 decode steps); the others stopped at different steps, as alone
    assert len(model.logs[0]) == m["n_forwards"] == 58
    assert len({len(l) for l in model.logs}) > 1


class _Tok:
    eos_token_id = -1

    def decode(self, ids, skip_special_tokens=True):
        return " ".join(str(i) for i in ids)


@pytest.mark.parametrize("kv_dtype", ["auto", None])
@pytest.mark.parametrize("kind", ["llama", "mistral"])
def test_hf_seam_batched_decode(kind, kv_dtype, monkeypatch):
    """Three prompts of different lengths on a tiny HF model, greedy: one batched attend per layer and decode forward, and each
    sequence's tokens equal its solo run's for every step before the first one at which the SOLO run's top-2 logit gap is smaller
    than 8 x the largest |batched - solo| logit difference seen so far (a batched GEMM and a one-row GEMM round differently: the bar
    is about the model's matmuls, not the attention path).  At least the first 8 tokens of every sequence are bound.
    Observed (model seed 0, prompt seed 3; Llama and Mistral, kv_dtype 'auto' and default, three sequences each): the largest
    |batched - solo| logit difference is 0 in all twelve runs — at hidden size 256 the [3, 256] and [1, 256] GEMMs round alike — so all
    24 of 24 tokens of every sequence are bound.  The test prints both figures per sequence ([hf-batch] lines)."""
    import easykv_amd
    from easykv_amd import api, engine, hf
    from tests.test_hip_bf16 import _tiny
    model = hf.patch_model(_tiny(kind, seed=0))
    easykv_amd.enable_fixed_kv(model, _Tok(), mode="decoding", stride=1)
    g = torch.Generator().manual_seed(3)
    prompts = [torch.randint(0, 97, (1, n), generator=g).cuda() for n in (20, 33, 41)]
    gen = dict(kv_policy="roco", budget=16, max_new_tokens=24, eos_token_ids=[-1], temperature=1.0, top_p=1e-6)
    if kv_dtype is not None:
        gen["kv_dtype"] = kv_dtype
    seen = []
    orig = api.logits_adapter
    monkeypatch.setattr(api, "logits_adapter", lambda logits, t, p: (seen.append(logits.clone()), orig(logits, t, p))[1])
    solo_tok, solo_logits = [], []
    for p in prompts:
        seen.clear()
        with contextlib.redirect_stdout(io.StringIO()):
            solo_tok.append([int(x) for x in model.easykv_generate(input_ids=p, generation_config=gen).split()])
        solo_logits.append([x[0] for x in seen])
    seen.clear()
    calls = []
    orig_attend = engine.KVBankBatch.attend
    monkeypatch.setattr(engine.KVBankBatch, "attend", lambda self, *a, **k: (calls.append(a[4]), orig_attend(self, *a, **k))[1])
    with contextlib.redirect_stdout(io.StringIO()):
        res = model.easykv_generate_batch(input_ids_list=prompts, generation_config=gen)
    n_layers = model.config.num_hidden_layers
    assert calls == [l for _ in range(gen["max_new_tokens"]) for l in range(n_layers)]      # one batched attend per layer and forward
    batch_logits = list(seen)      # (the prefills sample nothing: one [B', vocab] block per decode step)
    assert len(batch_logits) == gen["max_new_tokens"]
    for i in range(len(prompts)):
        toks = [int(x) for x in res[i].split()]
        worst, bound = 0.0, 0
        for step in range(gen["max_new_tokens"]):
            a, b = batch_logits[step][i].float(), solo_logits[i][step].float()
            top2 = torch.topk(b, 2).values
            gap = float(top2[0] - top2[1])
            if toks[:step] != solo_tok[i][:step]:
                break
            worst = max(worst, float((a - b).abs().max()))
            if gap < 8 * worst:
                break
            assert toks[step] == solo_tok[i][step], (kind, i, step, gap, worst)
            bound += 1
        print(f"[hf-batch] {kind} kv_dtype={kv_dtype} sequence {i}: {bound} tokens bound, largest |batched - solo| logit difference {worst:.4g}")
        assert bound >= 8, (kind, i, bound, worst)


def test_generate_batch_refusals_come_before_any_bank(monkeypatch):
    import easykv_amd
    from easykv_amd import engine
    from tests.batch_fake_model import BatchFakeModel
    from oracle.fake_model import make_streams
    made = []
    monkeypatch.setattr(engine.KVBank, "__init__", lambda self, *a, **k: made.append(1))
    model = BatchFakeModel(*make_streams(2, 4, 4, 32, 64, seed=1))
    easykv_amd.enable_fixed_kv(model, model.tokenizer, mode="decoding", stride=1)
    ids = [_ids(16), _ids(20)]
    gen = dict(kv_policy="roco", budget=8, max_new_tokens=4)
    for extra, match in ((dict(streaming=True), "streaming"), (dict(kv_quant="fp8"), "kv_quant"), (dict(hipgraph=True), "hipgraph")):
        with pytest.raises(ValueError, match=match):
            model.easykv_generate_batch(input_ids_list=ids, generation_config=dict(gen, **extra))
    with pytest.raises(ValueError, match="ppl"):
        easykv_amd.generate_batch(model, ids, gen, kv_mode="ppl")
    with pytest.raises(ValueError, match="prompts"):
        model.easykv_generate_batch(input_ids_list=[], generation_config=gen)
    with pytest.raises(ValueError, match="prompts"):
        model.easykv_generate_batch(input_ids_list=[torch.zeros(2, 8, dtype=torch.long)], generation_config=gen)

    class Shard:
        world, rank, begin, count = 2, 0, 0, 1
    model.layer_shard = Shard()
    with pytest.raises(ValueError, match="layer-sharded"):
        model.easykv_generate_batch(input_ids_list=ids, generation_config=gen)
    assert made == []
    # the single-sequence contract one level down is unchanged
    with pytest.raises(ValueError, match="batch"):
        easykv_amd.generate(model, torch.zeros(2, 8, dtype=torch.long), gen, kv_mode="decoding")
