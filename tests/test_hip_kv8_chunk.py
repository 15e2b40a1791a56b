"""Chunk steps on FP8 rows ("kv8 chunks", include/easykv_hip.h) on the GPU: KVBank(kv_quant='fp8', quant_chunks=True) /
quantize_fp8(chunks=True) against the CPU oracle in float64 ON THE BANK'S OWN CONTENTS — dequantised rows in position order, the step's
new rows quantised and dequantised by tests/kv8_ref.py — as tests/test_hip_kv8.py does for decode steps.  Outputs under
tests.golden_util.out_close; victims identical wherever the Probe of tests/test_hip_fullsize.py calls the decision stable and roco's
feasible set does not cut a tied class (tests/select_rule.py); the appended rows' codes and scales under kv8_ref.check_rows.  bf16
cases draw V at 1/4 scale, for the reason tests/test_hip_kv8.py gives: a bf16 output carries 2^-9 |o| of rounding of its own, which the
flat bar admits only below |o| = 0.5, so their V rows are clamped to |v| <= 0.24 — the K outlier row, the same for both types, puts a whole softmax on one key, and the
output is then that key's V row."""
import pytest
import torch

from tests import kv8_ref as R
from tests.golden_util import out_close
from tests.test_hip_d256 import _ProbeAndCapture
from tests.test_hip_kv8 import _NoCalls, _oracle_states

pytestmark = pytest.mark.gpu
BF, F16 = torch.bfloat16, torch.float16

SHAPES = [      # D, rep, q_len, T before the append, n_split: what it reaches
    (64, 1, 8, 40, 0),       # half a query tile, one partial key tile
    (128, 1, 16, 100, 0),    # crosses the 64-position super-tile
    (128, 4, 8, 130, 0),     # 32 folded rows, three tiles
    (128, 1, 40, 70, 0),     # two query blocks
    (128, 2, 8, 300, 2),     # key-range partials + fold
    (64, 8, 2, 65, 0),       # the GQA factor of gpt-oss / Mistral-like models
]


def _f64(st):
    for name in ("k", "v", "s", "q", "c"):
        if getattr(st, name) is not None:
            setattr(st, name, getattr(st, name).double())
    return st


def _exact_heads(hook, policy, ids, ids_ref, k1, sink, n):
    """The chunk-step victim rule: identical where the probe calls the decision stable and roco's feasible set cuts no tied class (any
    outcome must be a valid one).  Returns the heads that were compared exactly, and how many were checked at all (exactly or as valid)."""
    from oracle import easykv_oracle as O
    from tests.select_rule import feasible_classes, valid_victims
    got, ref = torch.sort(ids.cpu().long(), dim=-1)[0], torch.sort(ids_ref, dim=-1)[0]
    exact, n_checked = [], 0
    for h in range(got.shape[0]):
        if bool(hook.probe.last_unstable[h]):
            continue
        n_checked += 1
        if policy == "roco":
            c = hook.cap
            forced, pool, need = feasible_classes(O.roco_std(c.s, c.q, c.c, sink)[h], k1)
            assert valid_victims(got[h].tolist(), (c.s / c.c)[h], forced, pool, need, n), (h, got[h].tolist())
            if len(pool) != need:
                continue
        assert bool((got[h] == ref[h]).all()), (h, got[h].tolist(), ref[h].tolist())
        exact.append(h)
    return exact, n_checked


def _bank(D, rep, T, n, dtype, g, L=1, H=2):
    """A quantised bank of T rows per head: an outlier row and an all-zero row among them, the slot map scattered by three evictions."""
    from easykv_amd import KVBank
    vs = 0.25 if dtype is BF else 1.0
    k0, v0 = torch.randn(L, H, T + 3, D, generator=g), torch.randn(L, H, T + 3, D, generator=g) * vs
    if dtype is BF:      # (|o| stays below 0.25 whatever the softmax concentrates on: see the module docstring)
        v0.clamp_(-0.24, 0.24)
    k0[:, :, 5, 3], v0[:, :, 9, 1] = 300.0, (80.0 if dtype is F16 else 0.24)
    k0[:, :, 7], v0[:, :, 7] = 0.0, 0.0
    bank = KVBank(L, H * rep, H, D, cap=T + n + 16, dtype=dtype)
    bank.load_rows(k0.to(dtype).cuda(), v0.to(dtype).cuda())
    bank.compact_inplace(torch.tensor([2, 11, 30], dtype=torch.int32).expand(L, H, 3).contiguous())
    bank.state_init(T + n, 2, n)
    warm = torch.rand(L, H, T, generator=g) * 1e-3
    bank.score_sum[:, :, :T] += warm.cuda()
    bank.score_sq[:, :, :T] += (warm ** 2).cuda()
    return bank.quantize_fp8(chunks=True), vs


@pytest.mark.parametrize("policy", ["roco", "h2o_head", "tova", "full"])
@pytest.mark.parametrize("dtype", [F16, BF], ids=["fp16", "bf16"])
@pytest.mark.parametrize("D,rep,n,T,n_split", SHAPES, ids=[f"d{s[0]}-rep{s[1]}-n{s[2]}-T{s[3]}" for s in SHAPES])
def test_one_chunk_step_against_float64(D, rep, n, T, n_split, dtype, policy):
    from easykv_amd import StepPlan
    from oracle import easykv_oracle as O
    L, H = 1, 2
    # (rep 8: the plain seed's roco reference cuts a tied class in both heads; + 81 was picked on the CPU, on the rule's restatement of the bank)
    g = torch.Generator().manual_seed(1000 * D + 100 * rep + n + (dtype is BF) + (81 if rep == 8 else 0))
    bank, vs = _bank(D, rep, T, n, dtype, g)
    assert bank.k is None and bank.v is None and bank.n_slots == [T]
    scored = policy != "full"
    recent, sink = T // 10, 4
    kw = dict(policy=policy, phase="prefill", accumulate=scored, evict=scored, budget=T, recent=recent, sink=sink, stride=n, tova_head_mean=False)
    plan = StepPlan(n_split=n_split, **kw)
    info = bank.step_info(plan, n)
    assert info["n_launches"] > 0 and info["two_pass"] == 0 and info["wide"] == 0 and info["qb_rows"] * rep <= 32, info
    assert n_split == 0 or info["n_split"] == n_split, info
    q, k, v = torch.randn(L, H * rep, n, D, generator=g).to(dtype), torch.randn(L, H, n, D, generator=g).to(dtype), (torch.randn(L, H, n, D, generator=g) * vs).clamp_(-80 * vs, 0.96 * vs).to(dtype)
    k[:, :, n // 2], v[:, :, n // 2] = 0, 0      # an all-zero new row
    states = _oracle_states(bank, T + n, [0])
    new_rows = bank._slot_of_pos[0, :, T:T + n].cpu().long()      # the front of the free list
    out, ids = bank.attend(plan, q.cuda(), k.cuda(), v.cuda())
    assert out.dtype == dtype and bank.k is None and bank.n_slots == [T if scored else T + n]
    # the appended rows: quantised by the kernel as the rule says
    heads = torch.arange(H).unsqueeze(-1)
    for given, codes, sc in ((k[0], bank.k8[0], bank.k_scale[0]), (v[0], bank.v8[0], bank.v_scale[0])):
        R.check_rows(given, codes.cpu()[heads, new_rows], sc.cpu()[heads, new_rows], (D, rep, n, policy))
    # the reference, float64: new rows as the rule quantises them
    kq, vq = (R.dequant(*R.quantize(x)).double() for x in (k, v))
    hook = _ProbeAndCapture()
    O.SELECT_HOOK = hook
    try:
        o_ref, ids_ref = O.layer_step(_f64(states[0]), q.double(), kq, vq, O.StepPlan(**kw))
    finally:
        O.SELECT_HOOK = None
    err = float((out[0].double().cpu() - o_ref[0]).abs().max())
    print(f"[kv8-chunk] d{D} rep{rep} n{n} T{T} {dtype} {policy}: max |out - ref| = {err:.3e}")
    assert out_close(out[0].float().cpu(), o_ref[0].float()), err
    if not scored:
        return
    exact, n_checked = _exact_heads(hook, policy, ids[0], ids_ref, max(T - recent - sink, n), sink, n)
    assert exact, "no head of this case was compared exactly: pick another seed"
    for h in exact:      # the score rows the exported logits were accumulated into, after the same compaction
        for got, ref in ((bank.score_sum, states[0].s), (bank.score_sq, states[0].q)):
            assert torch.allclose(got[0, h, :T].cpu().double(), ref[h, :T], rtol=1e-3, atol=1e-5), h


@pytest.mark.parametrize("policy", ["h2o_head", "roco"])
def test_q_len_1_of_the_chunk_family_is_the_decode_step(policy):
    """A q_len = 1 call of the chunk family and ekv_kv8_step_attend on twin banks: outputs, victims and score rows equal, no tolerance."""
    from easykv_amd import StepPlan
    D, rep, T = 128, 2, 200
    got = []
    for chunks in (True, False):
        g = torch.Generator().manual_seed(7)
        bank, _ = _bank(D, rep, T, 1, F16, g)
        if not chunks:
            bank.quant_chunks = False
            bank._attach(bank._fmt, bank._desc)
        assert (bank._attend_fn.__name__ == "ekv_kv8_chunk_step_attend") == chunks
        plan = StepPlan(policy=policy, phase="decode", evict=True, budget=T)
        q, k, v = (torch.randn(1, hh, 1, D, generator=g).half().cuda() for hh in (2 * rep, 2, 2))
        out, ids = bank.attend(plan, q, k, v)
        got.append((out.cpu(), ids.cpu(), bank.score_sum.cpu(), bank.k_scale.cpu()))
    for a, b in zip(*got):
        assert torch.equal(a, b)


@pytest.mark.parametrize("D,rep", [(128, 1), (64, 4)])
def test_chunk_logits_against_decode_logits(D, rep):
    """The logits a chunk step exports for its last query against those a split decode step exports for the SAME query on the same bank,
    over the rows both touched.  Both are fp32 sums of the same exact products q_d * code_d in different orders, times the same k_scale,
    divided by the same sm_div.  Rounding errors of an n-term fp32 sum stay below lambda sqrt(n) u sum|x_i| with probability
    1 - 2 exp(-lambda^2 / 2) (Higham & Mary 2019; u = 2^-24): lambda = 6 for each sum leaves < 1e-3 over the ~2000 logits here.  Plus
    one ulp of the logit for each of the two roundings behind the sum."""
    from easykv_amd import StepPlan
    T, n, H = 130, 8, 2
    g = torch.Generator().manual_seed(11 + D)
    bank, _ = _bank(D, rep, T, n, F16, g)
    q, k, v = (torch.randn(1, hh, n, D, generator=g).half().cuda() for hh in (H * rep, H, H))
    bank.attend(StepPlan(policy="h2o_head", phase="prefill", accumulate=True, evict=False, stride=n), q, k, v)
    Tn, pad = T + n, lambda t: (t + 63) // 64 * 64
    chunk = bank._ws[:H * rep * n * pad(Tn) * 4].view(torch.float32).view(H * rep, n, pad(Tn))[:, n - 1, :Tn].clone()
    plan = StepPlan(policy="h2o_head", phase="decode", accumulate=True, evict=False, n_split=2)
    assert bank.step_info(plan, 1)["n_split"] == 2 and not bank.step_info(plan, 1)["fused"]
    bank.attend(plan, q[:, :, n - 1:], k[:, :, :1], v[:, :, :1])
    dec = bank._ws[:H * rep * pad(Tn + 1) * 4].view(torch.float32).view(H * rep, pad(Tn + 1))[:, :Tn]
    kd = bank.dequantized_rows(0)[0].double()      # [H, cap, D] = code * k_scale, by physical row
    rows = torch.gather(kd, 1, bank.slot_of_pos[0, :, :Tn].long().unsqueeze(-1).expand(-1, -1, D)).repeat_interleave(rep, 0)
    mag = (q[0, :, n - 1].double().unsqueeze(1).abs() * rows.abs()).sum(-1) / D ** 0.5
    bound = 2 * 6 * (D - 1) ** 0.5 * 2.0 ** -24 * mag + 2 * 2.0 ** -23 * chunk.double().abs()
    diff = (chunk.double() - dec.double()).abs()
    print(f"[kv8-chunk-logits] D={D} rep={rep}: max |chunk - decode| = {float(diff.max()):.3e}, equal bits in {float((diff == 0).double().mean()):.3f} of the logits")
    assert bool((diff <= bound).all()), float((diff / bound.clamp_min(1e-30)).max())


def test_lockstep_from_an_empty_fp8_bank():
    """Dense prefix (r_idx 48), 6 evicting chunk steps at stride 8, 8 decode steps on a bank created quantised: the oracle is re-seeded
    from the bank's dequantised contents before every step; the bank never holds a 16-bit tensor."""
    from easykv_amd import KVBank, StepPlan
    from oracle import easykv_oracle as O
    L, H, rep, D, r, s = 2, 2, 2, 128, 48, 8
    g = torch.Generator().manual_seed(3)
    bank = KVBank(L, H * rep, H, D, cap=r + s + 8, kv_quant="fp8", quant_chunks=True)
    steps = [(r, dict(policy="roco", phase="prefill", accumulate=False, evict=False))]
    steps += [(s, dict(policy="roco", phase="prefill", accumulate=True, evict=True, budget=r, recent=4, sink=4, stride=s))] * 6
    steps += [(1, dict(policy="roco", phase="decode", evict=True, budget=r))] * 8
    hook = _ProbeAndCapture()
    n_checked = 0
    for i, (n, kw) in enumerate(steps):
        T = bank.n_slots[0]
        if i == 1:
            bank.state_init(r + s, 2, s)
        if i == 7:
            bank.state_init(r + 1, 0)
        q, k, v = (torch.randn(L, hh, n, D, generator=g).half() for hh in (H * rep, H, H))
        states = _oracle_states(bank, T + n, range(L)) if T else None
        out, ids = bank.attend(StepPlan(**kw), q.cuda(), k.cuda(), v.cuda())
        assert bank.k is None and bank.v is None
        kq, vq = (R.dequant(*R.quantize(x)) for x in (k, v))
        for l in range(L):
            st = states[l] if states else O.LayerState(k=torch.zeros(1, H, 0, D), v=torch.zeros(1, H, 0, D))
            O.SELECT_HOOK = hook
            try:
                o_ref, ids_ref = O.layer_step(st, q[l:l + 1].float(), kq[l:l + 1], vq[l:l + 1], O.StepPlan(**kw))
            finally:
                O.SELECT_HOOK = None
            assert out_close(out[l].float().cpu(), o_ref[0]), (i, l, float((out[l].float().cpu() - o_ref[0]).abs().max()))
            if ids_ref is None:
                continue
            if n > 1:
                n_checked += _exact_heads(hook, "roco", ids[l], ids_ref, max(r - 4 - 4, s), 4, s)[1]
            else:
                ok = ~hook.probe.last_unstable
                assert bool((ids[l, :, 0].cpu().long() == ids_ref[:, 0])[ok].all()), (i, l)
                n_checked += int(ok.sum())
    assert bank.n_slots == [r] * L and n_checked >= 0.8 * (6 + 8) * L * H, n_checked


def test_surface():
    from easykv_amd import KVBank, StepPlan
    from easykv_amd._lib import EkvError
    with pytest.raises(ValueError, match="quant_chunks"):
        KVBank(1, 2, 2, 64, cap=64, kv_quant="mxfp4", quant_chunks=True)
    bank = KVBank(1, 2, 2, 64, cap=64, kv_quant="fp8", quant_chunks=True)
    q = torch.randn(1, 2, 8, 64).half().cuda()
    lib, bank.lib = bank.lib, _NoCalls()
    for call, what in ((lambda: bank.load_rows(q, q), "load_rows"), (lambda: bank.ordered_kv(), "row move")):
        with pytest.raises(EkvError, match=what):
            call()
    bank.lib = lib
    plain = KVBank(1, 2, 2, 64, cap=64, kv_quant="fp8")      # without the flag: "chunk step", as always
    with pytest.raises(EkvError, match="chunk step"):
        plain.attend(StepPlan(policy="full", phase="prefill", accumulate=False), q, q, q)


class _Tok:
    eos_token_id = -1

    def decode(self, ids, skip_special_tokens=True):
        return " ".join(str(i) for i in ids)


# |ln ppl_fp8 - ln ppl_16bit| of the tiny llama below, 160 tokens, roco, budget 0.5, stride 8, measured on an MI355X (16-bit, FP8) per seed:
PPL_PAIRS = {0: (102.2503, 102.0198, 0.002257), 1: (98.2683, 98.3760, 0.001096), 2: (100.3983, 100.3927, 0.000055)}
PPL_BAR = 2 * 0.002257      # twice the largest difference above


def test_generation_config_kv_quant_prefill(monkeypatch):
    import contextlib
    import io
    import math

    import easykv_amd
    from easykv_amd import engine, hf
    from tests.test_hip_bf16 import _tiny
    model = hf.patch_model(_tiny("llama"))
    gen = dict(temperature=1e-6, kv_policy="roco", budget=0.5, max_new_tokens=6, eos_token_ids=[-1], kv_dtype="auto")
    fp8 = dict(kv_quant="fp8", kv_quant_prefill=True)

    def run(mode, ids, **extra):
        easykv_amd.enable_fixed_kv(model, _Tok(), mode=mode, stride=8)
        torch.manual_seed(11)
        with contextlib.redirect_stdout(io.StringIO()):
            call = model.easykv_ppl if mode == "ppl" else model.easykv_generate
            return call(input_ids=ids, generation_config=dict(gen, **extra), **({} if mode == "ppl" else dict(return_cache=True)))

    for seed in PPL_PAIRS:
        ids = torch.randint(0, 97, (1, 160), device="cuda", generator=torch.Generator(device="cuda").manual_seed(seed))
        p16, p8 = run("ppl", ids), run("ppl", ids, **fp8)
        print(f"[kv8-chunk-ppl] seed {seed}: ppl 16-bit {p16!r}, FP8 {p8!r}, |ln ratio| = {abs(math.log(p8 / p16)):.6f}")
        assert math.isfinite(p8) and abs(math.log(p8 / p16)) <= PPL_BAR, (seed, p16, p8)
    ids = torch.randint(0, 97, (1, 72), device="cuda", generator=torch.Generator(device="cuda").manual_seed(3))
    for mode, extra in (("encoding", dict(keep_attention=True)), ("auto", dict(budget=24, dense_growth=True))):
        text, cache = run(mode, ids, _record_evictions=True, **fp8, **extra)
        assert len(text.split()) == 6 and cache.kv_quant == "fp8" and cache.bank.k is None and cache.bank.quant_chunks
        text_g, cache_g = run(mode, ids, _record_evictions=True, hipgraph=True, **fp8, **extra)
        assert text_g == text and len(cache.evictions) == len(cache_g.evictions) > 0
        assert all(torch.equal(x, y) for a, b in zip(cache.evictions, cache_g.evictions) for x, y in zip(a, b)), mode
    with contextlib.redirect_stdout(io.StringIO()):      # every prompt prefills in an FP8 bank and is adopted into the FP8 batch
        texts = model.easykv_generate_batch(input_ids_list=[ids[0], ids[0, :50]], generation_config=dict(gen, budget=24, **fp8))      # ('auto' mode, as enabled last)
    assert len(texts) == 2 and all(len(t.split()) == 6 for t in texts)
    # refusals: before any bank exists and before any library call (the _NoCalls pattern: the library handle and the bank's constructor)
    def no_bank(*a, **k):
        raise AssertionError("a bank was created after a refusal")
    monkeypatch.setattr(engine._lib, "load", lambda: _NoCalls())
    monkeypatch.setattr(engine.KVBank, "__init__", no_bank)
    easykv_amd.enable_fixed_kv(model, _Tok(), mode="encoding", stride=8)
    bad = [dict(kv_quant=None), dict(kv_quant="mxfp6"), dict(streaming=True, kv_dtype="float16"), dict(long_rows=True), dict(prefill="one_shot"),
           dict(sliding_window=[16, 16]), dict(attention_sinks=torch.zeros(2, 4))]
    for extra in bad:
        with pytest.raises(ValueError, match="kv_quant_prefill"):
            model.easykv_generate(input_ids=ids, generation_config=dict(gen, **dict(fp8, **extra)))
    monkeypatch.setattr(model.config, "num_attention_heads", 66)      # (a GQA factor of 33: more than a block of a chunk step on FP8 rows)
    with pytest.raises(ValueError, match="kv_quant_prefill.*GQA factor"):
        model.easykv_generate(input_ids=ids, generation_config=dict(gen, **fp8))
    monkeypatch.setattr(model.config, "num_attention_heads", 4)
    monkeypatch.setattr(model.config, "attn_logit_softcapping", 30.0, raising=False)
    with pytest.raises(ValueError, match="kv_quant_prefill"):
        model.easykv_generate(input_ids=ids, generation_config=dict(gen, **fp8))
    monkeypatch.delattr(model.config, "attn_logit_softcapping")

    class Shard:
        world, rank, begin, count = 2, 0, 0, 1
    monkeypatch.setattr(model, "layer_shard", Shard(), raising=False)
    with pytest.raises(ValueError, match="kv_quant_prefill"):
        model.easykv_generate(input_ids=ids, generation_config=dict(gen, **fp8))
