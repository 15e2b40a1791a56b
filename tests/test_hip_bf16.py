"""bf16 K/V banks (KVBank(dtype=torch.bfloat16), include/easykv_hip.h EKV_DTYPE_BF16): every plain-key path the planner picks runs
its bf16 kernel instance, against the fp32 oracle on .float() of the same bf16 values.

Victims equal the oracle's wherever tests.test_hip_lockstep.Hook calls the decision well defined, and are one of the oracle's own
answers under a +-2e-5 perturbation elsewhere.  Outputs satisfy |o - ref| <= 2^-8 (|ref| + pv) + 1e-6 pv with pv = p.|V| (the fp32
probability row times |V|): P is rounded to bf16 where it feeds a PV MFMA (<= 2^-9 relative per term) and the output is rounded once
(<= 2^-8 |o|).  The largest |o - ref| / pv seen is printed as [bf16-bar]."""
import contextlib
import ctypes as C
import io
import math

import pytest
import torch

from tests.test_hip_lockstep import Hook

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
WORST = [0.0]


def _pv(q, k_all, v_all, t_prev):
    """p.|V| of the oracle's fp32 probabilities: q [Hq, n, D], k_all / v_all [H, T, D] (float), causal inside the chunk."""
    hq, n, d = q.shape
    rep = hq // k_all.shape[0]
    k, v = k_all.repeat_interleave(rep, 0), v_all.repeat_interleave(rep, 0)
    s = q @ k.transpose(1, 2) / math.sqrt(d)
    T = k.shape[1]
    mask = torch.arange(T)[None, :] > (t_prev + torch.arange(n))[:, None]
    s = s.masked_fill(mask, float("-inf"))
    return torch.softmax(s, dim=-1) @ v.abs()


def _check_out(out, ref, pv, what):
    out, ref = out.float().cpu(), ref.float().cpu()
    err = (out - ref).abs()
    bar = 2.0 ** -8 * (ref.abs() + pv) + 1e-6 * pv
    assert torch.isfinite(out).all(), what
    assert bool((err <= bar).all()), (what, float((err - bar).max()), float(err.max()))
    WORST[0] = max(WORST[0], float((err / pv.clamp_min(1e-30)).max()))


def _check_ids(hook, got, ref, what):
    """got / ref [H, k]: equal, or in the oracle's tolerance class where they differ.  Returns the heads that differed."""
    got, ref = torch.sort(got.long(), -1)[0], torch.sort(ref.long(), -1)[0]
    bad = (got != ref).any(-1).nonzero().flatten().tolist()
    for h in bad:
        assert hook.in_tolerance_class(h, got[h]), (what, h, bool(hook.last["unstable"][h]))
    return bad


def _seed(bank, W):
    from oracle import easykv_oracle as O
    kk, vv = bank.ordered_kv()
    S, Q, Cn = bank.score_sum.cpu(), bank.score_sq.cpu(), bank.score_cnt.cpu()
    out = []
    for l in range(bank.n_layers):
        st = O.LayerState(k=kk[l:l + 1].float().cpu(), v=vv[l:l + 1].float().cpu())
        st.s, st.q, st.c = S[l, :, :W].clone(), Q[l, :, :W].clone(), Cn[l, :, :W].clone()
        out.append(st)
    return out


@pytest.fixture(autouse=True, scope="module")
def _report():
    yield
    print(f"[bf16-bar] largest |o - ref| / (p.|V|) over the bf16 steps: {WORST[0]:.3e} (bar 2^-8 = {2 ** -8:.3e})")


# ---- (a) decode ---------------------------------------------------------------------------------------------------------------
DECODE = [
    # name, L, hq, h, D, budget, policy, n_split, defer, expect (fused, slot rows, n_split > 1)
    ("fused 32 layers roco", 32, 8, 8, 128, 48, "roco", 0, False, (1, True, False)),
    ("fused 4 layers n_split=1 h2o GQA4", 4, 16, 4, 64, 48, "h2o_head", 1, False, (1, False, False)),
    ("split + fold tova GQA3 d96", 2, 24, 8, 96, 600, "tova", 4, False, (0, False, True)),
    ("deferred roco GQA8 d32", 4, 16, 2, 32, 48, "roco", 0, True, (0, False, False)),
    ("recency GQA1 d64", 2, 8, 8, 64, 48, "recency", 0, False, (1, False, False)),
]


@pytest.mark.parametrize("name,L,hq,h,D,budget,policy,n_split,defer,expect", DECODE, ids=[c[0] for c in DECODE])
def test_decode_against_the_oracle(name, L, hq, h, D, budget, policy, n_split, defer, expect):
    from easykv_amd import KVBank, StepPlan
    from oracle import easykv_oracle as O
    steps = 40
    T = budget + 1
    g = torch.Generator().manual_seed(L * 1000 + hq + D)
    bank = KVBank(L, hq, h, D, cap=T + 8, dtype=BF)
    bank.load_rows(torch.randn(L, h, budget, D, generator=g).to(BF).cuda(), torch.randn(L, h, budget, D, generator=g).to(BF).cuda())
    bank.state_init(T, 0)
    warm = torch.rand(L, h, budget, generator=g) * 1e-3
    bank.score_sum[:, :, :budget] += warm.cuda()
    bank.score_sq[:, :, :budget] += (warm ** 2).cuda()
    states = _seed(bank, T)
    rs = 4 if policy == "recency" else -1
    plan = StepPlan(policy=policy, phase="decode", evict=True, score_off=0, budget=budget, n_split=n_split, range_start=rs)
    oplan = O.StepPlan(policy=policy, phase="decode", evict=True, score_off=0, budget=budget, range_start=rs)
    info = bank.step_info(plan, 1, 0, 1 if defer else L, phases=5 if defer else 0)
    assert info["fused"] == expect[0] and (info["n_split"] > 1) == expect[2], info
    hook = Hook()
    O.SELECT_HOOK = hook
    n_slot = 0
    try:
        for i in range(steps):
            q, k, v = torch.randn(L, hq, 1, D, generator=g).to(BF), torch.randn(L, h, 1, D, generator=g).to(BF), torch.randn(L, h, 1, D, generator=g).to(BF)
            if defer:
                outs = [bank.attend(plan, q[l:l + 1].cuda(), k[l:l + 1].cuda(), v[l:l + 1].cuda(), layer_begin=l, defer=True)[0] for l in range(L)]
                ids = bank.flush()
                out = torch.cat(outs)
            else:
                out, ids = bank.attend(plan, q.cuda(), k.cuda(), v.cuda())
                n_slot += int(all(bank._slot_rows))
            assert out.dtype == BF
            reseed = []
            for l in range(L):
                st = states[l]
                k_all, v_all = torch.cat([st.k[0], k[l].float()], 1), torch.cat([st.v[0], v[l].float()], 1)
                pv = _pv(q[l].float(), k_all, v_all, k_all.shape[1] - 1)
                o_ref, ids_ref = O.layer_step(st, q[l:l + 1].float(), k[l:l + 1].float(), v[l:l + 1].float(), oplan)
                _check_out(out[l], o_ref[0], pv, (name, i, l))
                if policy != "recency" and _check_ids(hook, ids[l].cpu(), ids_ref.view(h, -1), (name, i, l)):
                    reseed.append(l)
                elif policy == "recency":
                    assert (ids[l].cpu().long() == rs).all()
            if reseed:
                fresh = _seed(bank, T)
                for l in set(reseed):
                    states[l] = fresh[l]
                    states[l].s, states[l].q, states[l].c = states[l].s[:, :T], states[l].q[:, :T], states[l].c[:, :T]
                bank._slot_short = 0
    finally:
        O.SELECT_HOOK = None
    if expect[1]:
        assert n_slot >= steps // 2, n_slot      # the one-launch step on the slot-indexed score rows


# ---- (b) chunk steps ----------------------------------------------------------------------------------------------------------
CHUNK = [
    # name, L, hq, h, D, t_prev (idx), stride, policy, two_pass, expect: dict of step_info fields
    ("logits-in-LDS stride 8", 2, 8, 8, 128, 504, 8, "roco", 0, dict(fused=1, wide=0, two_pass=0)),
    ("16x16 one pass d96", 2, 8, 8, 96, 496, 16, "roco", -1, dict(wide=0, two_pass=0)),
    ("16x16 two pass d96", 2, 8, 8, 96, 480, 48, "h2o_head", 1, dict(wide=0, two_pass=1)),
    ("wide two pass 96 rows", 2, 8, 8, 128, 576, 96, "roco", 0, dict(wide=1, two_pass=1)),
    ("resident short GQA4", 2, 8, 2, 128, 1232, 16, "roco", 0, dict(fused=1, wide=1, two_pass=1, n_launches=1)),
    ("resident LONG stride 8", 2, 8, 2, 128, 2056, 8, "roco", 0, dict(fused=1, wide=1, two_pass=1, n_launches=1)),
]


@pytest.mark.parametrize("name,L,hq,h,D,idx,stride,policy,two_pass,expect", CHUNK, ids=[c[0] for c in CHUNK])
def test_chunk_step_against_the_oracle(name, L, hq, h, D, idx, stride, policy, two_pass, expect):
    from easykv_amd import KVBank, StepPlan
    from oracle import easykv_oracle as O
    W = idx + stride
    g = torch.Generator().manual_seed(idx + stride + D)
    bank = KVBank(L, hq, h, D, cap=W, dtype=BF)
    bank.load_rows(torch.randn(L, h, idx, D, generator=g).to(BF).cuda(), torch.randn(L, h, idx, D, generator=g).to(BF).cuda())
    bank.state_init(W, 2, stride)
    bp = idx
    kw = dict(policy=policy, phase="prefill", accumulate=True, evict=True, budget=bp, recent=int(bp * 0.1), sink=4, stride=stride)
    plan, oplan = StepPlan(two_pass=two_pass, **kw), O.StepPlan(**kw)
    info = bank.step_info(plan, stride)
    assert all(info[k_] == v_ for k_, v_ in expect.items()), (info, expect)
    hook = Hook()
    O.SELECT_HOOK = hook
    try:
        for i in range(3):
            states = _seed(bank, W)
            q, k, v = (torch.randn(L, hh, stride, D, generator=g).to(BF) for hh in (hq, h, h))
            out, ids = bank.attend(plan, q.cuda(), k.cuda(), v.cuda())
            assert out.dtype == BF
            for l in range(L):
                st = states[l]
                k_all, v_all = torch.cat([st.k[0], k[l].float()], 1), torch.cat([st.v[0], v[l].float()], 1)
                pv = _pv(q[l].float(), k_all, v_all, idx)
                o_ref, ids_ref = O.layer_step(st, q[l:l + 1].float(), k[l:l + 1].float(), v[l:l + 1].float(), oplan)
                _check_out(out[l], o_ref[0], pv, (name, i, l))
                _check_ids(hook, ids[l].cpu(), ids_ref, (name, i, l))
    finally:
        O.SELECT_HOOK = None
    assert bank.n_slots == [idx] * L


@pytest.mark.parametrize("scored", [False, True], ids=["unscored", "scored"])
def test_dense_prefix_against_the_oracle(scored):
    """The dense prefix of a prompt (t_prev = 0, q_len = r): 'full', and keep_attention (scored, no eviction) — outputs and S."""
    from easykv_amd import KVBank, StepPlan
    from oracle import easykv_oracle as O
    L, hq, h, D, n = 2, 8, 8, 128, 320
    g = torch.Generator().manual_seed(11 + scored)
    bank = KVBank(L, hq, h, D, cap=n + 64, dtype=BF)
    q, k, v = (torch.randn(L, hh, n, D, generator=g).to(BF) for hh in (hq, h, h))
    kw = dict(policy="roco" if scored else "full", phase="prefill", accumulate=scored, evict=False, stride=n)
    plan, oplan = StepPlan(**kw), O.StepPlan(**kw)
    if scored:
        bank.state_init(n, 1, n)
    info = bank.step_info(plan, n)
    assert info["wide"] == 1 and info["two_pass"] == int(scored), info
    states = []
    for l in range(L):
        st = O.LayerState(k=torch.zeros(1, h, 0, D), v=torch.zeros(1, h, 0, D))
        if scored:
            st.s, st.q, st.c = bank.score_sum[l, :, :n].cpu().clone(), bank.score_sq[l, :, :n].cpu().clone(), bank.score_cnt[l, :, :n].cpu().clone()
        states.append(st)
    out, _ = bank.attend(plan, q.cuda(), k.cuda(), v.cuda())
    S = bank.score_sum.cpu()
    for l in range(L):
        pv = _pv(q[l].float(), k[l].float(), v[l].float(), 0)
        o_ref, _ = O.layer_step(states[l], q[l:l + 1].float(), k[l:l + 1].float(), v[l:l + 1].float(), oplan)
        _check_out(out[l], o_ref[0], pv, ("prefix", scored, l))
        if scored:
            assert torch.allclose(S[l, :, :n], states[l].s[:, :n], rtol=2e-5, atol=1e-7)


# ---- (c) range ----------------------------------------------------------------------------------------------------------------
def test_range_beyond_fp16():
    """K and V of magnitude 1e5 .. 1e6 (bf16 has fp32's range; fp16 overflows above 65 504): the bf16 bank is finite and within the
    bar, an fp16 bank given the same values returns non-finite outputs — the reason bf16 banks exist."""
    from easykv_amd import KVBank, StepPlan
    from oracle import easykv_oracle as O
    L, hq, h, D, P, steps = 2, 8, 4, 128, 16, 8
    g = torch.Generator().manual_seed(3)
    big = lambda *s: (torch.randn(*s, generator=g) * torch.empty(*s).uniform_(1e5, 1e6, generator=g)).to(BF)
    k0, v0 = big(L, h, P + steps, D), big(L, h, P + steps, D)
    q = (torch.randn(L, hq, P + steps, D, generator=g) / 5e5).to(BF)
    assert k0.float().abs().max() > 65504
    plan, oplan = StepPlan(policy="full", phase="decode", accumulate=False), O.StepPlan(policy="full", phase="decode", accumulate=False)
    banks = {dt: KVBank(L, hq, h, D, cap=P + steps + 8, dtype=dt) for dt in (BF, torch.float16)}
    for b in banks.values():
        b.load_rows(k0[:, :, :P].cuda(), v0[:, :, :P].cuda())
    states = [O.LayerState(k=k0[l:l + 1, :, :P].float(), v=v0[l:l + 1, :, :P].float()) for l in range(L)]
    nonfinite = 0
    for i in range(steps):
        t = P + i
        args = (q[:, :, t:t + 1].cuda(), k0[:, :, t:t + 1].cuda(), v0[:, :, t:t + 1].cuda())
        out, _ = banks[BF].attend(plan, *args)
        o16, _ = banks[torch.float16].attend(plan, *args)
        nonfinite += int((~torch.isfinite(o16)).any())
        for l in range(L):
            st = states[l]
            k_all, v_all = torch.cat([st.k[0], k0[l, :, t:t + 1].float()], 1), torch.cat([st.v[0], v0[l, :, t:t + 1].float()], 1)
            pv = _pv(q[l, :, t:t + 1].float(), k_all, v_all, t)
            o_ref, _ = O.layer_step(st, q[l:l + 1, :, t:t + 1].float(), k0[l:l + 1, :, t:t + 1].float(), v0[l:l + 1, :, t:t + 1].float(), oplan)
            assert float(o_ref.abs().max()) > 1e4
            _check_out(out[l], o_ref[0], pv, ("range", i, l))
    assert nonfinite == steps


# ---- (d) bank operations ------------------------------------------------------------------------------------------------------
def test_bank_operations_on_a_bf16_bank():
    from easykv_amd import KVBank, StepPlan
    L, hq, h, D, n = 2, 8, 4, 64, 40
    g = torch.Generator().manual_seed(9)
    bank = KVBank(L, hq, h, D, cap=128, dtype=BF)
    k0, v0 = torch.randn(L, h, n, D, generator=g).to(BF), torch.randn(L, h, n, D, generator=g).to(BF)
    bank.load_rows(k0[:, :, :8].cuda(), v0[:, :, :8].cuda())
    plan = StepPlan(policy="full", phase="decode", accumulate=False)
    for t in range(8, n):       # appended rows
        bank.attend(plan, torch.randn(L, hq, 1, D, generator=g).to(BF).cuda(), k0[:, :, t:t + 1].cuda(), v0[:, :, t:t + 1].cuda())
    kk, vv = bank.ordered_kv()
    assert kk.dtype == BF and torch.equal(kk.cpu(), k0) and torch.equal(vv.cpu(), v0)
    # load_rows -> compact_inplace: exactly the survivors, in order
    b2 = KVBank(L, hq, h, D, cap=64, dtype=BF)
    b2.load_rows(k0.cuda(), v0.cuda())
    ev = torch.stack([torch.sort(torch.randperm(n, generator=g)[:5])[0] for _ in range(L * h)]).view(L, h, 5).int()
    b2.compact_inplace(ev.cuda())
    kk, vv = b2.ordered_kv()
    for l in range(L):
        for hh in range(h):
            keep = torch.ones(n, dtype=torch.bool)
            keep[ev[l, hh].long()] = False
            assert torch.equal(kk[l, hh].cpu(), k0[l, hh][keep]) and torch.equal(vv[l, hh].cpu(), v0[l, hh][keep])
    # rows_to_slots -> rows_to_order leaves the slot map and the score rows as they were
    b3 = KVBank(L, hq, h, D, cap=64, dtype=BF)
    b3.load_rows(k0.cuda(), v0.cuda())
    b3.state_init(n, 0)
    b3.score_sum[:, :, :n] += torch.rand(L, h, n, generator=g).cuda()
    before = (b3.slot_of_pos.clone(), b3.score_sum.clone(), b3.score_sq.clone(), b3.score_cnt.clone())
    s = torch.cuda.current_stream().cuda_stream
    assert b3.lib.ekv_rows_to_slots(C.byref(b3._bank), 0, L, n, C.c_void_p(s)) == 0
    assert b3.lib.ekv_rows_to_order(C.byref(b3._bank), 0, L, n, C.c_void_p(s)) == 0
    after = (b3._slot_of_pos, b3._score_sum, b3._score_sq, b3._score_cnt)
    for a, b_ in zip(before, after):
        assert torch.equal(a[:, :, :n], b_[:, :, :n])


# ---- (e) HF seam --------------------------------------------------------------------------------------------------------------
class _Tok:
    eos_token_id = -1

    def decode(self, ids, skip_special_tokens=True):
        return " ".join(str(i) for i in ids)


def _tiny(kind, seed=0):
    from transformers import LlamaConfig, LlamaForCausalLM, MistralConfig, MistralForCausalLM
    torch.manual_seed(seed)
    common = dict(vocab_size=97, hidden_size=256, intermediate_size=256, num_hidden_layers=2, num_attention_heads=4,
                  num_key_value_heads=2, head_dim=64, max_position_embeddings=512, attn_implementation="eager")
    if kind == "mistral":
        return MistralForCausalLM(MistralConfig(sliding_window=4096, **common)).to(BF).cuda().eval()
    return LlamaForCausalLM(LlamaConfig(**common)).to(BF).cuda().eval()


@pytest.mark.parametrize("kind", ["llama", "mistral"])
def test_hf_seam_bf16(kind, monkeypatch):
    import copy

    import easykv_amd
    from easykv_amd import api, engine, hf
    model = _tiny(kind)
    ref_model = copy.deepcopy(model).float()
    n0, n_dec = 40, 6
    ids = torch.randint(0, 97, (1, n0 + n_dec), device="cuda")
    with torch.inference_mode():
        ref_logits = ref_model(input_ids=ids).logits.float()
    hf.patch_model(model)
    easykv_amd.enable_fixed_kv(model, _Tok(), mode="decoding", stride=1)
    seen = []
    orig_cache_attend, orig_bank_attend = api.BudgetedKVCache.attend, engine.KVBank.attend

    def cache_attend(self, layer_idx, q, k, v):
        seen.append(("in", q.data_ptr(), k.data_ptr(), v.data_ptr(), q.dtype))
        return orig_cache_attend(self, layer_idx, q, k, v)

    def bank_attend(self, plan, q, k_new, v_new, *a, **kw):
        out = orig_bank_attend(self, plan, q, k_new, v_new, *a, **kw)
        seen.append(("bank", q.data_ptr(), k_new.data_ptr(), v_new.data_ptr(), q.dtype, out[0].data_ptr()))
        return out

    monkeypatch.setattr(api.BudgetedKVCache, "attend", cache_attend)
    monkeypatch.setattr(engine.KVBank, "attend", bank_attend)
    o_in = []
    hooks = [m.register_forward_pre_hook(lambda mod, args: o_in.append(args[0].data_ptr())) for name, m in model.named_modules()
             if name.endswith("self_attn.o_proj")]
    cache = easykv_amd.BudgetedKVCache(2, 4, 2, 64, 64, torch.device("cuda"), dtype=BF)
    got = []
    with torch.inference_mode():
        with cache.active(easykv_amd.StepPlan(policy="full", phase="prefill", accumulate=False)):
            got.append(model(input_ids=ids[:, :n0], past_key_values=cache, position_ids=torch.arange(n0, device="cuda").view(1, -1),
                             use_cache=True).logits.float())
        for t in range(n0, n0 + n_dec):       # teacher-forced decode
            with cache.active(easykv_amd.StepPlan(policy="full", phase="decode", accumulate=False)):
                got.append(model(input_ids=ids[:, t:t + 1], past_key_values=cache, position_ids=torch.tensor([[t]], device="cuda"),
                                 use_cache=True).logits.float())
    for hk in hooks:
        hk.remove()
    monkeypatch.undo()
    got = torch.cat(got, 1)
    assert torch.allclose(got, ref_logits, atol=3e-2, rtol=0), float((got - ref_logits).abs().max())
    ins, banks = [s for s in seen if s[0] == "in"], [s for s in seen if s[0] == "bank"]
    assert len(ins) == len(banks) == 2 * (1 + n_dec)
    for a, b in zip(ins, banks):
        assert a[1:4] == b[1:4] and a[4] == b[4] == BF      # the module's own bf16 views, read in place
    assert o_in == [b[5] for b in banks]                     # the output reaches o_proj without a conversion
    # encoding and auto modes with roco: the reference's geometry, as printed — the same lines as with an fp16 bank
    lines = {}
    for dt in ("bfloat16", "float16"):
        for mode, budget, stride in (("encoding", 0.5, 8), ("auto", 24, 8)):
            easykv_amd.enable_fixed_kv(model, _Tok(), mode=mode, stride=stride)
            buf = io.StringIO()
            with contextlib.redirect_stdout(buf):
                model.easykv_generate(input_ids=ids[:, :n0], generation_config=dict(temperature=1e-6, kv_policy="roco", budget=budget,
                                                                                    max_new_tokens=8, eos_token_ids=[-1], kv_dtype=dt))
            lines[(dt, mode)] = [ln for ln in buf.getvalue().splitlines() if "udget ratio" in ln]
    assert lines[("bfloat16", "encoding")] == lines[("float16", "encoding")] and lines[("bfloat16", "encoding")]
    assert lines[("bfloat16", "auto")] == lines[("float16", "auto")] and lines[("bfloat16", "auto")]
    if kind == "llama":      # one hipGraph decode run equals the eager run
        easykv_amd.enable_fixed_kv(model, _Tok(), mode="decoding", stride=1)
        runs = []
        for graph in (False, True):
            torch.manual_seed(11)     # the sampler draws from the global generator: same stream for both runs
            with contextlib.redirect_stdout(io.StringIO()):
                runs.append(model.easykv_generate(input_ids=ids[:, :n0], generation_config=dict(
                    temperature=0.7, kv_policy="roco", budget=24, max_new_tokens=40, eos_token_ids=[-1], kv_dtype="bfloat16", hipgraph=graph)))
        assert runs[0] == runs[1]


def test_kv_dtype_key():
    from easykv_amd import api
    model = _tiny("llama")
    assert api._kv_dtype(model, "auto") is BF and api._kv_dtype(model.half(), "auto") is torch.float16
    assert api._kv_dtype(model, "float16") is torch.float16 and api._kv_dtype(model, "bfloat16") is BF
    with pytest.raises(ValueError):
        api._kv_dtype(model, "fp8")


# ---- (f) refusal --------------------------------------------------------------------------------------------------------------
def test_bf16_with_streaming_is_refused_before_any_launch(monkeypatch):
    import easykv_amd
    from easykv_amd import engine, hf
    model = hf.patch_model(_tiny("llama"))
    easykv_amd.enable_fixed_kv(model, _Tok(), mode="encoding", stride=8)
    calls = []
    monkeypatch.setattr(engine.KVBank, "attend", lambda *a, **k: calls.append(1))
    ids = torch.randint(0, 97, (1, 40), device="cuda")
    with pytest.raises(ValueError, match="RoPE-on-read"):
        model.easykv_generate(input_ids=ids, generation_config=dict(kv_policy="roco", budget=0.5, streaming=True, kv_dtype="bfloat16",
                                                                    max_new_tokens=4, eos_token_ids=[-1]))
    assert calls == []
    from easykv_amd import KVBank, StepPlan
    bank = KVBank(1, 4, 2, 64, cap=64, dtype=BF)
    info = bank.step_info(StepPlan(policy="roco", phase="prefill", streaming=True, evict=True, budget=24, stride=8), 8)
    assert info["n_launches"] == 0 and info["fused"] == 0
