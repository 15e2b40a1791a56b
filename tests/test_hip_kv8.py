"""FP8 K/V storage with per-row scales ("kv8", include/easykv_hip.h) on the GPU.

* the quantiser (ekv_kv8_quantize / ekv_kv8_dequantize) against the properties of the rule (tests/kv8_ref.py);
* decode steps on a quantised bank against the CPU oracle ON THE BANK'S OWN CONTENTS: the oracle's cache is seeded with the
  dequantised rows and, step by step, is given the row the kernel appended (read back through dequantized_rows), so what is compared
  is the kernels' arithmetic on FP8 rows and nothing else.  Outputs under tests.golden_util.out_close (1e-3 flat, half an fp16 ulp
  above |ref| >= 1); victims identical wherever tests.test_hip_fullsize.Probe calls the oracle's decision well defined, and at least
  90 % of a case's decisions are.  The bf16-I/O cases draw V at 1/4 scale: a bf16 output carries up to half a bf16 ulp = 2^-9 |o| of
  rounding of its own, which the flat 1e-3 bar admits only below |o| = 0.5 — unit-variance V rows put a few outputs per thousand
  above that, and the bar would then measure the output format, not the kernel (DESIGN.md §7 gives bf16 outputs a relative bar for
  that reason); at 1/4 scale every |o| stays below 0.25 and the same flat bar applies to both types;
* refusals, the generation_config key, the HF seam end to end, and the recorded fidelity of a quantised bank against its 16-bit twin."""
import contextlib
import ctypes as C
import io
import json
import math
import os

import pytest
import torch

from tests import kv8_ref as R
from tests.golden_util import out_close
from tests.test_hip_fullsize import Probe

pytestmark = pytest.mark.gpu
BF, F16 = torch.bfloat16, torch.float16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- (a) the quantiser ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F16, BF], ids=["fp16", "bf16"])
@pytest.mark.parametrize("D", [64, 128])
def test_quantiser(dtype, D):
    from easykv_amd import KVBank, _lib
    L, hq, h, n = 2, 6, 3, 17      # rows of each kind per (layer, head): 68 physical rows, extent 68 < cap 128
    g = torch.Generator().manual_seed(D + (dtype is BF))
    bank = KVBank(L, hq, h, D, cap=100, dtype=dtype)
    ext = 4 * n
    assert ext < bank.cap
    perm = torch.stack([torch.randperm(bank.cap, generator=g) for _ in range(L * h)]).view(L, h, bank.cap).int()
    bank.slot_of_pos.copy_(perm.cuda())                      # a fragmented slot map: the conversion must not care
    xk = torch.stack([R.special_rows(n, D, g, dtype)[torch.randperm(ext, generator=g)] for _ in range(L * h)]).view(L, h, ext, D)
    xv = torch.stack([R.special_rows(n, D, g, dtype)[torch.randperm(ext, generator=g)] for _ in range(L * h)]).view(L, h, ext, D)
    bank.k.fill_(float("nan"))
    bank.v.fill_(float("nan"))
    bank.k[:, :, :ext] = xk.cuda()
    bank.v[:, :, :ext] = xv.cuda()
    src = (bank.k.clone(), bank.v.clone())
    k8 = torch.full((L, h, bank.cap, D), 0x55, dtype=torch.uint8, device="cuda")
    v8 = torch.full_like(k8, 0x55)
    ks = torch.full((L, h, bank.cap), 7.0, dtype=torch.float32, device="cuda")
    vs = torch.full_like(ks, 7.0)
    kv8 = _lib.Kv8(k8.data_ptr(), v8.data_ptr(), ks.data_ptr(), vs.data_ptr())
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert bank.lib.ekv_kv8_quantize(C.byref(bank._bank), C.byref(kv8), bank._dt, 0, L, ext, s) == 0
    torch.cuda.synchronize()
    same = True
    for x, codes, sc in ((xk, k8, ks), (xv, v8, vs)):
        R.check_rows(x, codes[:, :, :ext], sc[:, :, :ext], (dtype, D))
        assert bool((codes[:, :, ext:] == 0x55).all()) and bool((sc[:, :, ext:] == 7.0).all())       # rows >= extent untouched
        rc, rs = R.quantize(x)
        same &= torch.equal(rc, codes[:, :, :ext].cpu()) and torch.equal(rs, sc[:, :, :ext].cpu())
    print(f"[kv8-codes] {dtype} D={D}: codes and scales byte-identical to the torch restatement: {same}")
    assert torch.equal(bank.k.view(torch.int16), src[0].view(torch.int16)) and torch.equal(bank.v.view(torch.int16), src[1].view(torch.int16))
    # the inverse: exact in fp32, rounded once in the 16-bit types; a sub-range of layers
    for code, odt in ((_lib.DTYPE_F32, torch.float32), (_lib.DTYPE_F16, F16), (_lib.DTYPE_BF16, BF)):
        ko = torch.empty(1, h, ext, D, dtype=odt, device="cuda")
        vo = torch.empty_like(ko)
        assert bank.lib.ekv_kv8_dequantize(C.byref(bank._bank), C.byref(kv8), code, 1, 1, ext, ko.data_ptr(), vo.data_ptr(), s) == 0
        want_k, want_v = R.dequant(k8[1:2, :, :ext].cpu(), ks[1:2, :, :ext].cpu()), R.dequant(v8[1:2, :, :ext].cpu(), vs[1:2, :, :ext].cpu())
        assert torch.equal(ko.cpu().float(), want_k.to(odt).float()) and torch.equal(vo.cpu().float(), want_v.to(odt).float()), odt
    assert bank.lib.ekv_kv8_dequantize(C.byref(bank._bank), C.byref(kv8), 3, 0, 1, ext, ko.data_ptr(), vo.data_ptr(), s) == -1
    # KVBank.quantize_fp8: the same conversion in place; the slot map carries over, the 16-bit rows are released
    bank.extent, bank.n_slots = [ext] * L, [ext] * L
    before = bank.kv_bytes()
    assert before == L * h * bank.cap * 4 * D and bank.kv_quant is None
    bank.quantize_fp8()
    assert bank.kv_quant == "fp8" and bank.k is None and bank.v is None
    assert bank.kv_bytes() == L * h * bank.cap * (2 * D + 8)
    assert torch.equal(bank.slot_of_pos.cpu(), perm)
    assert torch.equal(bank.k8[:, :, :ext], k8[:, :, :ext]) and torch.equal(bank.v_scale[:, :, :ext], vs[:, :, :ext])
    kd, vd = bank.dequantized_rows(1)
    assert torch.equal(kd[:, :ext].cpu(), want_k[0]) and torch.equal(vd[:, :ext].cpu(), want_v[0])
    assert bool((kd[:, ext:] == 0).all())


# ---- (b) decode steps against the oracle on the bank's own contents ---------------------------------------------------------------
def _oracle_states(bank, W, layers):
    """LayerState of `layers` from the bank as it stands: dequantised rows in position order + the ordered score rows."""
    from oracle import easykv_oracle as O
    slot = bank.slot_of_pos.cpu().long()
    scored = bank._score_sum is not None
    S, Q, Cn = (bank.score_sum.cpu(), bank.score_sq.cpu(), bank.score_cnt.cpu()) if scored else (None, None, None)
    out = {}
    for l in layers:
        kd, vd = (x.cpu() for x in bank.dequantized_rows(l))
        t = bank.n_slots[l]
        idx = slot[l, :, :t].unsqueeze(-1).expand(-1, -1, kd.shape[-1])
        st = O.LayerState(k=torch.gather(kd, 1, idx).unsqueeze(0), v=torch.gather(vd, 1, idx).unsqueeze(0))
        if scored:
            st.s, st.q, st.c = S[l, :, :W].clone(), Q[l, :, :W].clone(), Cn[l, :, :W].clone()
        out[l] = st
    return out


STEPS = [
    # name, L, hq, h, D, dtype, budget, policy, n_split, defer, slot rows, expect (fused, split), steps
    ("fused 8-wave slot-indexed roco d128", 32, 8, 8, 128, F16, 96, "roco", 0, False, True, (1, False), 48),
    ("fused 8-wave ordered h2o GQA4 d64 bf16", 32, 32, 8, 64, BF, 96, "h2o_head", 0, False, False, (1, False), 44),
    ("fused 4-wave slot-indexed tova GQA3 d128", 4, 12, 4, 128, F16, 96, "tova", 1, False, True, (1, False), 44),
    ("fused 4-wave ordered roco GQA5 d64", 2, 10, 2, 64, F16, 96, "roco", 1, False, False, (1, False), 44),
    ("split roco d64", 2, 4, 4, 64, F16, 300, "roco", 3, False, False, (0, True), 24),
    ("split tova GQA4 d128 bf16", 2, 8, 2, 128, BF, 300, "tova", 3, False, False, (0, True), 24),
    ("split recency d128", 2, 4, 4, 128, F16, 300, "recency", 3, False, False, (0, True), 12),
    ("split random GQA4 d64 bf16", 2, 8, 2, 64, BF, 300, "random", 3, False, False, (0, True), 12),
    ("split full d64", 2, 4, 4, 64, F16, 300, "full", 3, False, False, (0, True), 12),
    ("fused full GQA4 d128", 2, 8, 2, 128, F16, 96, "full", 1, False, False, (1, False), 12),
    ("fused recency d64 bf16", 32, 8, 8, 64, BF, 96, "recency", 0, False, False, (1, False), 12),
    ("deferred roco GQA4 d128 bf16", 4, 8, 2, 128, BF, 96, "roco", 0, True, False, (0, False), 44),
    ("deferred h2o d64", 3, 4, 4, 64, F16, 96, "h2o_head", 0, True, False, (0, False), 44),
]


@pytest.mark.parametrize("name,L,hq,h,D,dtype,budget,policy,n_split,defer,slot,expect,steps", STEPS, ids=[c[0] for c in STEPS])
def test_decode_steps_against_the_oracle_on_the_banks_own_contents(name, L, hq, h, D, dtype, budget, policy, n_split, defer, slot, expect, steps, monkeypatch):
    from easykv_amd import KVBank, StepPlan, engine
    from oracle import easykv_oracle as O
    monkeypatch.setattr(engine.KVBank, "use_slot_rows", slot)
    scored = policy in ("roco", "h2o_head", "tova")
    evict = policy != "full"
    T = budget + 1
    v_scale = 0.25 if dtype is BF else 1.0      # (see the module docstring)
    g = torch.Generator().manual_seed(5)
    bank = KVBank(L, hq, h, D, cap=T + (steps if not evict else 0) + 8, dtype=dtype)
    bank.load_rows(torch.randn(L, h, budget, D, generator=g).to(dtype).cuda(), (torch.randn(L, h, budget, D, generator=g) * v_scale).to(dtype).cuda())
    if scored:
        bank.state_init(T, 0)
        warm = torch.rand(L, h, budget, generator=g) * 1e-3
        bank.score_sum[:, :, :budget] += warm.cuda()
        bank.score_sq[:, :, :budget] += (warm ** 2).cuda()
    bank.quantize_fp8()
    check_layers = sorted({0, L - 1})
    states = _oracle_states(bank, T, check_layers)
    kw = dict(policy=policy, phase="decode", evict=evict, accumulate=scored, score_off=0, budget=budget)
    info = bank.step_info(StepPlan(n_split=n_split, range_start=4 if policy in ("recency", "random") else -1, **kw), 1, 0, 1 if defer else L,
                          phases=5 if defer else 0)
    assert info["fused"] == expect[0] and (info["n_split"] > 1) == expect[1] and info["n_launches"] >= 1, info
    probe = Probe()
    O.SELECT_HOOK = probe
    n_dec = n_stable = n_slot = 0
    rows = torch.arange(h)
    try:
        for i in range(steps):
            q, k, v = torch.randn(L, hq, 1, D, generator=g).to(dtype), torch.randn(L, h, 1, D, generator=g).to(dtype), (torch.randn(L, h, 1, D, generator=g) * v_scale).to(dtype)
            rs = -1
            if policy == "recency":
                rs = 4
            elif policy == "random":
                rs = int(torch.randint(0, budget - 1, (1,), generator=g))
            plan = StepPlan(n_split=n_split, range_start=rs, **kw)
            # the row this step appends to: the front of the free list (valid in either score-row layout)
            new_row = torch.stack([bank._slot_of_pos[l, :, bank.n_slots[l]] for l in check_layers]).cpu().long()
            if defer:
                outs = [bank.attend(plan, q[l:l + 1].cuda(), k[l:l + 1].cuda(), v[l:l + 1].cuda(), layer_begin=l, defer=True)[0] for l in range(L)]
                ids = bank.flush()
                out = torch.cat(outs)
            else:
                out, ids = bank.attend(plan, q.cuda(), k.cuda(), v.cuda())
                n_slot += int(all(bank._slot_rows))
            assert out.dtype == dtype
            reseed = []
            for j, l in enumerate(check_layers):
                # the appended row: quantised by the kernel as the rule says, and attended as stored
                for given, codes, sc in ((k[l, :, 0], bank.k8[l], bank.k_scale[l]), (v[l, :, 0], bank.v8[l], bank.v_scale[l])):
                    R.check_rows(given, codes[rows, new_row[j]], sc[rows, new_row[j]], (name, i, l))
                kd, vd = bank.dequantized_rows(l)
                kq, vq = kd[rows, new_row[j]].cpu().view(1, h, 1, D), vd[rows, new_row[j]].cpu().view(1, h, 1, D)
                o_ref, ids_ref = O.layer_step(states[l], q[l:l + 1].float(), kq, vq, O.StepPlan(range_start=rs, **kw))
                assert out_close(out[l].float().cpu(), o_ref[0]), (name, i, l, float((out[l].float().cpu() - o_ref[0]).abs().max()))
                if scored:
                    unstable = probe.last_unstable
                    same = ids[l, :, 0].cpu().long() == ids_ref[:, 0]
                    n_dec += h
                    n_stable += int((~unstable).sum())
                    assert bool(same[~unstable].all()), (name, i, l)      # a well-defined decision: identical
                    if not bool(same.all()):
                        reseed.append(l)
                elif evict:
                    assert bool((ids[l].cpu().long() == rs).all())
            if reseed:      # an ill-defined decision went the other way: the oracle follows the bank from here
                fresh = _oracle_states(bank, T, reseed)
                states.update(fresh)
                bank._slot_short = 0
    finally:
        O.SELECT_HOOK = None
    if scored:
        assert n_stable >= 0.9 * n_dec, (n_stable, n_dec)
    if slot:
        assert n_slot >= steps - 4, n_slot      # the one-launch step ran on the slot-indexed score rows
    assert bank.n_slots == [budget + (0 if evict else steps)] * L


# ---- (c) refusals ---------------------------------------------------------------------------------------------------------------
class _NoCalls:
    def __getattr__(self, name):
        raise AssertionError(f"library call {name} after a refusal")


def test_refusals_after_quantize_fp8():
    from easykv_amd import KVBank, StepPlan
    from easykv_amd._lib import EkvError
    from oracle import easykv_oracle as O
    L, hq, h, D = 2, 4, 2, 64
    g = torch.Generator().manual_seed(1)
    bank = KVBank(L, hq, h, D, cap=128)
    bank.load_rows(torch.randn(L, h, 40, D, generator=g).half().cuda(), torch.randn(L, h, 40, D, generator=g).half().cuda())
    bank.quantize_fp8()
    assert bank.quantize_fp8() is bank      # idempotent
    # what the library itself says to a chunk step / RoPE-on-read step of a kv8 bank: unsupported, nothing planned
    chunk = StepPlan(policy="full", phase="prefill", accumulate=False)
    assert bank.step_info(chunk, 8)["n_launches"] == 0 and bank.step_plan(chunk, 8)[1] is False
    assert bank.step_info(StepPlan(policy="full", phase="decode", accumulate=False, streaming=True), 1)["n_launches"] == 0
    lib, bank.lib = bank.lib, _NoCalls()
    q8, k8 = torch.randn(L, hq, 8, D).half().cuda(), torch.randn(L, h, 8, D).half().cuda()
    with pytest.raises(EkvError, match="chunk step"):
        bank.attend(chunk, q8, k8, k8)
    with pytest.raises(EkvError, match="chunk step"):
        bank.attend(chunk, q8[:1], k8[:1], k8[:1], layer_begin=0, defer=True)
    with pytest.raises(EkvError, match="set_rope"):
        bank.set_rope(*O.rope_tables(128, D))
    with pytest.raises(EkvError, match="load_rows"):
        bank.load_rows(k8, k8)
    with pytest.raises(EkvError, match="row move"):
        bank.ordered_kv()
    with pytest.raises(EkvError, match="row move"):
        bank.compact_inplace(torch.zeros(L, h, 1, dtype=torch.int32))
    bank.lib = lib
    assert bank.n_slots == [40] * L
    with pytest.raises(EkvError):      # a RoPE-on-read decode step: refused by the dry run of the call itself
        bank.attend(StepPlan(policy="full", phase="decode", accumulate=False, streaming=True), q8[:, :, :1], k8[:, :, :1], k8[:, :, :1])
    assert bank.n_slots == [40] * L
    for d in (32, 96):
        b2 = KVBank(1, 2, 2, d, cap=64)
        with pytest.raises(EkvError, match="head_dim"):
            b2.quantize_fp8()
    b3 = KVBank(1, 2, 2, 64, cap=64)
    b3.set_rope(*O.rope_tables(64, 64))
    with pytest.raises(EkvError, match="RoPE-on-read"):
        b3.quantize_fp8()


class _Tok:
    eos_token_id = -1

    def decode(self, ids, skip_special_tokens=True):
        return " ".join(str(i) for i in ids)


def _tiny(kind):
    from tests.test_hip_bf16 import _tiny as tiny
    return tiny(kind)


def test_kv_quant_key_refusals(monkeypatch):
    import easykv_amd
    from easykv_amd import engine, hf
    model = hf.patch_model(_tiny("llama"))
    calls = []
    monkeypatch.setattr(engine.KVBank, "attend", lambda *a, **k: calls.append(1))
    ids = torch.randint(0, 97, (1, 40), device="cuda")
    gen = dict(kv_policy="roco", budget=0.5, max_new_tokens=4, eos_token_ids=[-1], kv_quant="fp8")
    easykv_amd.enable_fixed_kv(model, _Tok(), mode="encoding", stride=8)
    with pytest.raises(ValueError, match="streaming"):
        model.easykv_generate(input_ids=ids, generation_config=dict(gen, streaming=True))
    with pytest.raises(ValueError, match="ppl"):
        model.easykv_ppl(input_ids=ids, generation_config=gen)
    with pytest.raises(ValueError, match="kv_quant"):
        model.easykv_generate(input_ids=ids, generation_config=dict(gen, kv_quant="int4"))
    with pytest.raises(ValueError):      # 'fp8' stays an invalid kv_dtype
        model.easykv_generate(input_ids=ids, generation_config=dict(gen, kv_quant=None, kv_dtype="fp8"))

    class Shard:
        world, rank, begin, count = 2, 0, 0, 1
    model.layer_shard = Shard()
    try:
        with pytest.raises(ValueError, match="layer-sharded"):
            model.easykv_generate(input_ids=ids, generation_config=gen)
    finally:
        del model.layer_shard
    assert calls == []


# ---- (d) end to end -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["llama", "mistral"])
def test_generate_with_kv_quant_fp8(kind):
    import easykv_amd
    from easykv_amd import hf
    model = hf.patch_model(_tiny(kind))
    n0, new = 40, 12
    ids = torch.randint(0, 97, (1, n0), device="cuda", generator=torch.Generator(device="cuda").manual_seed(3))

    def run(mode, budget, stride, **extra):
        easykv_amd.enable_fixed_kv(model, _Tok(), mode=mode, stride=stride)
        gen = dict(temperature=1e-6, kv_policy="roco", budget=budget, max_new_tokens=new, eos_token_ids=[-1], kv_dtype="auto", **extra)
        torch.manual_seed(11)
        with contextlib.redirect_stdout(io.StringIO()):
            return model.easykv_generate(input_ids=ids, generation_config=gen, return_cache=True)

    for mode, budget, stride in (("decoding", 8, 1), ("encoding", 0.5, 8), ("auto", 24, 8)):
        text, cache = run(mode, budget, stride, kv_quant="fp8")
        assert len(text.split()) == new, (mode, text)
        b = cache.bank
        assert cache.kv_quant == "fp8" and b.k is None
        assert cache.kv_bytes() == b.n_layers * b.n_kv_heads * b.cap * (2 * b.head_dim + 8)
        # greedy eager == hipGraph, token for token (the decode forward is captured after the conversion)
        text_g, cache_g = run(mode, budget, stride, kv_quant="fp8", hipgraph=True)
        assert text_g == text and cache_g.kv_quant == "fp8", mode
        # kv_quant=None is a run without the key: ids and evictions
        t0, c0 = run(mode, budget, stride, _record_evictions=True)
        t1, c1 = run(mode, budget, stride, _record_evictions=True, kv_quant=None)
        assert t0 == t1 and c0.kv_quant is None and c1.kv_quant is None
        assert len(c0.evictions) == len(c1.evictions)
        for a, b_ in zip(c0.evictions, c1.evictions):
            assert all(torch.equal(x, y) for x, y in zip(a, b_))


# ---- (e) fidelity: recorded, not barred -------------------------------------------------------------------------------------------
def test_fidelity_of_a_quantised_bank_is_recorded():
    """The same prompt rows and the same 64 decode steps on a 16-bit bank and on its quantised twin, both against the oracle on the
    UNQUANTISED rows.  Recorded in profiles/kv8_fidelity.json; no pass mark for the quantised twin (nothing is known yet), the
    16-bit twin still meets its own bar."""
    from easykv_amd import KVBank, StepPlan
    from oracle import easykv_oracle as O
    L, hq, h, D, budget, steps = 2, 8, 8, 128, 256, 64
    T = budget + 1
    result = {"shape": dict(layers=L, q_heads=hq, kv_heads=h, head_dim=D, budget=budget, steps=steps, rows="standard normal, fp16"), "policies": {}}
    for policy in ("roco", "h2o_head", "tova"):
        g = torch.Generator().manual_seed(21)
        k0, v0 = torch.randn(L, h, budget, D, generator=g).half(), torch.randn(L, h, budget, D, generator=g).half()
        warm = torch.rand(L, h, budget, generator=g) * 1e-3
        banks = {}
        for name in ("fp16", "fp8"):
            b = KVBank(L, hq, h, D, cap=T + 8)
            b.load_rows(k0.cuda(), v0.cuda())
            b.state_init(T, 0)
            b.score_sum[:, :, :budget] += warm.cuda()
            b.score_sq[:, :, :budget] += (warm ** 2).cuda()
            banks[name] = b
        banks["fp8"].quantize_fp8()
        states = []
        for l in range(L):
            st = O.LayerState(k=k0[l:l + 1].float(), v=v0[l:l + 1].float())
            st.s, st.q, st.c = O.init_state_decoding((h,), budget)
            st.s[:, :budget] += warm[l]
            st.q[:, :budget] += warm[l] ** 2
            states.append(st)
        kw = dict(policy=policy, phase="decode", evict=True, score_off=0, budget=budget)
        probe = Probe()
        O.SELECT_HOOK = probe
        sq = {n: 0.0 for n in banks}
        mx = {n: 0.0 for n in banks}
        diff = {n: 0 for n in banks}
        n_el = n_dec = 0
        alive = torch.ones(L, h, dtype=torch.bool)
        try:
            for i in range(steps):
                q, k, v = (torch.randn(L, n, 1, D, generator=g).half() for n in (hq, h, h))
                got = {n: b.attend(StepPlan(**kw), q.cuda(), k.cuda(), v.cuda()) for n, b in banks.items()}
                for l in range(L):
                    o_ref, ids_ref = O.layer_step(states[l], q[l:l + 1].float(), k[l:l + 1].float(), v[l:l + 1].float(), O.StepPlan(**kw))
                    unstable = probe.last_unstable
                    for n, (o, ids) in got.items():
                        err = (o[l].float().cpu() - o_ref[0]).abs()
                        sq[n] += float((err.double() ** 2).sum())
                        mx[n] = max(mx[n], float(err.max()))
                        diff[n] += int((ids[l, :, 0].cpu().long() != ids_ref[:, 0]).sum())
                    n_el += err.numel()
                    n_dec += h
                    # the 16-bit twin's own bar: outputs, and victims wherever the decision is well defined (heads still in lockstep)
                    same = got["fp16"][1][l, :, 0].cpu().long() == ids_ref[:, 0]
                    ok = alive[l] & ~unstable
                    assert bool(same[ok].all()), (policy, i, l)
                    alive[l] &= ~unstable & same
                    if bool(alive[l].all()):
                        assert out_close(got["fp16"][0][l].float().cpu(), o_ref[0]), (policy, i, l)
        finally:
            O.SELECT_HOOK = None
        result["policies"][policy] = {n: dict(max_abs_err=mx[n], rms_err=math.sqrt(sq[n] / n_el), evictions_differing=diff[n] / n_dec) for n in banks}
        result["policies"][policy]["decisions"] = n_dec
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    path = os.path.join(ROOT, "profiles", "kv8_fidelity.json")
    with open(path, "w") as f:
        json.dump(result, f, indent=1)
    back = json.load(open(path))
    for policy, r in back["policies"].items():
        for n in ("fp16", "fp8"):
            assert all(math.isfinite(x) for x in r[n].values()), (policy, n, r[n])
    print("[kv8-fidelity]", json.dumps(back["policies"]))
