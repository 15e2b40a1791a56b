"""MXFP6 K/V storage with block exponents ("kv6", include/easykv_hip.h) on the GPU.

* the packing of a block as the conversions read it (crafted planes through ekv_kv6_dequantize);
* the quantiser (ekv_kv6_quantize / ekv_kv6_dequantize) IS the rule (tests/kv6_ref.py): exponents equal, codes equal up to +-0 — the
  rule has no rounding of its own, so identity is what an implementation owes;
* decode steps on a quantised bank against the CPU oracle ON THE BANK'S OWN CONTENTS, by the scheme of tests/test_hip_kv8.py: the
  oracle's cache is seeded with the dequantised rows and, step by step, is given the row the kernel appended (read back through
  dequantized_rows), so what is compared is the kernels' arithmetic on MXFP6 rows and nothing else.  Outputs under
  tests.golden_util.out_close; victims identical wherever tests.test_hip_fullsize.Probe calls the oracle's decision well defined, and
  at least 90 % of a case's decisions are (tests/test_kv6_cpu.py holds the seeded cases to that on the reference side alone);
* the edges of the 16-row wave-load, refusals, the generation_config key, the HF seam end to end, and the recorded fidelity."""
import contextlib
import ctypes as C
import io
import json
import math
import os

import pytest
import torch

from tests import kv6_cases as K
from tests import kv6_ref as R
from tests.golden_util import out_close
from tests.test_hip_fullsize import Probe

pytestmark = pytest.mark.gpu
BF, F16 = torch.bfloat16, torch.float16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D = 128


# ---- (a) the packing, then the quantiser ------------------------------------------------------------------------------------------
def test_packing_probe():
    """Crafted planes through ekv_kv6_dequantize to fp32: a block whose codes are 0 .. 31 in element order, blocks that hold all 64
    codes (the negative half reversed), and every exponent byte that scales them differently — bit-equal to kv6_ref.dequant, so the
    element order of the 24 bytes, the sign bit and the grid are what the header says."""
    from easykv_amd import KVBank, _lib
    h, cap = 2, 64
    bank = KVBank(1, h, h, D, cap=cap)
    codes = torch.zeros(1, h, cap, D, dtype=torch.int32)
    codes[0, 0, 0, :32] = torch.arange(32)
    codes[0, 0, 0, 32:64] = torch.arange(32, 64)
    codes[0, 0, 0, 64:96] = torch.arange(63, 31, -1)
    codes[0, 0, 0, 96:] = torch.arange(31, -1, -1)
    g = torch.Generator().manual_seed(6)
    codes[0, :, 1:] = torch.randint(0, 64, (h, cap - 1, D), generator=g, dtype=torch.int32)
    exps = torch.randint(100, 150, (1, h, cap, D // 32), generator=g, dtype=torch.int32).to(torch.uint8)
    exps[0, 0, 0] = torch.tensor([127, 128, 1, 254], dtype=torch.uint8)
    planes = R.pack(codes)
    assert planes.shape == (1, h, cap, 96) and torch.equal(R.unpack(planes), codes)
    assert planes[0, 0, 0, :3].tolist() == [0 | (1 << 6) & 255, (1 >> 2) | (2 << 4) & 255, (2 >> 4) | (3 << 2)]      # elements 0..3 in bytes 0..2
    kc, ke = planes.cuda(), exps.cuda()
    vc, ve = kc.flip(2).contiguous(), ke.flip(2).contiguous()
    kv6 = _lib.Kv6(kc.data_ptr(), vc.data_ptr(), ke.data_ptr(), ve.data_ptr())
    ko = torch.empty(1, h, cap, D, dtype=torch.float32, device="cuda")
    vo = torch.empty_like(ko)
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert bank.lib.ekv_kv6_dequantize(C.byref(bank._bank), C.byref(kv6), _lib.DTYPE_F32, 0, 1, cap, ko.data_ptr(), vo.data_ptr(), s) == 0
    torch.cuda.synchronize()
    want = R.dequant(planes, exps)
    assert torch.equal(ko.cpu().view(torch.int32), want.view(torch.int32)), int((ko.cpu() != want).sum())
    assert torch.equal(vo.cpu().view(torch.int32), want.flip(2).view(torch.int32))
    assert ko[0, 0, 0, :32].cpu().tolist() == R.GRID.tolist() and ko[0, 0, 0, 32:64].cpu().tolist() == (-R.GRID * 2).tolist()


@pytest.mark.parametrize("dtype", [F16, BF], ids=["fp16", "bf16"])
def test_quantiser(dtype):
    from easykv_amd import KVBank, _lib
    L, hq, h, n = 2, 6, 3, 11      # rows of each of the 6 kinds per (layer, head): 66 physical rows, extent 66 < cap 128
    g = torch.Generator().manual_seed(128 + (dtype is BF))
    bank = KVBank(L, hq, h, D, cap=100, dtype=dtype)
    ext = 6 * n
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
    k6 = torch.full((L, h, bank.cap, 3 * D // 4), 0x55, dtype=torch.uint8, device="cuda")
    v6 = torch.full_like(k6, 0x55)
    ke = torch.full((L, h, bank.cap, D // 32), 77, dtype=torch.uint8, device="cuda")
    ve = torch.full_like(ke, 77)
    kv6 = _lib.Kv6(k6.data_ptr(), v6.data_ptr(), ke.data_ptr(), ve.data_ptr())
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert bank.lib.ekv_kv6_quantize(C.byref(bank._bank), C.byref(kv6), bank._dt, 0, L, ext, s) == 0
    torch.cuda.synchronize()
    for x, codes, ex in ((xk, k6, ke), (xv, v6, ve)):
        R.check_rows(x, codes[:, :, :ext], ex[:, :, :ext], dtype)      # exponents equal, codes equal up to +-0
        assert bool((codes[:, :, ext:] == 0x55).all()) and bool((ex[:, :, ext:] == 77).all())       # rows >= extent untouched
    assert torch.equal(bank.k.view(torch.int16), src[0].view(torch.int16)) and torch.equal(bank.v.view(torch.int16), src[1].view(torch.int16))
    # the inverse: exact in fp32 (code * 2^e), rounded once in the 16-bit types; a sub-range of layers
    for code, odt in ((_lib.DTYPE_F32, torch.float32), (_lib.DTYPE_F16, F16), (_lib.DTYPE_BF16, BF)):
        ko = torch.empty(1, h, ext, D, dtype=odt, device="cuda")
        vo = torch.empty_like(ko)
        assert bank.lib.ekv_kv6_dequantize(C.byref(bank._bank), C.byref(kv6), code, 1, 1, ext, ko.data_ptr(), vo.data_ptr(), s) == 0
        want_k, want_v = R.dequant(k6[1:2, :, :ext].cpu(), ke[1:2, :, :ext].cpu()), R.dequant(v6[1:2, :, :ext].cpu(), ve[1:2, :, :ext].cpu())
        assert torch.equal(ko.cpu().float(), want_k.to(odt).float()) and torch.equal(vo.cpu().float(), want_v.to(odt).float()), odt
    assert bank.lib.ekv_kv6_dequantize(C.byref(bank._bank), C.byref(kv6), 3, 0, 1, ext, ko.data_ptr(), vo.data_ptr(), s) == -1
    # KVBank.quantize_mxfp6: the same conversion in place; the slot map carries over, the 16-bit rows are released
    bank.extent, bank.n_slots = [ext] * L, [ext] * L
    assert bank.kv_bytes() == L * h * bank.cap * 4 * D and bank.kv_quant is None
    bank.quantize_mxfp6()
    assert bank.kv_quant == "mxfp6" and bank.k is None and bank.v is None
    assert bank.kv_bytes() == L * h * bank.cap * 200
    assert torch.equal(bank.slot_of_pos.cpu(), perm)
    assert torch.equal(bank.k6[:, :, :ext], k6[:, :, :ext]) and torch.equal(bank.v_exp[:, :, :ext], ve[:, :, :ext])
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


def _appended_rows_are_the_rules(bank, l, rows, new_row, k, v, what):
    """The row a step appended: quantised by the kernel as the rule says (exponents equal, codes equal up to +-0)."""
    for given, codes, ex in ((k, bank.k6[l], bank.k_exp[l]), (v, bank.v6[l], bank.v_exp[l])):
        R.check_rows(given, codes[rows, new_row], ex[rows, new_row], what)


@pytest.mark.parametrize("case", K.STEPS, ids=[c[0] for c in K.STEPS])
def test_decode_steps_against_the_oracle_on_the_banks_own_contents(case, monkeypatch):
    from easykv_amd import KVBank, StepPlan, engine
    from oracle import easykv_oracle as O
    name, L, hq, h, dtype, budget, policy, n_split, defer, slot, expect, steps = case
    monkeypatch.setattr(engine.KVBank, "use_slot_rows", slot)
    scored = policy in K.SCORED
    evict = policy != "full"
    T = budget + 1
    k0, v0, warm, per_step = K.inputs(case)
    bank = KVBank(L, hq, h, D, cap=T + (steps if not evict else 0) + 8, dtype=dtype)
    bank.load_rows(k0.cuda(), v0.cuda())
    if scored:
        bank.state_init(T, 0)
        bank.score_sum[:, :, :budget] += warm.cuda()
        bank.score_sq[:, :, :budget] += (warm ** 2).cuda()
    bank.quantize_mxfp6()
    check_layers = sorted({0, L - 1})
    states = _oracle_states(bank, T, check_layers)
    kw = K.plan_kw(case)
    info = bank.step_info(StepPlan(n_split=n_split, range_start=4 if policy in ("recency", "random") else -1, **kw), 1, 0, 1 if defer else L,
                          phases=5 if defer else 0)
    assert info["fused"] == expect[0] and (info["n_split"] > 1) == expect[1] and info["n_launches"] >= 1 and info["fused_order"] == 0, info
    probe = Probe()
    O.SELECT_HOOK = probe
    n_dec = n_stable = n_slot = 0
    rows = torch.arange(h)
    try:
        for i, (q, k, v, rs) in enumerate(per_step):
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
                _appended_rows_are_the_rules(bank, l, rows, new_row[j], k[l, :, 0], v[l, :, 0], (name, i, l))
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
                states.update(_oracle_states(bank, T, reseed))
                bank._slot_short = 0
    finally:
        O.SELECT_HOOK = None
    if scored:
        assert n_stable >= 0.9 * n_dec, (n_stable, n_dec)
    if slot:
        assert n_slot >= steps - 4, n_slot      # the one-launch step ran on the slot-indexed score rows
    assert bank.n_slots == [budget + (0 if evict else steps)] * L


class _ProbeAndCapture:
    """oracle.SELECT_HOOK: the stability probe, and the score rows the selection saw."""

    def __init__(self):
        from tests.select_rule import Capture
        self.probe, self.cap = Probe(), Capture()

    def __call__(self, *args):
        self.probe(*args)
        self.cap(*args)


# budgets around the 16 rows of a wave-load (a 4-lane row group: 16 rows per load instruction), and a cache that fills its bank
# (KVBank rounds cap up to a multiple of 64: budget 63 appends into the last row, cap == n_slots + 1)
EDGES = [(1, "full"), (15, "roco"), (16, "roco"), (17, "roco"), (63, "roco"), (63, "full")]


@pytest.mark.parametrize("budget,policy", EDGES, ids=[f"budget{b}-{p}" for b, p in EDGES])
@pytest.mark.parametrize("n_split", [1, 2], ids=["one-launch", "split"])
def test_wave_load_edges(budget, policy, n_split):
    from easykv_amd import KVBank, StepPlan
    from oracle import easykv_oracle as O
    from tests.select_rule import feasible_classes, valid_victims
    if n_split > budget:
        n_split = 1
    n_tied = 0
    L, hq, h = 2, 4, 2
    scored, evict = policy != "full", policy != "full"
    T = budget + 1
    g = torch.Generator().manual_seed(11 + budget)
    bank = KVBank(L, hq, h, D, cap=T)
    assert bank.cap == 64 and (budget != 63 or bank.cap == budget + 1)
    bank.load_rows(torch.randn(L, h, budget, D, generator=g).half().cuda(), torch.randn(L, h, budget, D, generator=g).half().cuda())
    if scored:
        bank.state_init(T, 0)
        warm = torch.rand(L, h, budget, generator=g) * 1e-3
        bank.score_sum[:, :, :budget] += warm.cuda()
        bank.score_sq[:, :, :budget] += (warm ** 2).cuda()
    bank.quantize_mxfp6()
    states = _oracle_states(bank, T, range(L))
    kw = dict(policy=policy, phase="decode", evict=evict, accumulate=scored, score_off=0, budget=budget)
    plan = StepPlan(n_split=n_split, **kw)
    info = bank.step_info(plan, 1)
    assert info["n_launches"] >= 1 and info["n_split"] <= max(n_split, 1), info
    print(f"[kv6-edge] budget {budget} {policy} n_split asked {n_split}: {info}")
    q, k, v = torch.randn(L, hq, 1, D, generator=g).half(), torch.randn(L, h, 1, D, generator=g).half(), torch.randn(L, h, 1, D, generator=g).half()
    new_row = torch.stack([bank._slot_of_pos[l, :, bank.n_slots[l]] for l in range(L)]).cpu().long()
    hook = _ProbeAndCapture()
    O.SELECT_HOOK = hook
    k1 = budget - int(budget * O.DECODE_RECENT_RATIO)      # roco's feasible set: the k1 smallest standard deviations
    try:
        out, ids = bank.attend(plan, q.cuda(), k.cuda(), v.cuda())
        rows = torch.arange(h)
        for l in range(L):
            _appended_rows_are_the_rules(bank, l, rows, new_row[l], k[l, :, 0], v[l, :, 0], (budget, policy, l))
            kd, vd = bank.dequantized_rows(l)
            kq, vq = kd[rows, new_row[l]].cpu().view(1, h, 1, D), vd[rows, new_row[l]].cpu().view(1, h, 1, D)
            o_ref, ids_ref = O.layer_step(states[l], q[l:l + 1].float(), kq, vq, O.StepPlan(**kw))
            assert out_close(out[l].float().cpu(), o_ref[0]), (budget, policy, l, float((out[l].float().cpu() - o_ref[0]).abs().max()))
            if scored:
                got = ids[l, :, 0].cpu().long()
                c = hook.cap
                for hd in range(h):
                    if bool(hook.probe.last_unstable[hd]):
                        continue
                    # budgets below 30 leave fewer than k1 rows outside roco's 10-row tail, so the feasible set takes part of the
                    # tail's tied sentinel class: torch takes an arbitrary subset there, the kernels the lowest indices (DESIGN.md
                    # section 7), and tests/select_rule.py decides exactly whether the victim is one the reference's rule can give
                    forced, pool, need = feasible_classes(O.roco_std(c.s, c.q, c.c)[hd], k1)
                    assert valid_victims([int(got[hd])], (c.s / c.c)[hd], forced, pool, need, 1), (budget, policy, l, hd, int(got[hd]))
                    if len(pool) == need:      # no tied class at the cut: the decision is well defined, so identical
                        assert int(got[hd]) == int(ids_ref[hd, 0]), (budget, policy, l, hd, int(got[hd]), int(ids_ref[hd, 0]))
                    else:
                        n_tied += 1
    finally:
        O.SELECT_HOOK = None
    assert bank.n_slots == [budget + (0 if evict else 1)] * L
    assert n_tied == 0 or budget < 30, (budget, n_tied)      # identity is given up only where the reference's rule itself is a set


# ---- (c) refusals ---------------------------------------------------------------------------------------------------------------
class _NoCalls:
    def __getattr__(self, name):
        raise AssertionError(f"library call {name} after a refusal")


def test_refusals_after_quantize_mxfp6():
    from easykv_amd import KVBank, StepPlan
    from easykv_amd._lib import EkvError
    from oracle import easykv_oracle as O
    L, hq, h = 2, 4, 2
    g = torch.Generator().manual_seed(1)
    bank = KVBank(L, hq, h, D, cap=128)
    bank.load_rows(torch.randn(L, h, 40, D, generator=g).half().cuda(), torch.randn(L, h, 40, D, generator=g).half().cuda())
    bank.quantize_mxfp6()
    # what the library itself says to a chunk step / RoPE-on-read step of a kv6 bank: unsupported, nothing planned
    chunk = StepPlan(policy="full", phase="prefill", accumulate=False)
    assert bank.step_info(chunk, 8)["n_launches"] == 0 and bank.step_plan(chunk, 8)[1] is False
    assert bank.step_info(StepPlan(policy="full", phase="decode", accumulate=False, streaming=True), 1)["n_launches"] == 0
    lib, bank.lib = bank.lib, _NoCalls()
    q8, k8 = torch.randn(L, hq, 8, D).half().cuda(), torch.randn(L, h, 8, D).half().cuda()
    for again in (bank.quantize_mxfp6, bank.quantize_fp8):      # a second quantisation of either kind
        with pytest.raises(EkvError, match="quantised already|MXFP6 already"):
            again()
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
    assert bank.n_slots == [40] * L and bank.kv_quant == "mxfp6"
    with pytest.raises(EkvError):      # a RoPE-on-read decode step: refused by the dry run of the call itself
        bank.attend(StepPlan(policy="full", phase="decode", accumulate=False, streaming=True), q8[:, :, :1], k8[:, :, :1], k8[:, :, :1])
    assert bank.n_slots == [40] * L
    # before converting: other head dims, GQA factors above 4, RoPE-on-read banks, FP8 banks
    for d in (32, 64, 96):
        b2 = KVBank(1, 2, 2, d, cap=64)
        b2.lib = _NoCalls()
        with pytest.raises(EkvError, match="head_dim"):
            b2.quantize_mxfp6()
        assert b2.k is not None and b2.kv_quant is None
    b3 = KVBank(1, 10, 2, D, cap=64)
    b3.lib = _NoCalls()
    with pytest.raises(EkvError, match="GQA"):
        b3.quantize_mxfp6()
    assert b3.k is not None and b3.kv_quant is None
    b4 = KVBank(1, 2, 2, D, cap=64)
    b4.set_rope(*O.rope_tables(64, D))
    with pytest.raises(EkvError, match="RoPE-on-read"):
        b4.quantize_mxfp6()
    b5 = KVBank(1, 2, 2, D, cap=64).quantize_fp8()
    with pytest.raises(EkvError, match="quantised already"):
        b5.quantize_mxfp6()
    assert b5.kv_quant == "fp8"


class _Tok:
    eos_token_id = -1

    def decode(self, ids, skip_special_tokens=True):
        return " ".join(str(i) for i in ids)


def _tiny(kind, seed=0):
    """Two-layer HF model with head_dim 128 (4 query heads over 2 KV heads), bf16."""
    from transformers import LlamaConfig, LlamaForCausalLM, MistralConfig, MistralForCausalLM
    torch.manual_seed(seed)
    common = dict(vocab_size=97, hidden_size=256, intermediate_size=256, num_hidden_layers=2, num_attention_heads=4,
                  num_key_value_heads=2, head_dim=128, max_position_embeddings=512, attn_implementation="eager")
    if kind == "mistral":
        return MistralForCausalLM(MistralConfig(sliding_window=4096, **common)).to(BF).cuda().eval()
    return LlamaForCausalLM(LlamaConfig(**common)).to(BF).cuda().eval()


# ---- (d) end to end -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["llama", "mistral"])
def test_generate_with_kv_quant_mxfp6(kind):
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
        text, cache = run(mode, budget, stride, kv_quant="mxfp6")
        assert len(text.split()) == new, (mode, text)
        b = cache.bank
        assert cache.kv_quant == "mxfp6" and b.kv_quant == "mxfp6" and b.k is None
        assert cache.kv_bytes() == b.n_layers * b.n_kv_heads * b.cap * 200
        # greedy eager == hipGraph, token for token (the decode forward is captured after the conversion)
        text_g, cache_g = run(mode, budget, stride, kv_quant="mxfp6", hipgraph=True)
        assert text_g == text and cache_g.kv_quant == "mxfp6", mode


@pytest.mark.parametrize("policy,hq,h", [("roco", 4, 2), ("h2o_head", 4, 4), ("recency", 8, 2)], ids=["roco-gqa2", "h2o-mha", "recency-gqa4"])
def test_generate_on_the_fake_model_equals_its_step_by_step_twin(policy, hq, h):
    """generate(kv_quant='mxfp6') on the fake model (deterministic streams and logits) against the same run spelled out on a bank by
    hand: a dense 16-bit prefill, quantize_mxfp6() once at the prefill -> decode boundary, then one decode step per token through the
    calls the cache makes (one deferred attend per layer + one flush).  Same library calls on the same data, so everything is
    IDENTICAL: the tokens, the attention outputs of every forward, every evicted id, and at the end the four planes, the slot maps
    and the lengths.  A conversion at another point, rows read from a stale 16-bit tensor or planes of another format cannot pass."""
    import easykv_amd
    from easykv_amd import KVBank, StepPlan
    from oracle.fake_model import make_streams
    from tests.native_fake_model import NativeFakeModel
    L, n, budget, new = 2, 33, 40, 60
    streams = make_streams(L, hq, h, D, 128, seed=23)
    cfg = dict(budget=budget, kv_policy=policy, max_new_tokens=new, kv_quant="mxfp6", _record_evictions=True)
    model = NativeFakeModel(*streams)
    ids = torch.arange(n).view(1, -1) % 16
    with contextlib.redirect_stdout(io.StringIO()):
        text, cache = easykv_amd.generate(model, ids, cfg, kv_mode="decoding", stride=1, return_cache=True)
    b = cache.bank
    assert cache.kv_quant == "mxfp6" and b.kv_quant == "mxfp6" and b.k is None and b.v is None
    assert cache.kv_bytes() == b.n_layers * b.n_kv_heads * b.cap * 200
    assert len(text.split()) == new and len(model.outputs_log) == 1 + new

    # ---- the twin
    qs, ks, vs = model.qs, model.ks, model.vs      # [L, heads, positions, D] fp16 on the GPU
    scored = policy in K.SCORED
    twin = KVBank(L, hq, h, D, cap=b.cap)
    assert twin.cap == b.cap
    dense = StepPlan(policy="full", phase="prefill", accumulate=False)
    outs = [twin.attend(dense, qs[l:l + 1, :, :n], ks[l:l + 1, :, :n], vs[l:l + 1, :, :n], layer_begin=l)[0] for l in range(L)]
    assert torch.equal(torch.cat(outs).float().cpu(), model.outputs_log[0])
    if scored:
        twin.state_init(budget + 1, 0)
    twin.quantize_mxfp6()      # the boundary: every decode step below runs on MXFP6 rows
    evictions, positions = [], []
    for t in range(new):
        pos = n + t
        evict = (twin.n_slots[0] + 1 - n) > budget
        plan = StepPlan(policy=policy, phase="decode", accumulate=scored, evict=evict, score_off=n, budget=budget)
        positions.append(pos)
        if evict and policy == "recency":      # the oldest generated slot
            positions.pop(0)
            plan.range_start = n
        outs = [twin.attend(plan, qs[l:l + 1, :, pos:pos + 1], ks[l:l + 1, :, pos:pos + 1], vs[l:l + 1, :, pos:pos + 1], layer_begin=l, defer=True)[0]
                for l in range(L)]
        got = twin.flush()
        assert torch.equal(torch.cat(outs).float().cpu(), model.outputs_log[1 + t]), (policy, t)
        if evict:
            evictions.append(got.cpu())
    assert len(evictions) == new - budget == len(cache.evictions) > 0
    for t, (mine, theirs) in enumerate(zip(evictions, cache.evictions)):
        assert torch.equal(mine, torch.stack(list(theirs)).cpu()), (policy, t)
    assert twin.n_slots == b.n_slots == [n + budget] * L and twin.extent == b.extent
    assert torch.equal(twin.slot_of_pos, b.slot_of_pos)
    for name in ("k6", "v6", "k_exp", "v_exp"):
        assert torch.equal(getattr(twin, name), getattr(b, name)), name


# ---- (e) fidelity: recorded, not barred -------------------------------------------------------------------------------------------
def test_fidelity_of_a_quantised_bank_is_recorded():
    """The same prompt rows and the same 64 decode steps on a 16-bit bank and on its FP8, MXFP4 and MXFP6 twins, all against the oracle on the
    UNQUANTISED rows.  Recorded in profiles/kv6_fidelity.json; no pass mark for the quantised twins, the
    16-bit twin still meets its own bar."""
    from easykv_amd import KVBank, StepPlan
    from oracle import easykv_oracle as O
    L, hq, h, budget, steps = 2, 8, 8, 256, 64
    T = budget + 1
    result = {"shape": dict(layers=L, q_heads=hq, kv_heads=h, head_dim=D, budget=budget, steps=steps, rows="standard normal, fp16"), "policies": {}}
    for policy in ("roco", "h2o_head", "tova"):
        g = torch.Generator().manual_seed(21)
        k0, v0 = torch.randn(L, h, budget, D, generator=g).half(), torch.randn(L, h, budget, D, generator=g).half()
        warm = torch.rand(L, h, budget, generator=g) * 1e-3
        banks = {}
        for name in ("fp16", "fp8", "mxfp4", "mxfp6"):
            b = KVBank(L, hq, h, D, cap=T + 8)
            b.load_rows(k0.cuda(), v0.cuda())
            b.state_init(T, 0)
            b.score_sum[:, :, :budget] += warm.cuda()
            b.score_sq[:, :, :budget] += (warm ** 2).cuda()
            banks[name] = b
        for name in ("fp8", "mxfp4", "mxfp6"):
            banks[name].quantize(name)
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
    path = os.path.join(ROOT, "profiles", "kv6_fidelity.json")
    with open(path, "w") as f:
        json.dump(result, f, indent=1)
    back = json.load(open(path))
    for policy, r in back["policies"].items():
        for n in ("fp16", "fp8", "mxfp4", "mxfp6"):
            assert all(math.isfinite(x) for x in r[n].values()), (policy, n, r[n])
    print("[kv6-fidelity]", json.dumps(back["policies"]))
