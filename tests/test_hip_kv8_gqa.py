"""FP8 rows at GQA factors 5 .. 16 on the GPU: the MFMA decode kernel behind KVBank.quantize_fp8(grouped=True) against the CPU oracle ON
THE BANK'S OWN CONTENTS, by the scheme and under the bars of tests/test_hip_kv8.py.  Cases and inputs: tests/test_kv8_gqa_cpu.py."""
import contextlib
import io

import pytest
import torch

from tests import kv4_cases as K
from tests import kv8_ref as R
from tests.golden_util import out_close
from tests.test_hip_fullsize import Probe
from tests.test_hip_kv4_gqa import _step
from tests.test_hip_kv8 import _Tok, _oracle_states
from tests.test_kv8_gqa_cpu import CASES, inputs

pytestmark = pytest.mark.gpu


def _bank(case, grouped=True):
    """The case's bank, its physical rows permuted (a fragmented slot map, live rows all over the bank), its workspace pre-filled."""
    from easykv_amd import KVBank
    name, L, hq, h, dtype, budget, policy, n_split, defer, slot, D, steps = case
    k0, v0, warm, _ = inputs(case)
    bank = KVBank(L, hq, h, D, cap=budget + 1 + steps + 8, dtype=dtype)
    bank.load_rows(k0.cuda(), v0.cuda())
    if policy in K.SCORED:
        bank.state_init(budget + 1, 0)
        bank.score_sum[:, :, :budget] += warm.cuda()
        bank.score_sq[:, :, :budget] += (warm ** 2).cuda()
    g = torch.Generator().manual_seed(17)
    perm = torch.stack([torch.randperm(bank.cap, generator=g) for _ in range(L * h)]).view(L, h, bank.cap).cuda()
    idx = perm.unsqueeze(-1).expand(-1, -1, -1, D)
    for rows_ in (bank.k, bank.v):      # position j's row now lives in physical row perm[j]; the rows of no position are zeros
        rows_[:, :, budget:] = 0
        rows_.copy_(torch.zeros_like(rows_).scatter_(2, idx, rows_))
    bank._slot_of_pos.copy_(perm.int())
    bank.extent = [bank.cap] * L
    bank._workspace(1 << 24).view(torch.float32).fill_(3.0)
    return bank.quantize_fp8(grouped=True) if grouped else bank.quantize_fp8()


_planes = lambda bank: [x.clone() for x in (bank.k8, bank.v8, bank.k_scale, bank.v_scale)]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_decode_steps_against_the_oracle_on_the_banks_own_contents(case):
    from easykv_amd import StepPlan
    from oracle import easykv_oracle as O
    name, L, hq, h, dtype, budget, policy, n_split, defer, slot, D, steps = case
    scored, evict, T = policy in K.SCORED, policy != "full", budget + 1
    bank = _bank(case)
    twin = _bank(case) if defer else None      # the immediate form of a deferred case, on the same rows
    assert bank.kv_quant == "fp8" and bank.kv_grouped and bank.k is None and bank._attend_fn is bank.lib.ekv_kv8_gqa_step_attend
    kw = K.plan_kw(case)
    info = bank.step_info(StepPlan(n_split=n_split, **kw), 1, 0, 1 if defer else L, phases=5 if defer else 0)
    assert info["fused"] == 0 and info["n_split"] == (3 if n_split == 3 else 1) and info["n_launches"] >= 1, info
    states = _oracle_states(bank, T, range(L))
    O.SELECT_HOOK = probe = Probe()
    n_dec = n_stable = 0
    rows = torch.arange(h)
    try:
        for i, (q, k, v, rs) in enumerate(inputs(case)[3]):
            plan = StepPlan(n_split=n_split, range_start=rs, **kw)
            new_row = torch.stack([bank._slot_of_pos[l, :, bank.n_slots[0]] for l in range(L)]).cpu().long()
            before = _planes(bank)
            out, ids = _step(bank, plan, q, k, v, defer)
            if twin is not None:      # deferred and immediate: the same bits
                out_t, ids_t = _step(twin, plan, q, k, v, False)
                assert torch.equal(out.view(torch.int16), out_t.view(torch.int16)) and torch.equal(ids, ids_t), (name, i)
            for b4, now in zip(before, _planes(bank)):      # rows no step names stay bit-equal
                keep = torch.ones(L, h, bank.cap, dtype=torch.bool, device="cuda")
                keep[torch.arange(L).view(-1, 1), rows.view(1, -1), new_row] = False
                assert torch.equal(b4[keep], now[keep]), (name, i)
            reseed = []
            for l in range(L):
                for given, codes, sc in ((k[l, :, 0], bank.k8[l], bank.k_scale[l]), (v[l, :, 0], bank.v8[l], bank.v_scale[l])):
                    R.check_rows(given, codes[rows, new_row[l]], sc[rows, new_row[l]], (name, i, l))
                kd, vd = bank.dequantized_rows(l)
                kq, vq = kd[rows, new_row[l]].cpu().view(1, h, 1, D), vd[rows, new_row[l]].cpu().view(1, h, 1, D)
                o_ref, ids_ref = O.layer_step(states[l], q[l:l + 1].float(), kq, vq, O.StepPlan(range_start=rs, **kw))
                assert bool(torch.isfinite(out[l]).all()) and out_close(out[l].float().cpu(), o_ref[0]), (name, i, l, float((out[l].float().cpu() - o_ref[0]).abs().max()))
                if not scored:
                    continue
                unstable, same = probe.last_unstable, ids[l, :, 0].cpu().long() == ids_ref[:, 0]
                n_dec += h
                n_stable += int((~unstable).sum())
                assert bool(same[~unstable].all()), (name, i, l)      # a well-defined decision: identical
                if not bool(same.all()):
                    reseed.append(l)
                    continue
                # the same victims: slot map and score rows (rtol / atol: tests/test_hip_kv4_gqa.py derives them for the MFMA's fp32 sum)
                now_st = _oracle_states(bank, budget, [l])[l]
                assert torch.equal(now_st.k, states[l].k) and torch.equal(now_st.v, states[l].v), (name, i, l)
                assert torch.allclose(now_st.s, states[l].s[:, :budget], rtol=1e-4, atol=1e-6), (name, i, l)
                assert torch.allclose(now_st.q, states[l].q[:, :budget], rtol=2e-4, atol=1e-6), (name, i, l)
            if reseed:      # an ill-defined decision went the other way: the oracle follows the bank from here
                states.update(_oracle_states(bank, T, reseed))
    finally:
        O.SELECT_HOOK = None
    if scored:
        assert n_stable >= 0.9 * n_dec, (n_stable, n_dec)
    assert bank.n_slots == [budget + (0 if evict else steps)] * L


def test_rep4_grouped_bank_is_the_plain_fp8_bank_bit_for_bit():
    """GQA x 4: a grouped call IS the kv8 call — outputs, victims and every plane, over three steps of a split and a one-launch plan."""
    from easykv_amd import StepPlan
    for n_split in (0, 3):
        case = ("rep4 twin", 2, 8, 2, torch.float16, 300, "roco", n_split, False, False, 128, 3)
        a, b, kw = _bank(case, grouped=True), _bank(case, grouped=False), K.plan_kw(case)
        assert a.kv_grouped and not b.kv_grouped
        assert a.step_info(StepPlan(n_split=n_split, **kw), 1) == b.step_info(StepPlan(n_split=n_split, **kw), 1)
        for q, k, v, rs in inputs(case)[3]:
            plan = StepPlan(n_split=n_split, range_start=rs, **kw)
            (oa, ia), (ob, ib) = _step(a, plan, q, k, v, False), _step(b, plan, q, k, v, False)
            assert torch.equal(oa.view(torch.int16), ob.view(torch.int16)) and torch.equal(ia, ib)
            assert all(torch.equal(x, y) for x, y in zip(_planes(a) + [a.score_sum, a.slot_of_pos], _planes(b) + [b.score_sum, b.slot_of_pos]))
        with pytest.raises(Exception, match="chunk"):      # a refused call leaves flag and calls as they were
            a.quantize_fp8(chunks=True, grouped=True)
        assert a.kv_grouped and a._attend_fn is a.lib.ekv_kv8_gqa_step_attend and b._attend_fn is b.lib.ekv_kv8_step_attend
    from easykv_amd import KVBank, _lib
    wide = KVBank(1, 34, 2, 128, cap=16, dtype=torch.float16)      # GQA x 17: the conversion is refused and the flag goes back to False
    wide.load_rows(*(torch.randn(1, 2, 4, 128).half().cuda() for _ in range(2)))
    was = wide._attend_fn
    with pytest.raises(_lib.EkvError, match="GQA factors up to 16, not 17"):
        wide.quantize_fp8(grouped=True)
    assert not wide.kv_grouped and wide.kv_quant is None and wide.k is not None and wide._attend_fn is was


def test_generate_runs_a_gqa8_model_with_and_without_the_key():
    import easykv_amd
    from easykv_amd import hf
    from transformers import LlamaConfig, LlamaForCausalLM
    torch.manual_seed(0)
    cfg = LlamaConfig(vocab_size=97, hidden_size=256, intermediate_size=256, num_hidden_layers=2, num_attention_heads=8, num_key_value_heads=1,
                      head_dim=128, max_position_embeddings=512, attn_implementation="eager")
    model = hf.patch_model(LlamaForCausalLM(cfg).to(torch.bfloat16).cuda().eval())
    ids = torch.randint(0, 97, (1, 40), device="cuda", generator=torch.Generator(device="cuda").manual_seed(3))
    easykv_amd.enable_fixed_kv(model, _Tok(), mode="decoding", stride=1)
    gen = dict(temperature=1e-6, kv_policy="roco", budget=8, max_new_tokens=12, eos_token_ids=[-1], kv_dtype="auto", kv_quant="fp8")
    with contextlib.redirect_stdout(io.StringIO()):      # without the key: the plain FP8 calls, as before
        text, cache = model.easykv_generate(input_ids=ids, generation_config=gen, return_cache=True)
    assert len(text.split()) == 12 and cache.bank.kv_quant == "fp8" and not cache.bank.kv_grouped
    texts = []
    for graph in (False, True):      # greedy eager == hipGraph, token for token (the capture comes after the conversion)
        torch.manual_seed(11)
        with contextlib.redirect_stdout(io.StringIO()):
            text, cache = model.easykv_generate(input_ids=ids, generation_config=dict(gen, kv_quant_gqa=True, hipgraph=graph), return_cache=True)
        assert len(text.split()) == 12 and cache.bank.kv_quant == "fp8" and cache.bank.kv_grouped and cache.bank.k is None
        texts.append(text)
    assert texts[0] == texts[1]
