"""Child process of tests/test_hip_twin_bank.py: the benched decode state (tests/test_hip_lockstep.py: Llama2-7B head shape, budget
2048, scattered slot map, roco, slot-indexed score rows) for 24 evicting steps on whichever one-launch instance EKV_FUSED_NW in the
environment selects, held to the oracle step by step with that test's bars: outputs within tests/golden_util.out_close, every
decision equal to the oracle's or one of its answers under a +-2e-5 perturbation (the tolerance class), final state as there.

    python -m tests.twin_bank_run OUT.pt"""
import sys

import torch


def main(out_path):
    from easykv_amd import StepPlan
    from oracle import easykv_oracle as O
    from tests.golden_util import out_close
    from tests.test_hip_lockstep import Hook, _scattered_bank, _seed_states
    L, H, D, budget, steps = 2, 32, 128, 2048, 24
    T = budget + 1
    g = torch.Generator().manual_seed(78)
    bank = _scattered_bank(L, H, H, D, budget, T + 63, g)
    bank.state_init(T, 0)
    warm = torch.rand(L, H, budget, generator=g) * 1e-3
    bank.score_sum[:, :, :budget] += warm.cuda()
    bank.score_sq[:, :, :budget] += (warm ** 2).cuda()
    states = _seed_states(bank, T)
    plan = StepPlan(policy="roco", phase="decode", evict=True, score_off=0, budget=budget, n_split=1)
    oplan = O.StepPlan(policy="roco", phase="decode", evict=True, score_off=0, budget=budget)
    assert bank.step_plan(plan, 1)[1]
    hook = Hook()
    n_dec = n_exact = n_class = n_slot_steps = 0
    outs, all_ids, n_reseed = [], [], 0
    O.SELECT_HOOK = hook
    try:
        for i in range(steps):
            q, k, v = (torch.randn(L, H, 1, D, generator=g).half() for _ in range(3))
            out, ids = bank.attend(plan, q.cuda(), k.cuda(), v.cuda())
            n_slot_steps += int(all(bank._slot_rows))
            got = ids[:, :, 0].cpu().long()
            outs.append(out.cpu())
            all_ids.append(got)
            reseed = []
            for l in range(L):
                o_ref, ids_ref = O.layer_step(states[l], q[l:l + 1].float(), k[l:l + 1].float(), v[l:l + 1].float(), oplan)
                assert out_close(out[l].float().cpu(), o_ref[0]), (i, l)
                same = got[l] == ids_ref[:, 0]
                n_dec += H
                n_exact += int(same.sum())
                for hh in (~same).nonzero().flatten().tolist():
                    assert hook.in_tolerance_class(hh, got[l, hh:hh + 1]), (i, l, hh)
                    n_class += 1
                    reseed.append(l)
            if reseed:      # the oracle's copy of those layers follows the bank again, as in the lockstep test
                n_reseed += 1
                fresh = _seed_states(bank, T)
                for l in set(reseed):
                    states[l] = fresh[l]
                    states[l].s, states[l].q, states[l].c = states[l].s[:, :T], states[l].q[:, :T], states[l].c[:, :T]
                bank._slot_short = 0
    finally:
        O.SELECT_HOOK = None
    assert n_exact + n_class == n_dec and n_exact >= 0.98 * n_dec, (n_exact, n_class, n_dec)
    assert n_slot_steps >= steps - 2 * n_reseed - 1, (n_slot_steps, n_reseed)
    info = bank.step_info(plan, 1, phases=16)      # (before the state is read back in the ordered layout)
    # final state of the layers, with the bars of the lockstep test
    kk, vv = bank.ordered_kv()
    S2, C2 = bank.score_sum.cpu(), bank.score_cnt.cpu()
    for l in range(L):
        assert torch.equal(kk[l].cpu(), states[l].k[0].half()) and torch.equal(vv[l].cpu(), states[l].v[0].half())
        assert torch.equal(C2[l, :, :budget], states[l].c[:, :budget])
        rel = ((S2[l, :, :budget] - states[l].s[:, :budget]).abs() / states[l].s[:, :budget].abs().clamp_min(1e-6)).max()
        assert float(rel) <= 1e-4, float(rel)
    torch.save(dict(outs=torch.stack(outs), ids=torch.stack(all_ids), n_dec=n_dec, n_exact=n_exact, n_class=n_class, n_reseed=n_reseed,
                    n_slot_steps=n_slot_steps, steps=steps, info=info), out_path)


if __name__ == "__main__":
    main(sys.argv[1])
