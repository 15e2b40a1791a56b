"""Every eviction decision of a long run at the headline shape (32 layers x 32 heads, head_dim 128, budget 2048, roco, scattered slot
map: what bench.py times), saved so that two libraries or two settings can be compared decision by decision:

    EASYKV_HIP_LIB=<parent's library> python tools/experiments/exp_rounds_decisions.py run a.pt [steps]
    python tools/experiments/exp_rounds_decisions.py run b.pt [steps]
    python tools/experiments/exp_rounds_decisions.py compare a.pt b.pt
    python tools/experiments/exp_rounds_decisions.py ties a.pt b.pt [out.txt]

`run` records the evicted id of every (step, layer, head), the attention outputs of steps 16 and the last, and the final slot map.
`compare` prints how many decisions differ, the first step at which any does, per-head counts of heads that ever differ, and the
output differences at the two recorded steps.
`ties` (run it under the settings that produced b.pt) repeats that run and, at the first step at which a head's decision in b differs
from a's, holds the decision to the tolerance-class rule of tests/test_hip_lockstep.py: the oracle's state of that layer is seeded from
the bank just before the step (ordered K / V rows and score rows), the oracle takes the step, and both decisions — this run's and
a's — must be the oracle's own or one of its answers under a +-2e-5 perturbation of its scores.  Up to its first differing step a
head has made the same decisions in both runs, so it holds the same rows in both and the seeded state stands for either.  The
repeated run must reproduce b's decisions (reading the state converts the score rows to the ordered layout and back)."""
import os, sys, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))


def setup():
    from easykv_amd import KVBank, StepPlan
    dev = torch.device("cuda")
    L = H = 32
    D, budget = 128, 2048
    T = budget + 1
    g = torch.Generator(device=dev).manual_seed(11)
    bank = KVBank(L, H, H, D, cap=T + 63, device=dev)
    bank.load_rows(torch.randn(L, H, budget, D, generator=g, device=dev).half(), torch.randn(L, H, budget, D, generator=g, device=dev).half())
    bank.slot_of_pos[:, :, :budget] = torch.argsort(torch.rand(L, H, budget, generator=g, device=dev), dim=-1).int()
    bank.state_init(T, 0)
    n_in = 64
    qs, ks, vs = (torch.randn(n_in, L, H, 1, D, generator=g, device=dev).half() for _ in range(3))
    o = torch.empty(L, H, 1, D, dtype=torch.float16, device=dev)
    ids = torch.empty(L, H, 1, dtype=torch.int32, device=dev)
    plan = StepPlan(policy="roco", phase="decode", evict=True, score_off=0, budget=budget)
    return bank, plan, qs, ks, vs, o, ids, n_in, budget


def run(out, steps=6144):
    bank, plan, qs, ks, vs, o, ids, n_in, budget = setup()
    L, H = bank.n_layers, bank.n_kv_heads
    dev = bank.device
    info = bank.step_info(plan, 1, phases=16)
    all_ids = torch.empty(steps, L, H, dtype=torch.int32, device=dev)
    outs = {}
    for i in range(steps):
        bank.attend(plan, qs[i % n_in], ks[i % n_in], vs[i % n_in], out=o, evict_ids=ids)
        all_ids[i] = ids[:, :, 0]
        if i in (15, steps - 1):
            outs[i + 1] = o.float().cpu()
        if i % 64 == 63:
            torch.cuda.synchronize()
    torch.cuda.synchronize()
    torch.save(dict(ids=all_ids.cpu(), outs=outs, slot_of_pos=bank._slot_of_pos.cpu(), info=info, slot_rows=list(bank._slot_rows)), out)
    print("saved", out, info)


def compare(a_path, b_path):
    a, b = torch.load(a_path), torch.load(b_path)
    print("plans:", a["info"], "|", b["info"])
    d = a["ids"] != b["ids"]
    steps = d.shape[0]
    print(f"decisions: {int(d.sum())} of {d.numel()} differ ({steps} steps x {d.shape[1] * d.shape[2]} heads)")
    if d.any():
        per_step = d.flatten(1).any(1).nonzero().flatten()
        heads = d.any(0)
        print(f"first step with a differing decision: {int(per_step[0]) + 1}; heads that ever differ: {int(heads.sum())} of {heads.numel()}")
        for n in (16, 4096, steps):
            print(f"  heads that have differed by step {n}: {int(d[:n].any(0).sum())}")
    for n in sorted(a["outs"]):
        x, y = a["outs"][n], b["outs"][n]
        ne = x != y
        print(f"attention outputs at step {n}: {int(ne.sum())} of {ne.numel()} elements differ, max |difference| {float((x - y).abs().max()):.3g}, "
              f"relative to max |out| {float((x - y).abs().max() / x.abs().max()):.3g}; heads with a differing element: {int(ne.flatten(2).any(2).sum())}")
    print("final slot maps equal:", bool(torch.equal(a["slot_of_pos"], b["slot_of_pos"])))


def ties(a_path, b_path, out=None):
    from oracle import easykv_oracle as O
    from tests.test_hip_lockstep import Hook
    a, b = torch.load(a_path), torch.load(b_path)
    d = a["ids"] != b["ids"]
    steps = d.shape[0]
    first = {}                                     # step -> [(layer, head)]: the first differing decision of every head that ever differs
    for l, h in d.any(0).nonzero().tolist():
        first.setdefault(int(d[:, l, h].nonzero()[0]), []).append((l, h))
    bank, plan, qs, ks, vs, o, ids, n_in, budget = setup()
    T = budget + 1
    oplan = O.StepPlan(policy="roco", phase="decode", evict=True, score_off=0, budget=budget)
    hook = Hook()
    lines, n_ok, n_heads, n_repro_bad = [], 0, 0, 0
    last = max(first) if first else -1
    O.SELECT_HOOK = hook
    try:
        for i in range(last + 1):
            seeded = {}
            if i in first:
                for l in sorted({l for l, _ in first[i]}):
                    kk, vv = bank.ordered_kv(l, 1)
                    st = O.LayerState(k=kk.float().cpu(), v=vv.float().cpu())
                    st.s, st.q, st.c = (x[l].cpu()[:, :T].clone() for x in (bank.score_sum, bank.score_sq, bank.score_cnt))
                    seeded[l] = st
                bank._slot_short = 0               # (a tool that reads the state is not the caller the thrash guard is for)
            bank.attend(plan, qs[i % n_in], ks[i % n_in], vs[i % n_in], out=o, evict_ids=ids)
            got = ids[:, :, 0].cpu().long()
            n_repro_bad += int((got != b["ids"][i].long()).sum())
            for l, st in seeded.items():
                q, k, v = (x[i % n_in][l:l + 1].float().cpu() for x in (qs, ks, vs))
                _, ids_ref = O.layer_step(st, q, k, v, oplan)
                for ll, h in first[i]:
                    if ll != l:
                        continue
                    mine, theirs, ref = int(got[l, h]), int(a["ids"][i, l, h]), int(ids_ref[h, 0])
                    ok_mine = mine == ref or hook.in_tolerance_class(h, torch.tensor([mine]))
                    ok_theirs = theirs == ref or hook.in_tolerance_class(h, torch.tensor([theirs]))
                    n_heads += 1
                    n_ok += int(ok_mine and ok_theirs)
                    lines.append(f"step {i + 1} layer {l} head {h}: this run evicts {mine}, the other {theirs}, the oracle {ref}; flagged unstable by the +-2e-5 probe: "
                                 f"{bool(hook.last['unstable'][h])}; in the tolerance class: this run {ok_mine}, the other {ok_theirs}")
                    print(lines[-1], flush=True)
    finally:
        O.SELECT_HOOK = None
    lines.append(f"{n_ok} of {n_heads} first differing decisions are ties by the tolerance-class rule (both answers in the oracle's class); "
                 f"{int(d.sum())} of {d.numel()} decisions differ over {steps} steps, {n_heads} heads ever; "
                 f"decisions of the repeated run that differ from the recorded one up to step {last + 1}: {n_repro_bad}")
    print(lines[-1])
    if out:
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return n_ok == n_heads and n_repro_bad == 0


if __name__ == "__main__":
    if sys.argv[1] == "ties":
        sys.exit(0 if ties(sys.argv[2], sys.argv[3], sys.argv[4] if len(sys.argv) > 4 else None) else 3)
    elif sys.argv[1] == "run":
        run(sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 6144)
    else:
        compare(sys.argv[2], sys.argv[3])
