"""The decode-step cases of the MXFP6 ("kv6") tests and their seeded inputs, shared by the CPU precondition (tests/test_kv6_cpu.py: the
oracle alone, on rows quantised by tests/kv6_ref.py) and the GPU test (tests/test_hip_kv6.py: the kernels against the oracle on the
bank's own contents).  Both draw from `inputs`, so the precondition is about the very numbers the GPU test runs on."""
import torch

BF, F16 = torch.bfloat16, torch.float16
SEED = 5      # (a seed that misses the 90 % cap of well-defined decisions is changed here; the cap is not)
SCORED = ("roco", "h2o_head", "tova")

# name, L, hq, h, dtype, budget, policy, n_split, defer, slot rows, expect (fused, split), steps — all head_dim 128
STEPS = [
    ("fused 8-wave slot-indexed roco", 32, 8, 8, F16, 96, "roco", 0, False, True, (1, False), 48),
    ("fused 8-wave ordered h2o GQA4 bf16", 32, 32, 8, BF, 96, "h2o_head", 0, False, False, (1, False), 44),
    ("fused 4-wave slot-indexed tova GQA3", 4, 12, 4, F16, 96, "tova", 1, False, True, (1, False), 44),
    ("split roco", 2, 4, 4, F16, 300, "roco", 3, False, False, (0, True), 24),
    ("split tova GQA4 bf16", 2, 8, 2, BF, 300, "tova", 3, False, False, (0, True), 24),
    ("fused recency bf16", 32, 8, 8, BF, 96, "recency", 0, False, False, (1, False), 12),
    ("fused random GQA2", 2, 4, 2, F16, 96, "random", 1, False, False, (1, False), 12),
    ("fused full GQA4", 2, 8, 2, F16, 96, "full", 1, False, False, (1, False), 12),
    ("split recency", 2, 4, 4, F16, 300, "recency", 3, False, False, (0, True), 12),
    ("split random GQA4 bf16", 2, 8, 2, BF, 300, "random", 3, False, False, (0, True), 12),
    ("split full", 2, 4, 4, F16, 300, "full", 3, False, False, (0, True), 12),
    ("deferred roco GQA2", 4, 4, 2, F16, 96, "roco", 0, True, False, (0, False), 44),
]
D = 128


def v_scale(dtype):
    """bf16 I/O draws V at 1/4 scale, for the reason tests/test_hip_kv8.py gives: the flat output bar then applies to both types."""
    return 0.25 if dtype is BF else 1.0


def inputs(case):
    """(k0, v0, warm or None, generator of per-step (q, k, v, range_start)) of a case, in the case's 16-bit type."""
    name, L, hq, h, dtype, budget, policy, n_split, defer, slot, expect, steps = case
    g = torch.Generator().manual_seed(SEED)
    vs = v_scale(dtype)
    k0 = torch.randn(L, h, budget, D, generator=g).to(dtype)
    v0 = (torch.randn(L, h, budget, D, generator=g) * vs).to(dtype)
    warm = torch.rand(L, h, budget, generator=g) * 1e-3 if policy in SCORED else None

    def per_step():
        for _ in range(steps):
            q = torch.randn(L, hq, 1, D, generator=g).to(dtype)
            k = torch.randn(L, h, 1, D, generator=g).to(dtype)
            v = (torch.randn(L, h, 1, D, generator=g) * vs).to(dtype)
            rs = -1
            if policy == "recency":
                rs = 4
            elif policy == "random":
                rs = int(torch.randint(0, budget - 1, (1,), generator=g))
            yield q, k, v, rs
    return k0, v0, warm, per_step()


def plan_kw(case):
    policy, budget = case[6], case[5]
    return dict(policy=policy, phase="decode", evict=policy != "full", accumulate=policy in SCORED, score_off=0, budget=budget)
