"""The decode-step cases of the FP8-key / MXFP4-value ("kv84") tests and their seeded inputs, shared by the CPU precondition
(tests/test_kv84_cpu.py: the oracle alone, on rows quantised by tests/kv8_ref.py (K) and tests/kv4_ref.py (V)) and the GPU tests
(tests/test_hip_kv84.py).  The cases, the seed and the inputs are those of tests/kv6_cases.py (seed 5: every decision of the six scored
cases is well defined under this format too), so the three formats of 200 and 264 bytes are held to the same numbers.

TWIN_EXTRA: cases of the FP8-twin test alone (no oracle, so no precondition): the GQA factors the kv6 cases cannot have."""
import torch

from tests.kv6_cases import BF, D, F16, SCORED, SEED, STEPS, inputs, plan_kw, v_scale      # noqa: F401  (re-exported)

# same columns as STEPS
TWIN_EXTRA = [
    ("fused 8-wave ordered roco GQA8", 4, 32, 4, F16, 96, "roco", 0, False, False, (1, False), 16),
    ("fused 4-wave ordered h2o GQA8 bf16", 2, 16, 2, BF, 96, "h2o_head", 1, False, False, (1, False), 16),
    ("split tova GQA8", 2, 16, 2, F16, 300, "tova", 3, False, False, (0, True), 12),
    ("fused 4-wave ordered roco GQA2 bf16", 2, 4, 2, BF, 96, "roco", 1, False, False, (1, False), 16),
]


def quantize_ref(k, v):
    """(K codes, K scales, V codes, V exponent bytes) of rows k, v [..., 128] by the two rules' restatements."""
    from tests import kv4_ref, kv8_ref
    kc, ks = kv8_ref.quantize(k)
    vc, ve = kv4_ref.quantize(v)
    return kc, ks, vc, ve


def dequant_ref(k, v):
    """What a kv84 bank holds of rows k, v, as fp32: K through the kv8 rule, V through the kv4 rule."""
    from tests import kv4_ref, kv8_ref
    return kv8_ref.dequant(*kv8_ref.quantize(k)), kv4_ref.dequant(*kv4_ref.quantize(v))


def spread_rows(n, gen, dtype=torch.float16, lo=-6):
    """n rows [128] whose four 32-element blocks differ in magnitude by 2^4 per block (block b: values within +-2^(4 b + lo)), in a
    per-row random order of the blocks: a V exponent byte taken from the wrong block is an error of a factor >= 16."""
    x = torch.zeros(n, 128)
    for i in range(n):
        order = torch.randperm(4, generator=gen)
        for b in range(4):
            x[i, 32 * b:32 * b + 32] = (torch.rand(32, generator=gen) * 2 - 1) * 2.0 ** (4 * int(order[b]) + lo)
    return x.to(dtype)
