"""The quantisation rule of the MXFP6 K/V rows (include/easykv_hip.h, "kv6") restated in torch, and the identity every
implementation of it is held to.  Runs on a CPU.

Rule of a block x[0..32), in fp32:  amax = max |x|;  e = the smallest integer with amax <= 7.5 * 2^e, clamped to [-126, 127], e = 0 for
an all-zero block;  byte = e + 127;  code = round-to-nearest(x / 2^e) onto the 32 e2m3 magnitudes with the sign of x (bit 5), ties to
the even code.  Element j of a block sits at bits [6j, 6j + 6) of the block's 24 bytes read as one little-endian integer (the order
the gfx950 pk32 conversions read, as measured on the part).  The quotient is exact (ldexp), so the rule has no rounding of its own:
two implementations agree bit for bit, up to the sign of zero (codes 0 and 32)."""
import torch

BLOCK = 32
BLOCK_BYTES = 24
# magnitude index i -> value: i / 8 below 1 (subnormals), (1 + (i & 7) / 8) * 2^((i >> 3) - 1) from 1 on
GRID = torch.tensor([i / 8 if i < 8 else (1 + (i & 7) / 8) * 2.0 ** ((i >> 3) - 1) for i in range(32)])


def block_exp(x):
    """x [..., D] (finite) -> e int32 [..., D / 32] of the rule."""
    b = x.float().reshape(*x.shape[:-1], x.shape[-1] // BLOCK, BLOCK)
    amax = b.abs().amax(dim=-1)
    m, ex = torch.frexp(amax)                   # amax = m * 2^ex, m in [0.5, 1): amax <= 7.5 * 2^e = 0.9375 * 2^(e + 3)
    e = ex - 3 + (m > 0.9375).to(ex.dtype)
    e = e.clamp(-126, 127)
    return torch.where(amax == 0, torch.zeros_like(e), e).to(torch.int32)


def _code_index(y):
    """|y| <= 7.5 (fp32, exact quotients) -> index 0..31 of the nearest magnitude, ties to the even index: the index is the number of
    midpoints below |y|, a midpoint above an even index counting only when it is exceeded."""
    a = y.abs()
    idx = torch.zeros_like(a, dtype=torch.int32)
    for i in range(31):
        mid = float(GRID[i] + GRID[i + 1]) / 2
        idx += (a > mid).int() if i % 2 == 0 else (a >= mid).int()
    return idx


def pack(code):
    """6-bit codes int [..., D] -> uint8 [..., 3 * D / 4]: four codes per three bytes, little-endian."""
    c = code.int().reshape(*code.shape[:-1], code.shape[-1] // 4, 4)
    w = c[..., 0] | (c[..., 1] << 6) | (c[..., 2] << 12) | (c[..., 3] << 18)
    out = torch.stack([w & 255, (w >> 8) & 255, (w >> 16) & 255], dim=-1)
    return out.reshape(*code.shape[:-1], code.shape[-1] * 3 // 4).to(torch.uint8)


def unpack(codes):
    """codes uint8 [..., 3 * D / 4] -> the 6-bit codes int32 [..., D]."""
    b = codes.int().reshape(*codes.shape[:-1], codes.shape[-1] // 3, 3)
    w = b[..., 0] | (b[..., 1] << 8) | (b[..., 2] << 16)
    out = torch.stack([w & 63, (w >> 6) & 63, (w >> 12) & 63, (w >> 18) & 63], dim=-1)
    return out.reshape(*codes.shape[:-1], codes.shape[-1] * 4 // 3)


def quantize(x):
    """x [..., D] (any float dtype, finite; D a multiple of 32) -> (codes uint8 [..., 3 * D / 4], exponent bytes uint8 [..., D / 32])."""
    x = x.float()
    e = block_exp(x)
    b = x.reshape(*x.shape[:-1], x.shape[-1] // BLOCK, BLOCK)
    y = torch.ldexp(b, -e.unsqueeze(-1))        # exact
    code = (_code_index(y) | (torch.signbit(y).int() << 5)).reshape(*x.shape)
    return pack(code), (e + 127).to(torch.uint8)


def dequant(codes, exps):
    """codes uint8 [..., 3 * D / 4], exponent bytes uint8 [..., D / 32] -> fp32 values code * 2^(byte - 127) (exact)."""
    c = unpack(codes)
    mag = GRID[(c & 31).long()]
    val = torch.where((c & 32) != 0, -mag, mag)
    e = (exps.int() - 127).repeat_interleave(BLOCK, dim=-1)
    return torch.ldexp(val, e)


def same_codes(a, b):
    """Packed codes equal up to the sign of zero (codes 0 and 32 are equivalent)."""
    ca, cb = unpack(a.cpu()), unpack(b.cpu())
    ca = torch.where((ca & 31) == 0, torch.zeros_like(ca), ca)
    cb = torch.where((cb & 31) == 0, torch.zeros_like(cb), cb)
    return torch.equal(ca, cb)


def check_rows(x, codes, exps, what=""):
    """Assert that stored codes / exponent bytes of rows x [..., D] ARE the rule's: exponents equal, codes equal up to +-0."""
    want_c, want_e = quantize(x.float().cpu())
    exps, codes = exps.cpu(), codes.cpu()
    assert bool((exps != 255).all()), (what, "exponent byte 255")
    bad = (exps != want_e).nonzero()
    assert bad.numel() == 0, (what, "block exponents differ from the rule", bad[:4].tolist(), exps[tuple(bad[0])].item() if bad.numel() else None)
    assert same_codes(codes, want_c), (what, "codes differ from the rule", int((unpack(codes) != unpack(want_c)).sum()))


def special_rows(n, d, gen, dtype=torch.float16):
    """tests.kv8_ref.special_rows' kinds (random normal, all-zero, one outlier, tiny magnitude), n rows each, plus n tie rows: values
    exactly half way between two neighbours of the grid, times a power of two, under a block maximum of exactly 7.5 * 2^e (1.9375, 3.875
    and 0.0625 must give 2, 4 and 0), and n rows whose blocks' maxima are exactly 7.5 * 2^e or 4 * 2^e among smaller random values.
    Every value has at most 6 significant bits, so fp16 and bf16 hold it exactly."""
    from tests import kv8_ref
    base = kv8_ref.special_rows(n, d, gen, dtype)
    ties = torch.tensor([0.0625, 0.1875, 0.9375, 1.0625, 1.9375, 2.125, 2.375, 3.875, 4.25, 4.75, 7.25, -0.0625, -1.9375, -3.875, -7.25, 7.5])
    tie = torch.zeros(n, d)
    edge = torch.zeros(n, d)
    for i in range(n):
        for b in range(d // BLOCK):
            p = float(2.0 ** int(torch.randint(-6, 7, (1,), generator=gen)))
            pick = ties[torch.randint(0, ties.numel(), (BLOCK,), generator=gen)]
            pick[int(torch.randint(0, BLOCK, (1,), generator=gen))] = 7.5      # the block maximum: exactly 7.5 * 2^e
            tie[i, b * BLOCK:(b + 1) * BLOCK] = pick * p
            blk = (torch.rand(BLOCK, generator=gen) * 2 - 1) * 3.9 * p
            blk[int(torch.randint(0, BLOCK, (1,), generator=gen))] = (7.5 if (i + b) % 2 == 0 else -4.0) * p
            edge[i, b * BLOCK:(b + 1) * BLOCK] = blk
    return torch.cat([base, tie.to(dtype), edge.to(dtype)])
