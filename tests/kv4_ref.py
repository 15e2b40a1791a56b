"""The quantisation rule of the MXFP4 K/V rows (include/easykv_hip.h, "kv4") restated in torch, and the identity every
implementation of it is held to.  Runs on a CPU.

Rule of a block x[0..32), in fp32:  amax = max |x|;  e = the smallest integer with amax <= 6 * 2^e, clamped to [-126, 127], e = 0 for an
all-zero block;  byte = e + 127;  code = round-to-nearest(x / 2^e) onto {0, .5, 1, 1.5, 2, 3, 4, 6} with the sign of x, ties to the
even code.  Two codes per byte: element 2i in the low nibble, element 2i + 1 in the high nibble.  The quotient is exact (ldexp), so
the rule has no rounding of its own: two implementations agree bit for bit, up to the sign of zero (codes 0 and 8)."""
import torch

BLOCK = 32
GRID = torch.tensor([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])


def block_exp(x):
    """x [..., D] (finite) -> e int32 [..., D / 32] of the rule."""
    b = x.float().reshape(*x.shape[:-1], x.shape[-1] // BLOCK, BLOCK)
    amax = b.abs().amax(dim=-1)
    m, ex = torch.frexp(amax)                   # amax = m * 2^ex, m in [0.5, 1): amax <= 6 * 2^e = 0.75 * 2^(e + 3)
    e = ex - 3 + (m > 0.75).to(ex.dtype)
    e = e.clamp(-126, 127)
    return torch.where(amax == 0, torch.zeros_like(e), e).to(torch.int32)


def _code_index(y):
    """|y| <= 6 (fp32, exact quotients) -> index 0..7 of the nearest magnitude, ties to the even index."""
    a = y.abs()
    return ((a > 0.25).int() + (a >= 0.75).int() + (a > 1.25).int() + (a >= 1.75).int() + (a > 2.5).int() + (a >= 3.5).int() + (a > 5.0).int())


def quantize(x):
    """x [..., D] (any float dtype, finite; D a multiple of 32) -> (codes uint8 [..., D / 2], exponent bytes uint8 [..., D / 32])."""
    x = x.float()
    e = block_exp(x)
    b = x.reshape(*x.shape[:-1], x.shape[-1] // BLOCK, BLOCK)
    y = torch.ldexp(b, -e.unsqueeze(-1))        # exact
    idx = _code_index(y)
    code = (idx | (torch.signbit(y).int() << 3)).reshape(*x.shape)
    packed = (code[..., 0::2] | (code[..., 1::2] << 4)).to(torch.uint8)
    return packed, (e + 127).to(torch.uint8)


def unpack(codes):
    """codes uint8 [..., D / 2] -> the 4-bit codes int32 [..., D]."""
    c = codes.int()
    return torch.stack([c & 15, c >> 4], dim=-1).reshape(*codes.shape[:-1], codes.shape[-1] * 2)


def dequant(codes, exps):
    """codes uint8 [..., D / 2], exponent bytes uint8 [..., D / 32] -> fp32 values code * 2^(byte - 127) (exact)."""
    c = unpack(codes)
    mag = GRID[(c & 7).long()]
    val = torch.where((c & 8) != 0, -mag, mag)
    e = (exps.int() - 127).repeat_interleave(BLOCK, dim=-1)
    return torch.ldexp(val, e)


def same_codes(a, b):
    """Packed codes equal up to the sign of zero (codes 0 and 8 are equivalent)."""
    ca, cb = unpack(a.cpu()), unpack(b.cpu())
    ca = torch.where((ca & 7) == 0, torch.zeros_like(ca), ca)
    cb = torch.where((cb & 7) == 0, torch.zeros_like(cb), cb)
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
    exactly at 0.25, 0.75, 1.25, 1.75, 2.5, 3.5 and 5 times a power of two under a block maximum of exactly 6 * 2^e (1.25, 2.5 and 5
    must give 1, 2 and 4), and n rows whose blocks' maxima are exactly 6 * 2^e or 4 * 2^e among smaller random values."""
    from tests import kv8_ref
    base = kv8_ref.special_rows(n, d, gen, dtype)
    ties = torch.tensor([0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0, -1.25, -2.5, -5.0, -0.25, 6.0])
    tie = torch.zeros(n, d)
    edge = torch.zeros(n, d)
    for i in range(n):
        for b in range(d // BLOCK):
            p = float(2.0 ** int(torch.randint(-6, 7, (1,), generator=gen)))
            pick = ties[torch.randint(0, ties.numel(), (BLOCK,), generator=gen)]
            pick[int(torch.randint(0, BLOCK, (1,), generator=gen))] = 6.0      # the block maximum: exactly 6 * 2^e
            tie[i, b * BLOCK:(b + 1) * BLOCK] = pick * p
            blk = (torch.rand(BLOCK, generator=gen) * 2 - 1) * 3.9 * p
            blk[int(torch.randint(0, BLOCK, (1,), generator=gen))] = (6.0 if (i + b) % 2 == 0 else -4.0) * p
            edge[i, b * BLOCK:(b + 1) * BLOCK] = blk
    return torch.cat([base, tie.to(dtype), edge.to(dtype)])
