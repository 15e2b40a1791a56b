"""The quantisation rule of the FP8 K/V rows (include/easykv_hip.h, "kv8") restated in torch, and the properties every
implementation of it must have.  Runs on a CPU.

Rule of a row x:  amax = max |x| over the row, in fp32;  s = amax / 448  (s = 1 when amax == 0);  code = RNE(x / s) as OCP e4m3fn."""
import torch

FP8 = torch.float8_e4m3fn
FP8_MAX = 448.0


def quantize(x):
    """x [..., D] (any float dtype, finite) -> (codes uint8 [..., D], scales fp32 [...])."""
    x = x.float()
    amax = x.abs().amax(dim=-1)
    s = torch.where(amax == 0, torch.ones_like(amax), amax / FP8_MAX)
    codes = (x / s.unsqueeze(-1)).to(FP8)
    return codes.view(torch.uint8), s


def dequant(codes, s):
    """codes uint8 [..., D], scales fp32 [...] -> fp32 values code * scale."""
    return codes.view(FP8).float() * s.float().unsqueeze(-1)


def _grid():
    """All finite e4m3fn values, ascending (float64)."""
    v = torch.arange(256, dtype=torch.uint8).view(FP8).float()
    return torch.sort(torch.unique(v[torch.isfinite(v)]).double())[0]


GRID = _grid()


def nearest_gap(y):
    """Distance (float64) from each y to the nearest representable e4m3fn value."""
    y = y.double()
    i = torch.searchsorted(GRID, y.contiguous()).clamp(1, GRID.numel() - 1)
    return torch.minimum((y - GRID[i - 1]).abs(), (GRID[i] - y).abs())


def check_rows(x, codes, s, what=""):
    """Assert the quantiser properties of rows x [..., D] against stored codes (uint8) and scales (fp32):
      * the scale is within one fp32 ulp of amax / 448 and never smaller than amax / 448 * (1 - 2^-23); 1 for an all-zero row;
      * |x| <= 448 * s up to the rounding of the scale, so nothing saturates;
      * every code is A nearest representable value to the fp32 quotient x / s (ties either way)."""
    x, s = x.float().cpu(), s.float().cpu()
    codes = codes.cpu()
    amax = x.abs().amax(dim=-1)
    want = amax / FP8_MAX
    zero = amax == 0
    assert bool((s[zero] == 1.0).all()), what
    nz = ~zero
    ulp = torch.ldexp(torch.ones_like(want), torch.frexp(want)[1] - 24)      # one ulp of `want` (normal range)
    assert bool(((s[nz] - want[nz]).abs() <= ulp[nz]).all()), (what, "scale off by more than one ulp")
    assert bool((s[nz].double() >= want[nz].double() * (1 - 2.0 ** -23)).all()), (what, "scale too small")
    assert bool((x.abs().double() <= FP8_MAX * s.double().unsqueeze(-1) * (1 + 2.0 ** -22)).all()), what
    val = codes.view(FP8).float()
    assert bool(torch.isfinite(val).all()), (what, "a NaN code")
    y = x / s.unsqueeze(-1)                     # the rule's fp32 quotient
    err = (val.double() - y.double()).abs()
    assert bool((err <= nearest_gap(y)).all()), (what, "a code that is not a nearest e4m3fn value", float((err - nearest_gap(y)).max()))


def special_rows(n, d, gen, dtype=torch.float16):
    """n rows of each kind: random normal, all-zero, one outlier, tiny magnitude."""
    rnd = torch.randn(n, d, generator=gen)
    zero = torch.zeros(n, d)
    out = torch.randn(n, d, generator=gen) * 0.05
    out[torch.arange(n), torch.randint(0, d, (n,), generator=gen)] = 300.0 * torch.sign(torch.randn(n, generator=gen))
    tiny = torch.randn(n, d, generator=gen) * (1e-6 if dtype is torch.float16 else 1e-20)
    return torch.cat([rnd, zero, out, tiny]).to(dtype)
