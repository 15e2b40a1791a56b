"""The P / V representations considered for the PV MFMA of the MXFP4 GQA kernel (ekv_attn_decode_mxg.inc; DESIGN.md §8, "MXFP4 at GQA > 4"),
emulated on the CPU over the first step of the cases of tests/test_kv4_gqa_cpu.py: rows quantised by tests/kv4_ref.py, logits and the
reference output in float64, p = exp(s - max) rounded to fp32 as the kernel holds it, then per candidate the operands rounded as the
candidate stores them and the products summed in float64 (so that only the REPRESENTATION differs, not the summation order):

  a  V = code * 2^e in bf16 (exact), P = bf16 hi + bf16 lo                      (the build)
  b  V as in a, P = one bf16
  c  V = fp16(code * 2^e * 2^-OFF), P = one fp16, the sum times 2^OFF           (OFF = 2: 6 * 2^14 * 2^-2 fits fp16)

Prints max |out - float64| per case and candidate, and whether every element meets tests.golden_util.out_close.
Usage: python tools/experiments/mxg_p_candidates.py"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tests import kv4_ref as R  # noqa: E402
from tests.golden_util import out_close  # noqa: E402
from tests.test_kv4_gqa_cpu import CASES, inputs  # noqa: E402

OFF = 2


def main():
    bf, hf, f64 = torch.bfloat16, torch.float16, torch.float64
    for case in CASES:
        name, L, hq, h, dtype = case[:5]
        k0, v0, _, steps = inputs(case)
        q, k1, v1, _ = next(iter(steps))
        deq = lambda x: R.dequant(*R.quantize(x.float().reshape(-1, 128))).reshape(x.shape).to(f64)
        k, v = deq(torch.cat([k0, k1], 2)), deq(torch.cat([v0, v1], 2))      # [L, h, T, 128], the appended row quantised too
        rep = hq // h
        s = torch.einsum("lhrd,lhtd->lhrt", q.to(f64).view(L, h, rep, 128), k) / 128 ** 0.5
        p = torch.exp(s - s.amax(-1, keepdim=True)).float()      # what the kernel holds: fp32
        ref = torch.einsum("lhrt,lhtd->lhrd", torch.softmax(s, -1), v)
        den = p.to(f64).sum(-1, keepdim=True)
        hi = p.to(bf)
        lo = (p - hi.float()).to(bf)
        cands = {"a": ((hi.to(f64) + lo.to(f64)), v.to(bf).to(f64), 1.0), "b": (hi.to(f64), v.to(bf).to(f64), 1.0),
                 "c": (p.to(hf).to(f64), (v * 2.0 ** -OFF).to(hf).to(f64), 2.0 ** OFF)}
        line = []
        for c, (pp, vv, scale) in cands.items():
            out = (torch.einsum("lhrt,lhtd->lhrd", pp, vv) * scale / den).to(dtype)      # rounded to the output type, as the fold does
            err = float((out.to(f64) - ref).abs().max())
            line.append(f"{c}: {err:.3e} {'ok' if out_close(out.float().reshape(-1, 128), ref.float().reshape(-1, 128)) else 'MISSES'}")
        print(f"{name:48s} " + "   ".join(line))


if __name__ == "__main__":
    main()
