"""Device-resident budgeted KV bank driven through the C ABI (include/easykv_hip.h).

PyTorch is used for device memory and streams only; every operation on the bank is a HIP kernel
of ``libeasykv_hip.so``.  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import Optional

import torch

from . import _lib
from ._lib import Bank, Step, check

DECODE_RECENT_RATIO = 0.3   # easykv/easykv.py:308, :709 (hard-wired in the reference)
ROCO_TAIL = 10              # easykv/easykv.py:321, :472, :721


@dataclass
class StepPlan:
    """What the driver decides for one model forward; identical for every layer (mirrors the
    branches of easykv/easykv.py:287-362 for ``phase='decode'`` and :443-499 for ``'prefill'``)."""
    policy: str = "roco"
    phase: str = "decode"
    accumulate: bool = True
    evict: bool = False
    score_off: int = 0          # P: first position covered by the score rows
    budget: int = 0             # decode: budget ; prefill: budget' (= budget + stride)
    recent: int = 0             # prefill: int(budget' * recent_ratio)
    sink: int = 0               # prefill: temp_length
    stride: int = 1
    tova_head_mean: bool = False
    range_start: int = -1       # recency / random
    streaming: bool = False
    n_split: int = 0
    two_pass: int = 0           # scored chunk steps: 0 auto, 1 force the two-pass kernels, -1 force one pass
    n_evict: Optional[int] = None   # prefill steps: victims per head (None: ``stride``); one-shot prompt compression evicts n - budget at once
    pool: int = 1               # pooled selection (include/easykv_hip.h): kernel size of the pooling of the ranking values, odd; 1 = off
    pool_op: str = "max"        # ... 'max' or 'avg'
    # adaptive head budgets (include/easykv_hip.h): (evict_min, evict_max), the bounds of a head's victims around n_evict; the layer evicts
    # H * n_evict rows and the pooled ranking values decide each head's share (pool = 1: the unpooled rows rank).  None = off
    head_adaptive: Optional[tuple] = None


# The row formats of a quantised bank, by ``kv_quant`` (include/easykv_hip.h, "kv8" / "kv4" / "kv6" / "kv84" / "kv164"): everything the bank, the batch and the
# driver (api.py) need to know about one.  rows: the calls' prefix (ekv_<rows>_*); desc: the descriptor of the four planes; planes:
# (attribute, trailing shape at head_dim d, dtype, fill) in the descriptor's order — rows that were never written keep code 0 and
# scale 1 (exponent byte 127), so every scale of the bank is finite whatever the kernels prefetch; head_dims / max_rep: the shapes the
# decode kernels of the format are built for; pair_bytes: bytes of one K + V row pair; keeps (optional): the 16-bit tensors the format
# keeps next to its planes ("k16_mxfp4": the K rows), which its descriptor does not carry.
ROW_FORMATS = {
    "fp8": dict(kind="fp8", rows="kv8", desc=_lib.Kv8, label="FP8", method="quantize_fp8", stored="FP8 codes with per-row scales",
                planes=(("k8", lambda d: (d,), torch.uint8, 0), ("v8", lambda d: (d,), torch.uint8, 0),
                        ("k_scale", lambda d: (), torch.float32, 1), ("v_scale", lambda d: (), torch.float32, 1)),
                head_dims=(64, 128), max_rep=None, pair_bytes=lambda d: 2 * d + 8),
    "mxfp4": dict(kind="mxfp4", rows="kv4", desc=_lib.Kv4, label="MXFP4", method="quantize_mxfp4", stored="MXFP4 codes with block exponents",
                  planes=(("k4", lambda d: (d // 2,), torch.uint8, 0), ("v4", lambda d: (d // 2,), torch.uint8, 0),
                          ("k_exp", lambda d: (d // 32,), torch.uint8, 127), ("v_exp", lambda d: (d // 32,), torch.uint8, 127)),
                  head_dims=(128,), max_rep=4, pair_bytes=lambda d: d + d // 16),
    "mxfp6": dict(kind="mxfp6", rows="kv6", desc=_lib.Kv6, label="MXFP6", method="quantize_mxfp6", stored="MXFP6 codes with block exponents",
                  planes=(("k6", lambda d: (3 * d // 4,), torch.uint8, 0), ("v6", lambda d: (3 * d // 4,), torch.uint8, 0),
                          ("k_exp", lambda d: (d // 32,), torch.uint8, 127), ("v_exp", lambda d: (d // 32,), torch.uint8, 127)),
                  head_dims=(128,), max_rep=4, pair_bytes=lambda d: 3 * d // 2 + d // 16),
    # FP8 keys (the "fp8" K planes) with MXFP4 values (the "mxfp4" V planes): the eviction decisions of FP8 rows at MXFP6's bytes
    "fp8_mxfp4": dict(kind="fp8_mxfp4", rows="kv84", desc=_lib.Kv84, label="FP8-key / MXFP4-value", method="quantize_fp8_mxfp4",
                      stored="FP8 key codes with per-row scales and MXFP4 value codes with block exponents",
                      planes=(("k8", lambda d: (d,), torch.uint8, 0), ("v4", lambda d: (d // 2,), torch.uint8, 0),
                              ("k_scale", lambda d: (), torch.float32, 1), ("v_exp", lambda d: (d // 32,), torch.uint8, 127)),
                      head_dims=(128,), max_rep=None, pair_bytes=lambda d: 3 * d // 2 + 4 + d // 32),
    # the bank's own 16-bit keys, untouched, with MXFP4 values (the "mxfp4" V planes): the eviction decisions of the 16-bit bank, exactly
    "k16_mxfp4": dict(kind="k16_mxfp4", rows="kv164", desc=_lib.Kv164, label="16-bit-key / MXFP4-value", method="quantize_k16_mxfp4",
                      stored="16-bit keys and MXFP4 value codes with block exponents", keeps=("k",),
                      planes=(("v4", lambda d: (d // 2,), torch.uint8, 0), ("v_exp", lambda d: (d // 32,), torch.uint8, 127)),
                      head_dims=(128,), max_rep=None, pair_bytes=lambda d: 2 * d + d // 2 + d // 32),
}


# head_dims the soft-capped kernels (KVBank(logit_cap=...)) are built for
CAPPED_HEAD_DIMS = (128, 256)
# head_dims the sink kernels (KVBank(sinks=...)) are built for
SINK_HEAD_DIMS = (64, 128)
# head_dim the window kernels (KVBank(windows=...)) are built for: without sinks, with sinks (gpt-oss's shape)
WINDOW_HEAD_DIM = {False: 128, True: 64}
# head_dims served with plain keys and 16-bit rows only: no RoPE-on-read build (set_rope, streaming) and no quantised row format
PLAIN_KEYS_HEAD_DIMS = (256,)


def row_format(kind, what="kv_quant"):
    """The entry of ROW_FORMATS for ``kind`` ('fp8', 'mxfp4', 'mxfp6', 'fp8_mxfp4' or 'k16_mxfp4'), or None for None (16-bit rows);
    anything else is a ValueError naming ``what``."""
    if kind is not None and kind not in ROW_FORMATS:
        raise ValueError(f"{what} must be None or 'fp8' / 'mxfp4', not {kind!r}; 'mxfp6' is accepted as well, and 'fp8_mxfp4'")
    return ROW_FORMATS.get(kind)


def _check_row_shape(fmt, head_dim, rep):
    """EkvError unless the decode kernels of ``fmt`` are built for this head_dim and GQA factor."""
    if head_dim not in fmt["head_dims"]:
        raise _lib.EkvError(f"{fmt['method']}(): {fmt['label']} rows are built for head_dim {' and '.join(map(str, fmt['head_dims']))}, not {head_dim}")
    if fmt["max_rep"] is not None and rep > fmt["max_rep"]:
        raise _lib.EkvError(f"{fmt['method']}(): {fmt['label']} rows are built for GQA factors up to {fmt['max_rep']}, not {rep}")


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


def _row_strides(t: torch.Tensor, dtype=torch.float16):
    """(token_stride, head_stride) in elements when the rows of ``t`` ``[layers, heads, n, D]`` can be read in place by the kernels
    (ekv_step.*_stride, ABI 8): the bank's 16-bit ``dtype``, D contiguous elements per row, layers dense blocks apart, strides
    multiples of 8 — e.g. the ``[1, heads, n, D]`` transposed views HF attention modules hand over.  (0, 0) = the dense layout;
    None = needs a copy."""
    layers, heads, n, d = t.shape
    s0, s1, s2, s3 = t.stride()
    if t.dtype != dtype or s3 != 1 or (t.data_ptr() & 15):
        return None
    if layers > 1 and s0 != heads * n * d:
        return None
    ts = s2 if n > 1 else d
    hs = s1 if heads > 1 else max(n * d, ts)
    if ts == d and hs == n * d:
        return 0, 0
    if n == 1:
        return (0, 0) if hs == d else None
    if ts < d or hs < d or (ts & 7) or (hs & 7):
        return None
    return ts, hs


def _stride_rows(st, q, k_new, v_new, out, dtype=torch.float16):
    """Fill the row strides of ``st`` from the tensors; tensors whose layout the kernels cannot read in place, or whose dtype is not
    the bank's ``dtype``, are converted / copied dense (k_new and v_new share one pair of strides).  Returns (q, k_new, v_new)."""
    f16 = dtype
    if (q.dtype is f16 and k_new.dtype is f16 and v_new.dtype is f16 and q.is_contiguous() and k_new.is_contiguous() and v_new.is_contiguous()
            and (out is None or out.is_contiguous())):
        # dense tensors (the bank-level callers: tests, bench): a few C++ calls — this sits on the per-layer critical path of a decoder
        # stack, where the host cost of a call is what bounds small layers
        if st.q_token_stride or st.q_head_stride or st.kv_token_stride or st.kv_head_stride or st.out_token_stride or st.out_head_stride:
            st.q_token_stride = st.q_head_stride = st.kv_token_stride = st.kv_head_stride = st.out_token_stride = st.out_head_stride = 0
        return q, k_new, v_new
    sq = _row_strides(q, dtype)
    if sq is None:
        q, sq = q.to(dtype).contiguous(), (0, 0)
    sk, sv = _row_strides(k_new, dtype), _row_strides(v_new, dtype)
    if sk is None or sv != sk:
        k_new, v_new, sk = k_new.to(dtype).contiguous(), v_new.to(dtype).contiguous(), (0, 0)
    so = (0, 0) if out is None else _row_strides(out, dtype)
    if so is None:
        raise ValueError(f"`out` must be a {dtype} tensor whose rows are head_dim contiguous elements at strides that are multiples of 8")
    (st.q_token_stride, st.q_head_stride), (st.kv_token_stride, st.kv_head_stride), (st.out_token_stride, st.out_head_stride) = sq, sk, so
    return q, k_new, v_new


class KVBank:
    """K/V rows + slot map + score rows of ``n_layers`` layers on one GPU.

    ``dtype`` (torch.float16 or torch.bfloat16) is the element type of the K/V rows, and of the queries, new rows and outputs of
    every step: tensors of another dtype are converted to it, ``out`` is allocated in it.  bf16 banks run the bf16 builds of the
    same kernels (include/easykv_hip.h, EKV_DTYPE_BF16); RoPE-on-read (``StepPlan.streaming``) has no bf16 build."""

    default_two_pass = 0    # StepPlan.two_pass used when a plan leaves it at 0 (tests force either chunk scheme with it)
    dtype, _dt = torch.float16, _lib.DTYPE_F16      # (set per bank by __init__)
    # byte budget of the resident rows of this bank's one-launch decode steps (include/easykv_hip.h, "resident rows"): None = the
    # library's default, 0 = every K/V load non-temporal — what a caller sets whose process streams more than the Infinity Cache holds
    # between two steps (easykv_amd.api: a model's weights)
    resident_bytes = None
    kv_quant = None      # quantize(): "fp8" / "mxfp4" / "mxfp6" / "fp8_mxfp4" / "k16_mxfp4" (ROW_FORMATS; _fmt is the entry, _desc the descriptor of its planes)

    long_rows = False    # KVBank(..., long_rows=True): the steps go to the long-row family (ekv_long_*), set per bank by __init__
    logit_cap = None     # KVBank(..., logit_cap=c): soft-capped logits, the steps go to the capped family (ekv_cap_*), set per bank by __init__
    sm_scale = None      # KVBank(..., sm_scale=s): logits are q.k * s (None: 1 / sqrt(head_dim)), in every call family
    sinks = None         # KVBank(..., sinks=t): attention sinks, the steps go to the sink family (ekv_sink_*), set per bank by __init__
    windows = None       # KVBank(..., windows=[...]): sliding windows, the steps go to the window family (ekv_win_*), set per bank by __init__
    tok_pos = None       # ... int32 [n_layers, H, cap]: the token position every physical row was appended at

    def __init__(self, n_layers, n_q_heads, n_kv_heads, head_dim, cap, device="cuda", scored=True, dtype=torch.float16, kv_quant=None, long_rows=False,
                 logit_cap=None, sm_scale=None, sinks=None, windows=None):
        """``windows``: ``n_layers`` integers >= 0, the sliding window of every layer (0: none; include/easykv_hip.h, "sliding windows";
        gpt-oss: 128 on every other layer).  A key appended ``W`` or more tokens behind the query is masked — by the token position its
        physical row carries (``tok_pos``), not by its place in the slot map, because eviction is per head.  A masked key stays live:
        it keeps its slot and score column, receives p = 0 and a count, and may be a victim.  All-zero windows are legal and still route
        to the window family (``ekv_win_*``), whose steps plan as the sink family's (decode: phase order F, no resident rows; chunk steps
        and the dense prefix: the 16x16 chunk kernel in blocks of at most 32 folded rows).  head_dim 128 without ``sinks``, 64 with them; 16-bit rows,
        plain keys: not with ``logit_cap``, ``kv_quant`` or ``long_rows``, and :meth:`quantize` / :meth:`set_rope` /
        :meth:`compact_inplace` refuse such a bank.  A negative value or a wrong shape raises ``ValueError``.
        ``sinks``: a tensor ``[n_layers, n_q_heads]`` of finite values, kept as fp32 on the device: learned attention sinks (gpt-oss:
        ``s_aux``; include/easykv_hip.h, "attention sinks").  The logit of layer ``l`` and query head ``h`` joins every softmax of that
        head as a virtual key with value 0: it takes its share of the probability mass and has no column, no score and is never a
        victim.  The bank's steps go to the sink call family: decode steps plan as the plain ones (phase order F, no resident rows),
        chunk steps and the dense prefix run on the 16x16 chunk kernel in blocks of at most 32 folded rows.  head_dim 64 and 128, 16-bit
        rows, plain keys: not with ``logit_cap``, ``kv_quant`` or ``long_rows``, and :meth:`quantize` / :meth:`set_rope` refuse such a
        bank.  A wrong shape or a non-finite value raises ``ValueError``.
        ``sm_scale``: the softmax scale, logits are ``q.k * sm_scale`` (None: ``1 / sqrt(head_dim)``; e.g. ``query_pre_attn_scalar ** -0.5``
        of a Gemma 2 / Gemma 3 model).  Every call family reads it (``ekv_step.sm_div = 1 / sm_scale``).
        ``logit_cap=c`` (finite, > 0): attention-logit soft-capping, ``s = c * tanh(q.k * sm_scale / c)`` before the mask and the
        softmax (Gemma 2: ``attn_logit_softcapping``; include/easykv_hip.h, "soft-capped logits").  The bank's steps go to the capped
        call family: decode steps plan as the uncapped ones, chunk steps and the dense prefix run on the 16x16 chunk kernel in blocks of
        at most 32 folded rows.  head_dim 128 and 256, 16-bit rows, plain keys: not with ``kv_quant`` or ``long_rows``, and
        :meth:`quantize` / :meth:`set_rope` refuse such a bank.
        ``long_rows=True``: a 16-bit bank whose steps go to the long-row call family (include/easykv_hip.h, "long score rows"):
        planned and run exactly as the plain calls, except that a scored step which would end in the generic scorer ends in the
        long-row scorer instead, whose width is bounded by ``cap`` and the workspace, not by one CU's LDS (the plain family refuses
        such a step beyond about 38 400 score columns).  Same bits wherever both run.  Not with ``kv_quant``, and :meth:`quantize`
        refuses such a bank.
        ``kv_quant='fp8'``: the bank is created holding FP8 planes only (see :meth:`quantize_fp8`); the 16-bit K/V rows are never
        allocated.  Such a bank is filled by decode steps or, as one sequence of a :class:`KVBankBatch`, by ``adopt()``.
        ``kv_quant='mxfp4'``: likewise with MXFP4 planes only (see :meth:`quantize_mxfp4`; head_dim 128, GQA factors up to 4).
        ``kv_quant='mxfp6'``: likewise with MXFP6 planes only (see :meth:`quantize_mxfp6`; the same shapes).
        ``kv_quant='fp8_mxfp4'``: likewise with FP8 key planes and MXFP4 value planes (see :meth:`quantize_fp8_mxfp4`; head_dim 128).
        ``kv_quant='k16_mxfp4'``: the 16-bit K rows and MXFP4 value planes (see :meth:`quantize_k16_mxfp4`; head_dim 128); a 16-bit V is
        never allocated."""
        if dtype not in _lib.DTYPE_CODES:
            raise ValueError(f"KVBank dtype must be torch.float16 or torch.bfloat16, not {dtype}")
        fmt = row_format(kv_quant, "KVBank kv_quant")
        if long_rows and fmt is not None:
            raise _lib.EkvError(f"KVBank(long_rows=True): the long-row scorer is built for 16-bit rows, not for {fmt['label']} rows "
                                f"(kv_quant={kv_quant!r}): a quantised bank serves decode steps through its own calls, which have no long form")
        self.long_rows = bool(long_rows)
        if sm_scale is not None and not (isinstance(sm_scale, (int, float)) and 0.0 < float(sm_scale) < math.inf):
            raise ValueError(f"KVBank sm_scale must be None (1 / sqrt(head_dim)) or a finite number > 0, not {sm_scale!r}")
        self.sm_scale = None if sm_scale is None else float(sm_scale)
        if logit_cap is not None:      # (before anything is allocated)
            if not (isinstance(logit_cap, (int, float)) and 0.0 < float(logit_cap) < math.inf):
                raise ValueError(f"KVBank logit_cap must be None or a finite number > 0, not {logit_cap!r}")
            if fmt is not None:
                raise _lib.EkvError(f"KVBank(logit_cap=...): soft-capped logits are built for 16-bit rows, not for {fmt['label']} rows "
                                    f"(kv_quant={kv_quant!r}): there is no capped quantised call")
            if long_rows:
                raise _lib.EkvError("KVBank(logit_cap=..., long_rows=True): there is no capped long call (the long-row family has no soft-capped form)")
            if head_dim not in CAPPED_HEAD_DIMS:
                raise _lib.EkvError(f"KVBank(logit_cap=...): soft-capped logits are built for head_dim {' and '.join(map(str, CAPPED_HEAD_DIMS))}, not {head_dim}")
            self.logit_cap = float(logit_cap)
        if sinks is not None:      # (before anything is allocated or loaded)
            if not (torch.is_tensor(sinks) and tuple(sinks.shape) == (n_layers, n_q_heads)):
                got = tuple(sinks.shape) if torch.is_tensor(sinks) else type(sinks).__name__
                raise ValueError(f"KVBank sinks must be a tensor of shape [n_layers, n_q_heads] = [{n_layers}, {n_q_heads}], not {got}")
            if not bool(torch.isfinite(sinks.detach().float()).all()):
                raise ValueError("KVBank sinks must be finite (a sink is a logit: -inf would be 'no sink', which is sinks=None)")
            if logit_cap is not None:
                raise _lib.EkvError("KVBank(sinks=..., logit_cap=...): there is no capped sink call (the sink family has no soft-capped form)")
            if fmt is not None:
                raise _lib.EkvError(f"KVBank(sinks=...): attention sinks are built for 16-bit rows, not for {fmt['label']} rows "
                                    f"(kv_quant={kv_quant!r}): there is no quantised sink call")
            if long_rows:
                raise _lib.EkvError("KVBank(sinks=..., long_rows=True): there is no long sink call (the long-row family has no sink form)")
            if head_dim not in SINK_HEAD_DIMS:
                raise _lib.EkvError(f"KVBank(sinks=...): attention sinks are built for head_dim {' and '.join(map(str, SINK_HEAD_DIMS))}, not {head_dim}")
        if windows is not None:      # (before anything is allocated or loaded)
            try:
                wl = windows.tolist() if torch.is_tensor(windows) else list(windows)
            except TypeError:
                wl = None
            if not (isinstance(wl, list) and len(wl) == n_layers and all(isinstance(w, int) and not isinstance(w, bool) for w in wl)):
                raise ValueError(f"KVBank windows must be {n_layers} integers (one per layer), not {windows!r}")
            if any(w < 0 for w in wl):
                raise ValueError(f"KVBank windows must be >= 0 (0: no window), not {wl}")
            if logit_cap is not None:
                raise _lib.EkvError("KVBank(windows=..., logit_cap=...): there is no capped window call (the window family has no soft-capped form)")
            if fmt is not None:
                raise _lib.EkvError(f"KVBank(windows=...): sliding windows are built for 16-bit rows, not for {fmt['label']} rows "
                                    f"(kv_quant={kv_quant!r}): there is no quantised window call")
            if long_rows:
                raise _lib.EkvError("KVBank(windows=..., long_rows=True): there is no long window call (the long-row family has no window form)")
            if head_dim != WINDOW_HEAD_DIM[sinks is not None]:
                raise _lib.EkvError(f"KVBank(windows=...): sliding windows {'with' if sinks is not None else 'without'} sinks are built for "
                                    f"head_dim {WINDOW_HEAD_DIM[sinks is not None]}, not {head_dim}")
        if fmt is not None:
            _check_row_shape(fmt, head_dim, n_q_heads // max(1, n_kv_heads))
        self.dtype, self._dt = dtype, _lib.DTYPE_CODES[dtype]
        self.lib = _lib.load()
        dev = torch.device(device)
        if dev.type != "cuda":
            raise _lib.EkvError("KVBank needs a GPU device; the product path has no CPU fallback")
        self.device = dev
        self._dev_index = dev.index if dev.index is not None else torch.cuda.current_device()
        cap = (cap + 63) // 64 * 64     # rows of the slot map / score rows stay 16-byte aligned (fused kernel, LDS-DMA)
        self.n_layers, self.n_q_heads, self.n_kv_heads, self.head_dim, self.cap = n_layers, n_q_heads, n_kv_heads, head_dim, cap
        keeps = ("k", "v") if fmt is None else fmt.get("keeps", ())      # the 16-bit tensors this bank holds
        self.k, self.v = (torch.empty(n_layers, n_kv_heads, cap, head_dim, dtype=dtype, device=dev) if name in keeps else None for name in ("k", "v"))
        # (the state tensors are reached through properties: reading one converts slot-indexed layers back to the ordered layout)
        self._slot_of_pos = torch.empty(n_layers, n_kv_heads, cap, dtype=torch.int32, device=dev)
        self._score_sum = torch.zeros(n_layers, n_kv_heads, cap, dtype=torch.float32, device=dev) if scored else None
        self._score_sq = torch.zeros_like(self._score_sum) if scored else None
        self._score_cnt = torch.zeros_like(self._score_sum) if scored else None
        # slot-indexed score rows (include/easykv_hip.h, EKV_PHASE_SLOT_ROWS): order keys, (count offset, next birth) per head, and
        # which layers currently hold that layout
        self.birth = torch.zeros(2, n_layers, n_kv_heads, cap, dtype=torch.int32, device=dev) if scored else None
        self.slot_state = torch.zeros(n_layers, n_kv_heads, 4, dtype=torch.float32, device=dev) if scored else None
        self._slot_rows = [False] * n_layers
        self._slot_min_tail = [1 << 30] * n_layers      # smallest protected tail of an evicting step since the conversion
        self._slot_ok = {}        # step shape -> does the slot-indexed decode kernel take it (ekv_step_check)
        self._slot_stretch = self._slot_short = 0      # steps since the layout was entered; short stretches seen (see _ensure_ordered)
        self._slot_cool = 0       # one-launch decode steps run on the ordered layout since the thrash guard closed (see _enter_slot_rows)
        self.n_slots = [0] * n_layers
        # High-water mark of live rows per layer.  The library keeps the free list as [freed rows (most recent first), never-
        # used rows ascending] and appends take from its front, so every live row has a physical index < extent: the
        # one-launch decode step streams the rows [0, extent) in address order (ekv_step.phys_extent).
        self.extent = [0] * n_layers
        self._ws = None
        # scorer off the critical path (attend(..., overlap_scorer=True)): side streams, a ring of workspaces and, per
        # layer, the event after which its slot map / score rows are up to date again
        self._side = None
        self._ws_ring = []
        self._ws_free = []
        self._ring_pos = 0
        self._score_done = [None] * n_layers
        self._defer = None      # deferred-scorer state of the token step in flight (attend(..., defer=True) ... flush())
        self._pool_fams = {}    # (radius, op) -> the pooled family's calls and struct (_family)
        self._ada_fams = {}     # (radius, op, evict_min, evict_max) -> the adaptive family's calls and struct (_ada_family)
        self._ada_out = None    # device int32 [n_layers][H]: the victim count of every head after an adaptive step
        self._view = None       # the bank as n_layers * H one-head layers, for decode steps over heads of different lengths (_attend_ragged)
        self.head_slots = None  # [n_layers][H] ints after an adaptive step (None: every head of a layer holds n_slots rows)
        self._heads = None      # device table, host copy and struct of the heads family (ekv_heads_*: deferred decode steps over heads of different lengths)
        self.head_table_uploads = 0      # times the device table of the heads family was written (lengths changed other than by uniform growth)
        self.arrive = torch.zeros(n_layers, n_kv_heads, dtype=torch.int32, device=dev)     # arrival counters of the in-kernel fold
        self._bank = Bank(_ptr(self.k), _ptr(self.v), self._slot_of_pos.data_ptr(),
                          self._score_sum.data_ptr() if scored else None, self._score_sq.data_ptr() if scored else None,
                          self._score_cnt.data_ptr() if scored else None, n_layers, n_q_heads, n_kv_heads, head_dim, cap,
                          self.arrive.data_ptr(), self.birth.data_ptr() if scored else None,
                          self.slot_state.data_ptr() if scored else None)
        self.rope_cos = self.rope_sin = None
        if sinks is not None:      # (a constant of the bank: the pointer every sink call carries, hipGraph capture included)
            self.sinks = sinks.detach().to(dev, torch.float32).contiguous().clone()
        self._tokens = [0] * n_layers      # tokens every head of a layer has been handed so far: the position of its next query
        if windows is not None:      # (allocated for a window bank only)
            self.windows = tuple(wl)
            self.tok_pos = torch.zeros(n_layers, n_kv_heads, cap, dtype=torch.int32, device=dev)
            self._windows_dev = torch.tensor(wl, dtype=torch.int32, device=dev)
            self._windows_host = (C.c_int32 * n_layers)(*wl)      # (the copy the library can check; kept alive with the bank)
            self._win = _lib.Win(self.tok_pos.data_ptr(), self._windows_dev.data_ptr(), self._windows_host,
                                 self.sinks.data_ptr() if self.sinks is not None else None, 0)
        self._attach(fmt)
        self.reset()

    # -- layout of the score rows -------------------------------------------------------------------
    use_slot_rows = True      # one-launch decode steps run on the slot-indexed layout where the library supports it
    SLOT_COOL_DOWN = 256      # ordered one-launch decode steps after which a bank whose thrash guard closed tries the layout again

    def layout_signature(self):
        """Which layers hold the slot-indexed layout.  A hipGraph captured over steps of this bank replays the kernels of the layout
        it was captured on: whoever replays one must find the same signature as at capture time (an eager call in between — a read
        of ``bank.score_sum``, a chunk step — converts layers back; only the conversion itself is refused DURING a capture)."""
        return tuple(self._slot_rows)

    def _ensure_ordered(self, layer_begin=0, layer_count=None):
        """Bring the score rows / slot map of the layers back to the ordered layout (every kernel but the one-launch decode step
        reads that one; so do the state tensors handed out below)."""
        end = self.n_layers if layer_count is None else layer_begin + layer_count
        l = layer_begin
        while l < end:
            if not self._slot_rows[l]:
                l += 1
                continue
            m = l
            while m < end and self._slot_rows[m] and self.n_slots[m] == self.n_slots[l]:
                m += 1
            if torch.cuda.is_current_stream_capturing():
                raise _lib.EkvError("a layout change of the score rows cannot be captured in a graph: run the step once outside the capture")
            check(self.lib.ekv_rows_to_order(C.byref(self._bank), l, m - l, self.n_slots[l], self._stream()), "ekv_rows_to_order")
            # a caller that alternates between one-launch decode steps and anything that reads the ordered layout pays two
            # conversions per step (~0.2 ms per 256 heads each): after a few stretches of under 16 steps the bank stays ordered
            self._slot_short = self._slot_short + 1 if self._slot_stretch < 16 else max(0, self._slot_short - 1)
            self._slot_stretch = 0
            for i in range(l, m):
                self._slot_rows[i] = False
            l = m

    def _enter_slot_rows(self, st) -> bool:
        """Decide whether this one-launch decode step runs on the slot-indexed layout, converting its layers if it does."""
        lb, lc = st.layer_begin, st.layer_count
        rows = self._slot_rows[lb:lb + lc]
        if not (self.use_slot_rows and self._score_sum is not None) or len(set(self.n_slots[lb:lb + lc])) != 1:
            return False
        if self._slot_short >= 4:
            # thrash guard (see _ensure_ordered): the caller kept interleaving state reads with decode steps.  Not for ever — a
            # generate that reads the state during its first tokens and then settles into pure decode gets the layout back after a
            # cool-down of ordered steps; one more short stretch closes the guard again at once
            self._slot_cool += 1
            if self._slot_cool < self.SLOT_COOL_DOWN or torch.cuda.is_current_stream_capturing():
                return False
            self._slot_short, self._slot_cool = 3, 0
        st.phases = _lib.PHASE_SLOT_ROWS
        key = bytes(st)
        ok = self._slot_ok.get(key)
        if ok is None:
            if len(self._slot_ok) > 4096:      # (a growing cache asks about a new shape every step)
                self._slot_ok.clear()
            ok = self._slot_ok[key] = self._step_check(st) == 0
        st.phases = 0
        if not ok:
            return False
        if not all(rows):
            if torch.cuda.is_current_stream_capturing():
                return False          # (no layout change inside a capture: this step runs on the ordered layout)
            self._ensure_ordered(lb, lc)     # (a partly converted range)
            check(self.lib.ekv_rows_to_slots(C.byref(self._bank), lb, lc, self.n_slots[lb], self._stream()), "ekv_rows_to_slots")
            for i in range(lb, lb + lc):
                self._slot_rows[i] = True
                self._slot_min_tail[i] = 1 << 30      # (births = order indices: every tail is consecutive)
        self._slot_stretch += 1
        return True

    @property
    def slot_of_pos(self):
        self._ensure_ordered()
        return self._slot_of_pos

    @property
    def score_sum(self):
        self._ensure_ordered()
        return self._score_sum

    @property
    def score_sq(self):
        self._ensure_ordered()
        return self._score_sq

    @property
    def score_cnt(self):
        self._ensure_ordered()
        return self._score_cnt

    # -- quantised K/V storage ("kv8" / "kv4", include/easykv_hip.h; ROW_FORMATS) ----------------------
    def _quant_refuse(self, cond, what):
        if cond and self._fmt is not None:
            raise _lib.EkvError(f"{what} is not available on a bank quantised by {self._fmt['method']}(): its K/V rows are "
                                f"{self._fmt['stored']}, which only decode steps (q_len == 1, plain keys) read and append to")

    def quantize(self, kind):
        """Convert the live bank in place to the row format ``kind`` ('fp8' / 'mxfp4' / 'mxfp6' / 'fp8_mxfp4' / 'k16_mxfp4'): codes and scales / exponents are written at the
        rows' physical indices (slot map, free list and score rows carry over as they are, in either layout), the 16-bit K/V tensors
        are released (``'k16_mxfp4'`` keeps ``k``, untouched, and releases ``v`` only), ``kv_quant`` is ``kind`` and ``attend`` / ``step_info`` / ``step_plan`` go to that format's calls.  From here on
        the bank serves decode steps only: chunk steps, ``load_rows``, ``set_rope`` and the row moves raise :class:`EkvError`.  A bank
        is quantised once: a second conversion raises."""
        fmt = row_format(kind, "quantize(kind)")
        if fmt is None:
            raise ValueError("quantize(kind): kind must be 'fp8' or 'mxfp4'")
        m = fmt["method"] + "()"
        if self.logit_cap is not None:
            raise _lib.EkvError(f"{m}: the bank was created with logit_cap={self.logit_cap:g}, and soft-capped logits are built for 16-bit "
                                f"rows, not for {fmt['label']} rows: there is no capped quantised call")
        if self.sinks is not None:
            raise _lib.EkvError(f"{m}: the bank was created with sinks, and attention sinks are built for 16-bit rows, not for "
                                f"{fmt['label']} rows: there is no quantised sink call")
        if self.windows is not None:
            raise _lib.EkvError(f"{m}: the bank was created with windows, and sliding windows are built for 16-bit rows, not for "
                                f"{fmt['label']} rows: there is no quantised window call")
        if self.long_rows:
            raise _lib.EkvError(f"{m}: the bank was created with long_rows=True, and the long-row scorer is built for 16-bit rows, not "
                                f"for {fmt['label']} rows: {fmt['label']} rows have no long form")
        if self._fmt is not None:
            raise _lib.EkvError(f"{m}: the bank's rows are quantised already ({self._fmt['label']} already: kv_quant={self.kv_quant!r})")
        _check_row_shape(fmt, self.head_dim, self.n_q_heads // self.n_kv_heads)
        if self.rope_cos is not None:
            raise _lib.EkvError(f"{m}: a RoPE-on-read (streaming) bank keeps un-rotated keys, which the {fmt['label']} decode kernels do not rotate")
        if self._defer is not None and self._defer["pending"]:
            raise _lib.EkvError(f"{m}: a deferred token step is open (flush() first)")
        if torch.cuda.is_current_stream_capturing():
            raise _lib.EkvError(f"{m} cannot be captured in a graph: convert the bank before the capture")
        self.join()
        desc = self._planes(fmt)
        call = f"ekv_{fmt['rows']}_quantize"
        check(getattr(self.lib, call)(C.byref(self._bank), C.byref(desc), self._dt, 0, self.n_layers, max(self.extent), self._stream()), call)
        cur = torch.cuda.current_stream(self.device)
        for name in ("k", "v"):      # (the 16-bit tensors the format does not keep)
            if name not in fmt.get("keeps", ()):
                getattr(self, name).record_stream(cur)
                setattr(self, name, None)
        self._attach(fmt, desc)
        return self

    def quantize_fp8(self):
        """:meth:`quantize` to FP8 (OCP e4m3fn) K/V rows with one fp32 scale per row (``k8`` / ``v8`` / ``k_scale`` / ``v_scale``),
        head_dim 64 and 128.  On a bank that holds FP8 rows already it does nothing."""
        return self if self.kv_quant == "fp8" else self.quantize("fp8")

    def quantize_mxfp4(self):
        """:meth:`quantize` to MXFP4 K/V rows: e2m1 codes, two per byte, with one E8M0 exponent per 32-element block (``k4`` / ``v4``
        / ``k_exp`` / ``v_exp``), head_dim 128 and GQA factors up to 4."""
        return self.quantize("mxfp4")

    def quantize_mxfp6(self):
        """:meth:`quantize` to MXFP6 K/V rows: e2m3 codes, 32 per 24-byte block, with one E8M0 exponent per 32-element block (``k6`` /
        ``v6`` / ``k_exp`` / ``v_exp``; 200 bytes per row pair), head_dim 128 and GQA factors up to 4."""
        return self.quantize("mxfp6")

    def quantize_fp8_mxfp4(self):
        """:meth:`quantize` to FP8 keys with MXFP4 values: the K planes of :meth:`quantize_fp8` (``k8`` / ``k_scale``) and the V planes of
        :meth:`quantize_mxfp4` (``v4`` / ``v_exp``), 200 bytes per row pair at head_dim 128, the only head_dim; every GQA factor FP8
        rows take.  Eviction reads logits only, so the bank evicts exactly what its FP8 twin evicts."""
        return self.quantize("fp8_mxfp4")

    def quantize_k16_mxfp4(self):
        """:meth:`quantize` to 16-bit keys with MXFP4 values: ``k`` stays as it is and only V becomes the V planes of
        :meth:`quantize_mxfp4` (``v4`` / ``v_exp``), 324 bytes per row pair at head_dim 128, the only head_dim; every GQA factor the
        16-bit decode step takes.  Eviction reads logits only and the keys are not quantised, so the bank evicts exactly what the
        16-bit bank evicts."""
        return self.quantize("k16_mxfp4")

    def _planes(self, fmt):
        """Allocate the planes of ``fmt`` as the bank's attributes; returns their descriptor."""
        shape = (self.n_layers, self.n_kv_heads, self.cap)
        for name, tail, dtype, fill in fmt["planes"]:
            setattr(self, name, torch.full(shape + tail(self.head_dim), fill, dtype=dtype, device=self.device))
        return fmt["desc"](*(getattr(self, name).data_ptr() for name, *_ in fmt["planes"]))

    def _attach(self, fmt, desc=None):
        """The bank's rows are in the format ``fmt`` from here on (None: 16-bit rows; ``desc=None``: a bank created without 16-bit rows
        allocates its planes now).  The library calls of the format and the descriptor reference are resolved here, once: the
        per-layer callers below are host-bound and look nothing up."""
        if fmt is not None:
            self._desc = self._planes(fmt) if desc is None else desc
            # the descriptor's planes stand where the rows were: the planning calls that take the bank alone never dereference them
            # (a format that keeps the 16-bit keys has no K plane: bank.k stays the rows')
            self._bank.k = _ptr(self.k) if "k" in fmt.get("keeps", ()) else self._desc.k_codes
            self._bank.v = self._desc.v_codes
            self.kv_quant = fmt["kind"]
            self._slot_ok.clear()
            self._defer = None
        rows = fmt["rows"] if fmt is not None else None
        self._fmt, self._desc_ref = fmt, () if fmt is None else (C.byref(self._desc),)
        self._calls = {(batch, what): getattr(self.lib, _lib.step_call_name(rows, batch, what))
                       for batch in (False, True) for what in _lib.STEP_CALLS}
        self._check_fn, self._info_fn, self._ws_fn, self._attend_fn = (self._calls[False, what] for what in _lib.STEP_CALLS)
        if self.long_rows:      # (16-bit rows: __init__ and quantize() refuse every other format) the long family, same signatures
            self._check_fn, self._info_fn, self._ws_fn, self._attend_fn = (getattr(self.lib, _lib.LONG_CALLS[what]) for what in _lib.STEP_CALLS)
        if self.logit_cap is not None:      # (16-bit rows likewise) the capped family: the cap stands behind the dtype, where a quantised call has its descriptor
            self._check_fn, self._info_fn, self._ws_fn, self._attend_fn = (getattr(self.lib, _lib.CAP_CALLS[what]) for what in _lib.STEP_CALLS)
            self._desc_ref = (C.c_float(self.logit_cap),)
        if self.sinks is not None:      # (16-bit rows likewise) the sink family: the sinks' device pointer stands behind the dtype
            self._check_fn, self._info_fn, self._ws_fn, self._attend_fn = (getattr(self.lib, _lib.SINK_CALLS[what]) for what in _lib.STEP_CALLS)
            self._desc_ref = (C.c_void_p(self.sinks.data_ptr()),)
        if self.windows is not None:      # (16-bit rows likewise) the window family: its struct (sinks or NULL inside) stands behind the dtype;
            # q_pos0 is written into the struct before every attention call (_set_q_pos), so cached references stay valid
            self._check_fn, self._info_fn, self._ws_fn, self._attend_fn = (getattr(self.lib, _lib.WIN_CALLS[what]) for what in _lib.STEP_CALLS)
            self._desc_ref = (C.byref(self._win),)

    tokens_seen = property(lambda self: max(self._tokens), doc="tokens the sequence has been handed so far (the next query's position)")

    def _set_q_pos(self, layer_begin, lc, q_pos):
        """The token position of the step's query row, into the window struct (a window bank; a no-op otherwise): ``q_pos`` or, for
        None, the tokens these layers have seen, which must agree.  Known on the host without a sync: every step appends ``q_len``
        tokens to every head (row ``i`` of a chunk step is at ``q_pos + i``)."""
        if self.windows is None:
            return
        if q_pos is None:
            seen = set(self._tokens[layer_begin:layer_begin + lc])
            if len(seen) != 1:
                raise _lib.EkvError(f"attend(): layers [{layer_begin}, {layer_begin + lc}) have seen different token counts {sorted(seen)}")
            q_pos = seen.pop()
        if not (isinstance(q_pos, int) and q_pos >= 0):
            raise ValueError(f"attend(q_pos=...) must be an integer >= 0, not {q_pos!r}")
        if torch.cuda.is_current_stream_capturing():
            raise _lib.EkvError("attend() on a bank created with windows during a hipGraph capture: the token position of the query (q_pos0) is a "
                                "host scalar of every window call, which a captured graph would freeze")
        self._win.q_pos0 = q_pos

    def ordered_tok_pos(self, layer_begin=0, layer_count=None):
        """The token positions of the live rows in slot-map order, int32 ``[layers, H, T]`` (a window bank; for tests and tools)."""
        if self.windows is None:
            raise _lib.EkvError("ordered_tok_pos(): the bank was created without windows")
        lc = self.n_layers - layer_begin if layer_count is None else layer_count
        t = self.n_slots[layer_begin]
        slots = self.slot_of_pos[layer_begin:layer_begin + lc, :, :t].long()
        return torch.gather(self.tok_pos[layer_begin:layer_begin + lc], 2, slots)

    def kv_bytes(self) -> int:
        """Bytes held for the K/V rows: 16-bit rows, FP8 codes + row scales (``2 * head_dim + 8`` per row pair), or MXFP4 codes +
        block exponents (``head_dim + head_dim / 16``: 136 at head_dim 128; MXFP6: ``3 * head_dim / 2 + head_dim / 16``, 200; FP8 keys with MXFP4
        values: ``3 * head_dim / 2 + 4 + head_dim / 32``, 200; 16-bit keys with MXFP4 values: ``2 * head_dim + head_dim / 2 + head_dim / 32``, 324)."""
        pair = 4 * self.head_dim if self._fmt is None else self._fmt["pair_bytes"](self.head_dim)
        return self.n_layers * self.n_kv_heads * self.cap * pair

    def dequantized_rows(self, layer):
        """(K, V) ``[H, cap, head_dim]`` fp32 of the PHYSICAL rows of ``layer``: code * scale of a quantised bank (exact), the 16-bit rows
        of any other widened.  Rows that were never written read as zeros on a quantised bank.  For tests and tools."""
        if self._fmt is None:
            return self.k[layer].float(), self.v[layer].float()
        k = torch.empty(self.n_kv_heads, self.cap, self.head_dim, dtype=torch.float32, device=self.device)
        v = torch.empty_like(k)
        call = f"ekv_{self._fmt['rows']}_dequantize"
        if "k" in self._fmt.get("keeps", ()):      # (the keys are 16-bit rows: the conversion is V's alone)
            check(getattr(self.lib, call)(C.byref(self._bank), *self._desc_ref, _lib.DTYPE_F32, layer, 1, self.cap, _ptr(v), self._stream()), call)
            return self.k[layer].float(), v
        check(getattr(self.lib, call)(C.byref(self._bank), *self._desc_ref, _lib.DTYPE_F32, layer, 1, self.cap, _ptr(k), _ptr(v), self._stream()), call)
        return k, v

    def _family(self, plan=None):
        """(check, info, workspace, attend, leading descriptor arguments) of the call family a step of ``plan`` goes to: the bank's own,
        or — a property of the STEP, ``plan.pool > 1`` — the pooled family (ekv_pool_*), whose struct stands behind the dtype.  There is
        no pooled capped, sink, window, long or quantised call: such a bank raises :class:`EkvError`."""
        if plan is not None and plan.head_adaptive is not None:
            return self._ada_family(plan)
        if plan is None or plan.pool == 1:
            return self._check_fn, self._info_fn, self._ws_fn, self._attend_fn, self._desc_ref
        if not (isinstance(plan.pool, int) and not isinstance(plan.pool, bool) and plan.pool >= 3 and plan.pool % 2 == 1):
            raise ValueError(f"StepPlan.pool is the kernel size of the pooling: 1 (off) or an odd integer >= 3, not {plan.pool!r}")
        if plan.pool_op not in _lib.POOL_OPS:
            raise ValueError(f"StepPlan.pool_op must be 'max' or 'avg', not {plan.pool_op!r}")
        for what, on in (("logit_cap", self.logit_cap is not None), ("sinks", self.sinks is not None), ("windows", self.windows is not None),
                         ("long_rows=True", self.long_rows), (f"kv_quant={self.kv_quant!r}", self._fmt is not None)):
            if on:
                raise _lib.EkvError(f"a pooled step (StepPlan.pool = {plan.pool}) on a bank created with {what}: there is no pooled "
                                    f"{what.split('=')[0].replace('_', ' ')} call (pooled selection serves plain 16-bit banks)")
        key = (plan.pool // 2, _lib.POOL_OPS[plan.pool_op])
        fam = self._pool_fams.get(key)
        if fam is None:
            desc = _lib.Pool(*key)      # (kept alive with the bank: a deferred token step caches the reference)
            fam = self._pool_fams[key] = tuple(getattr(self.lib, _lib.POOL_CALLS[what]) for what in _lib.STEP_CALLS) + ((C.byref(desc),), desc)
        return fam[:5]

    def _ada_family(self, plan):
        """The adaptive family (ekv_ada_*) of a step with ``plan.head_adaptive = (evict_min, evict_max)``: the struct carries the pooling
        (kernel size 1 = radius 0), the bounds and the device row ``[n_layers][H]`` the step writes each head's victim count to.  There is
        no adaptive capped, sink, window, long or quantised call: such a bank raises :class:`EkvError`."""
        bounds = plan.head_adaptive
        if not (isinstance(bounds, (tuple, list)) and len(bounds) == 2 and all(isinstance(x, int) and not isinstance(x, bool) for x in bounds)):
            raise ValueError(f"StepPlan.head_adaptive is (evict_min, evict_max), two integers, not {bounds!r}")
        if not (isinstance(plan.pool, int) and not isinstance(plan.pool, bool) and plan.pool >= 1 and plan.pool % 2 == 1):
            raise ValueError(f"StepPlan.pool is the kernel size of the pooling: an odd integer >= 1, not {plan.pool!r}")
        if plan.pool_op not in _lib.POOL_OPS:
            raise ValueError(f"StepPlan.pool_op must be 'max' or 'avg', not {plan.pool_op!r}")
        for what, on in (("logit_cap", self.logit_cap is not None), ("sinks", self.sinks is not None), ("windows", self.windows is not None),
                         ("long_rows=True", self.long_rows), (f"kv_quant={self.kv_quant!r}", self._fmt is not None)):
            if on:
                raise _lib.EkvError(f"an adaptive step (StepPlan.head_adaptive) on a bank created with {what}: there is no adaptive "
                                    f"{what.split('=')[0].replace('_', ' ')} call (adaptive head budgets serve plain 16-bit banks)")
        if self._ada_out is None:
            self._ada_out = torch.zeros(self.n_layers, self.n_kv_heads, dtype=torch.int32, device=self.device)
        key = self._ada_key(plan)
        fam = self._ada_fams.get(key)
        if fam is None:
            desc = _lib.Ada(*key, self._ada_out.data_ptr())      # (kept alive with the bank: a deferred token step caches the reference)
            fam = self._ada_fams[key] = tuple(getattr(self.lib, _lib.ADA_CALLS[what]) for what in _lib.STEP_CALLS) + ((C.byref(desc),), desc)
        return fam[:5]

    @staticmethod
    def _ada_key(plan):
        return (plan.pool // 2, _lib.POOL_OPS[plan.pool_op], int(plan.head_adaptive[0]), int(plan.head_adaptive[1]))

    def _ada_finish(self, layer_begin, lc, t):
        """After an adaptive step of layers [layer_begin, layer_begin + lc) over ``t`` rows: ONE device-to-host copy of the heads' victim
        counts; ``head_slots[l][h]`` = rows head h of layer l holds now, ``n_slots[l]`` their maximum (positions [head_slots, n_slots) of
        a shorter head's slot map are its free tail)."""
        k = self._ada_out[layer_begin:layer_begin + lc].cpu().tolist()
        if self.head_slots is None:
            self.head_slots = [None] * self.n_layers
        for i, row in enumerate(k):
            self.head_slots[layer_begin + i] = [t - x for x in row]
            self.n_slots[layer_begin + i] = max(self.head_slots[layer_begin + i])

    def _ada_row(self, plan, layer_begin):
        """Point the n_evict_out of ``plan``'s adaptive struct at row ``layer_begin`` (row i of a call is layer layer_begin + i).  The struct
        is shared by every step of the same pooling and bounds, so each call that launches sets it first."""
        self._ada_fams[self._ada_key(plan)][5].n_evict_out = self._ada_out.data_ptr() + 4 * layer_begin * self.n_kv_heads

    def _ada_ids(self, plan, lc, evict_ids):
        """The evict_ids of an adaptive step: ``[lc][H][evict_max]`` int32 on the bank's device, whatever the caller wants back — the
        scorer writes head h's entries at pitch evict_max.  A caller's tensor of any other shape, type or place is refused; a fresh one
        is filled with -1 (entries beyond a head's own count are left unwritten)."""
        shape = (lc, self.n_kv_heads, int(plan.head_adaptive[1]))
        if evict_ids is None or evict_ids is False:
            return torch.full(shape, -1, dtype=torch.int32, device=self.device)
        dev = torch.device(self.device)
        elsewhere = evict_ids.device.type != dev.type or (dev.index is not None and evict_ids.device.index != dev.index)
        if tuple(evict_ids.shape) != shape or evict_ids.dtype != torch.int32 or elsewhere or not evict_ids.is_contiguous():
            raise ValueError(f"evict_ids of an adaptive step must be a contiguous int32 tensor {list(shape)} ([layers][H][evict_max]) on {self.device}, "
                             f"not {list(evict_ids.shape)} {evict_ids.dtype} on {evict_ids.device}")
        return evict_ids

    def _ragged(self, layer_begin, lc):
        return self.head_slots is not None and any(r is not None for r in self.head_slots[layer_begin:layer_begin + lc])

    def ragged(self, layer):
        """Do the heads of ``layer`` hold different numbers of rows (an adaptive step ran on it)?"""
        return self._ragged(layer, 1)

    def _refuse_ragged(self, layer_begin, lc):
        if self._ragged(layer_begin, lc):
            raise _lib.EkvError("the heads of these layers hold different numbers of rows (an adaptive step ran): they take plain decode steps "
                                "(attend with phase='decode', whole call, plain keys) and nothing else until reset()")

    def _attend_ragged(self, plan, q, k_new, v_new, layer_begin, out, evict_ids):
        """A decode step of layers whose heads hold different numbers of rows (after an adaptive step), with no new attention kernel: the
        bank ``[L][H][cap]`` is byte for byte a bank of ``L * H`` layers with ONE KV head and ``rep`` query heads — K / V rows, slot
        maps, score rows, arrival counters, births and slot states are all indexed by ``layer * H + head`` — so one layer's step is the
        batched call (``ekv_batch_step_attend``, include/easykv_hip.h) on that view: ``H`` table entries ``{layer = l * H + h, n_slots =
        T_h + 1}``, and the layer's ``q`` / ``out`` ``[H * rep][1][D]`` and ``k_new`` / ``v_new`` ``[H][1][D]`` are the call's own
        ``[entries][rep][1][D]`` / ``[entries][1][1][D]``.  One call per layer.  Every entry evicts one row (every T_h stays put) or none
        (every head grows by one), as the plan says.  The batch call's limits hold: H <= 64, GQA <= 8, at most 6144 slots per head and
        cap % 4 == 0 for scored steps; the library refuses anything else before a launch."""
        lc, H = q.shape[0], self.n_kv_heads
        if any(self._slot_rows[layer_begin:layer_begin + lc]):
            self._ensure_ordered()
        if any(ev is not None for ev in self._score_done[layer_begin:layer_begin + lc]):
            self.join()
        if out is None:
            out = torch.empty(lc, self.n_q_heads, 1, self.head_dim, dtype=self.dtype, device=self.device)
        q, k_new, v_new = (t.to(self.device, self.dtype).contiguous() for t in (q, k_new, v_new))
        if not out.is_contiguous():
            raise ValueError("out of a step over heads of different lengths must be contiguous")
        if self._view is None:      # (made once per bank: the view struct, the two library calls, one table per layer)
            b = self._bank
            self._view = (_lib.Bank(b.k, b.v, b.slot_of_pos, b.score_sum, b.score_sq, b.score_cnt, self.n_layers * H, self.n_q_heads // H, 1, self.head_dim,
                                    self.cap, b.arrive, b.birth, b.slot_state),
                          {what: getattr(self.lib, _lib.step_call_name(None, True, what)) for what in ("workspace_bytes", "step_attend")},
                          [(_lib.Seq * H)() for _ in range(self.n_layers)])
        view, calls, tables = self._view
        first = self.make_step(plan, 1, layer_begin, 1)
        want_ids = evict_ids is not False and first.n_evict > 0
        if first.n_evict > 0 and (evict_ids is None or evict_ids is False):
            evict_ids = torch.empty(lc, H, 1, dtype=torch.int32, device=self.device)
        elif first.n_evict > 0 and (tuple(evict_ids.shape) != (lc, H, 1) or evict_ids.dtype != torch.int32 or not evict_ids.is_contiguous()
                                    or evict_ids.device.type != torch.device(self.device).type):
            raise ValueError(f"evict_ids of this decode step must be a contiguous int32 tensor [{lc}, {H}, 1] on {self.device}")
        _lib.set_resident_bytes(self.resident_bytes)
        for i in range(lc):
            l = layer_begin + i
            lens = self.head_slots[l] if self.head_slots[l] is not None else [self.n_slots[l]] * H
            st = self.make_step(plan, 1, l, 1)
            st.layer_begin, st.layer_count, st.n_split = 0, H, plan.n_split
            st.q_token_stride = st.q_head_stride = st.kv_token_stride = st.kv_head_stride = st.out_token_stride = st.out_head_stride = 0
            tb = tables[l]
            for h, e in enumerate(tb):
                e.layer, e.n_slots, e.score_off, e.n_evict = l * H + h, lens[h] + 1, st.score_off, st.n_evict
                e.phys_extent = max(self.extent[l], lens[h] + 1)
                e.win_lo, e.win_tail, e.roco_k1, e.range_start = st.win_lo, st.win_tail, st.roco_k1, st.range_start
            if max(lens) + 1 > self.cap:
                raise ValueError(f"layer {l}: a head holds {max(lens)} rows, the bank's capacity is {self.cap}")
            ws = self._workspace(calls["workspace_bytes"](C.byref(view), C.byref(st), self._dt, tb, H))
            check(calls["step_attend"](C.byref(view), C.byref(st), self._dt, tb, H, _ptr(q[i]), _ptr(k_new[i]), _ptr(v_new[i]), _ptr(out[i]),
                                       _ptr(evict_ids[i]) if st.n_evict > 0 else None, _ptr(ws), ws.numel(), self._stream()), "ekv_batch_step_attend")
            self.head_slots[l] = [t + 1 - st.n_evict for t in lens]
            self.n_slots[l] = max(self.head_slots[l])
            self.extent[l] = max(e.phys_extent for e in tb)
            self._tokens[l] += 1
        return out, (evict_ids if want_ids else None)

    # -- deferred decode steps over heads of different lengths: the heads family (ekv_heads_*, include/easykv_hip.h) ------------------
    def _heads_sync(self):
        """Make the device table of the heads family describe the bank's lengths now; returns (uploads, grow), the table's version.  The
        table ``[n_layers][H]`` (a layer whose heads are alike counts with ``n_slots``) is written when the lengths are not what the last
        step left: after an adaptive step, after a hand-over (a new bank), or when the layers' growths differ.  Uniform growth — every head
        of every layer longer by the same count — only advances ``grow``; unchanged lengths (evicting steps) touch nothing."""
        H = self.n_kv_heads
        hs = self.head_slots
        cur = [x for l in range(self.n_layers) for x in (hs[l] if hs[l] is not None else [self.n_slots[l]] * H)]
        h = self._heads
        if h is None:
            n = self.n_layers * H
            h = self._heads = dict(dev=torch.zeros(self.n_layers, H, dtype=torch.int32, device=self.device), host=(C.c_int32 * n)(), base=None, expect=None,
                                   fam=tuple(getattr(self.lib, _lib.HEADS_CALLS[what]) for what in _lib.STEP_CALLS))
            h["desc"] = _lib.Heads(h["dev"].data_ptr(), C.addressof(h["host"]), 0)
            h["ref"] = C.byref(h["desc"])
        if h["expect"] != cur:
            base = h["base"]
            g = cur[0] - base[0] if base is not None else -1
            if g >= 0 and all(c - b == g for c, b in zip(cur, base)):
                h["desc"].grow = g
            else:
                h["host"][:] = cur
                h["dev"].copy_(torch.tensor(cur, dtype=torch.int32).view(self.n_layers, H))
                h["base"], h["desc"].grow = cur, 0
                self.head_table_uploads += 1
            h["expect"] = cur
        return self.head_table_uploads, h["desc"].grow

    def _heads_plain(self, plan, n):
        """The steps the heads family takes: what _attend_ragged takes — a plain decode plan on plain keys.  Anything else on ragged layers
        keeps raising."""
        if not (n == 1 and plan.phase == "decode" and plan.head_adaptive is None and plan.pool == 1 and not plan.streaming):
            self._refuse_ragged(0, self.n_layers)

    def _heads_step(self, plan, d):
        """Open a token step of the heads family: everything that is the same for all its layers, resolved once per token step (as
        _attend_deferred does for the uniform form: the step struct, the flush's check, the workspace and a fresh ``ids`` tensor are made
        anew every token).  The flush's shape is validated before the first layer's attention appends a row."""
        if any(self._slot_rows):
            self._ensure_ordered()
        if any(ev is not None for ev in self._score_done):
            self.join()
        version = self._heads_sync()
        h = self._heads
        st = self.make_step(plan, 1, 0, 1)      # (n_slots is ignored by the family: the table has every head's)
        head = (C.byref(self._bank), C.byref(st), self._dt, h["ref"])
        st.defer_layers = self.n_layers
        if plan.n_split <= 0:      # the split count of a one-layer launch of the envelope (the layer of the longest head), fixed for both halves of the step
            st.phases, st.n_split, st.defer_layers = 1, 0, 0
            st.layer_begin = h["expect"].index(max(h["expect"])) // self.n_kv_heads
            info = (C.c_int32 * 10)()
            check(h["fam"][1](*head, info, 10), "ekv_heads_step_info")
            st.n_split, st.defer_layers = int(info[0]), self.n_layers
        st.layer_begin, st.layer_count, st.defer_index, st.phases = 0, self.n_layers, 0, 8
        st.phys_extent = 0
        check(h["fam"][0](*head), "ekv_heads_step_check (deferred scorer)")
        ws = self._workspace(h["fam"][2](*head))
        ids = torch.empty(self.n_layers, self.n_kv_heads, 1, dtype=torch.int32, device=self.device) if st.n_evict > 0 else None
        d = self._defer = dict(plan=plan, t=-2, n=1, st=st, ws=ws, ids=ids, pending=0, heads=version, ws_ptr=ws.data_ptr(), ws_len=ws.numel(),
                               stream=self._stream(), call=h["fam"][3], head=head)
        return d

    def _attend_heads(self, plan: StepPlan, q, k_new, v_new, layer, out):
        """Deferred step of ONE layer of a bank whose heads hold different numbers of rows: attention + in-kernel fold of this layer now, by
        the heads family's split kernel on the layer's own (KV head) grid — every workgroup reads its head's row count from the device
        table — and ONE scorer launch over all layers and heads at :meth:`flush`, exactly like a uniform bank's deferred step."""
        self._heads_plain(plan, q.shape[2])
        d = self._defer
        if d is not None and d["pending"] and (d.get("heads") is None or d["plan"] is not plan or d["pending"] >= self.n_layers):
            raise _lib.EkvError("attend(defer=True): the previous step was not flushed")
        if d is None or d["pending"] == 0:
            d = self._heads_step(plan, d)
        st = d["st"]
        st.layer_begin = st.defer_index = layer
        st.layer_count, st.phases = 1, 5
        lens = self.head_slots[layer]
        t = (max(lens) if lens is not None else self.n_slots[layer]) + 1
        ext = self.extent[layer]
        st.phys_extent = ext if ext > t else t
        if out is None:
            out = torch.empty(1, self.n_q_heads, 1, self.head_dim, dtype=self.dtype, device=self.device)
        q, k_new, v_new = _stride_rows(st, q, k_new, v_new, out, self.dtype)
        rc = d["call"](*d["head"], q.data_ptr(), k_new.data_ptr(), v_new.data_ptr(), out.data_ptr(), None, d["ws_ptr"], d["ws_len"], d["stream"])
        if rc != 0:
            check(rc, "ekv_heads_step_attend")
        self.extent[layer] = st.phys_extent
        self._tokens[layer] += 1
        d["pending"] += 1
        return out

    def _flush_heads(self, d):
        """The flush of a heads token step: the one scorer call over all layers; ``[L][H][1]`` ids (or None); lengths, extents and the
        table's expectation advance as _attend_ragged advances them per layer."""
        st, ws, H = d["st"], d["ws"], self.n_kv_heads
        st.layer_begin, st.layer_count, st.defer_index, st.phases = 0, self.n_layers, 0, 8
        st.q_token_stride = st.q_head_stride = st.kv_token_stride = st.kv_head_stride = st.out_token_stride = st.out_head_stride = 0
        st.phys_extent = 0
        p = ws.data_ptr()
        check(d["call"](*d["head"], p, p, p, p, _ptr(d["ids"]), p, ws.numel(), d["stream"]), "ekv_heads_step_attend")
        for l in range(self.n_layers):
            lens = self.head_slots[l] if self.head_slots[l] is not None else [self.n_slots[l]] * H
            self.head_slots[l] = [t + 1 - st.n_evict for t in lens]
            self.n_slots[l] = max(self.head_slots[l])
        h = self._heads
        if st.n_evict == 0:      # every head grew by one row: the table stands, its growth advances
            h["desc"].grow += 1
            h["expect"] = [x + 1 for x in h["expect"]]
        d["pending"] = 0
        return d["ids"] if st.n_evict > 0 else None

    def _step_check(self, st, fam=None):
        fam = fam or self._family()
        return fam[0](C.byref(self._bank), C.byref(st), self._dt, *fam[4])

    def _step_ws_bytes(self, st, fam=None):
        fam = fam or self._family()
        return fam[2](C.byref(self._bank), C.byref(st), self._dt, *fam[4])

    def _step_attend(self, st, *args, fam=None):
        fam = fam or self._family()
        _lib.set_resident_bytes(self.resident_bytes)
        return fam[3](C.byref(self._bank), C.byref(st), self._dt, *fam[4], *args)

    # -- plumbing -----------------------------------------------------------------------------
    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self._dev_index).cuda_stream)

    def _workspace(self, nbytes):
        if self._ws is None or self._ws.numel() < nbytes:
            self._ws = torch.empty(int(nbytes * 1.25) + 4096, dtype=torch.uint8, device=self.device)
        return self._ws

    def release_workspace(self, keep_bytes=0):
        """Drop the cached scratch buffer when it is larger than ``keep_bytes`` (a deferred chunk step of a long prefill keeps every
        layer's logits / column sums alive until the flush: up to GBs that the decode phase after it never needs)."""
        if self._ws is not None and self._ws.numel() > keep_bytes and (self._defer is None or not self._defer["pending"]):
            self._ws = None
            self._defer = None      # (its cached pointers referred to the buffer)

    def reset(self):
        check(self.lib.ekv_bank_reset(C.byref(self._bank), self._stream()), "ekv_bank_reset")
        self.n_slots = [0] * self.n_layers
        self.head_slots = None
        if self._heads is not None:
            self._heads["base"] = self._heads["expect"] = None      # (the next ragged step writes the table anew)
        self.extent = [0] * self.n_layers
        self._slot_rows = [False] * self.n_layers
        self._slot_min_tail = [1 << 30] * self.n_layers
        self._slot_stretch = self._slot_short = self._slot_cool = 0
        self._defer = None      # (a half-open deferred token step dies with the bank's contents; arrive[] is zeroed by the reset)
        self._tokens = [0] * self.n_layers

    def abort_step(self):
        """Drop a deferred token step that was opened (``attend(..., defer=True)`` on some layers) but never flushed — a model
        forward that raised half-way through the stack.  The layers that did attend have written the new token's row into the
        slot their free list pointed at, but ``n_slots`` has not advanced, so the next step of every layer reuses that very
        slot: the bank is as it was before the aborted token.  Returns the number of layers that had attended."""
        d, n = self._defer, 0
        if d is not None:
            n, d["pending"], d["t"] = d["pending"], 0, -1
            if n:   # a launch that died mid-way could leave arrival counters of the in-kernel fold non-zero
                self.arrive.zero_()
        return n

    def state_init(self, width, mode, stride=1, layer_begin=0, layer_count=None):
        """mode 0 decoding (easykv/easykv.py:242-245); 1 prefill+keep_attention; 2 prefill (:412-416)."""
        lc = self.n_layers - layer_begin if layer_count is None else layer_count
        self._ensure_ordered(layer_begin, lc)      # (the slot map is not rewritten by the initialisation)
        check(self.lib.ekv_state_init(C.byref(self._bank), layer_begin, lc, width, mode, stride, self._stream()), "ekv_state_init")

    def set_rope(self, cos, sin):
        """fp32 tables ``[>= cap, head_dim]`` for the streaming (rope-on-read) variant."""
        self._quant_refuse(True, "set_rope (RoPE-on-read)")
        if self.logit_cap is not None:
            raise _lib.EkvError("set_rope(): RoPE-on-read has no soft-capped build (a bank created with logit_cap serves plain keys only)")
        if self.sinks is not None:
            raise _lib.EkvError("set_rope(): RoPE-on-read has no sink build (a bank created with sinks serves plain keys only)")
        if self.windows is not None:
            raise _lib.EkvError("set_rope(): RoPE-on-read has no window build (a bank created with windows serves plain keys only)")
        if self.head_dim in PLAIN_KEYS_HEAD_DIMS:
            raise _lib.EkvError(f"set_rope(): RoPE-on-read has no build for head_dim {self.head_dim} (plain keys only)")
        self.rope_cos = cos.to(self.device, torch.float32).contiguous()
        self.rope_sin = sin.to(self.device, torch.float32).contiguous()
        half = self.head_dim // 2
        # the kernels read only the first half of a table row for both halves of the head (the reference's tables are
        # cat(freqs, freqs), llama_patch.py:74-98 / HF rotary modules)
        if not (torch.equal(self.rope_cos[:, :half], self.rope_cos[:, half:]) and torch.equal(self.rope_sin[:, :half], self.rope_sin[:, half:])):
            raise _lib.EkvError("rope tables must have the cat(freqs, freqs) layout (equal halves along head_dim)")
        # ... and must be a rotation that is linear in the position, row j = (cos(j * theta_f), sin(j * theta_f)): the decode stream
        # reads one row per run of consecutive positions and advances (cos, sin) by the angle-addition recurrence with row 1 as the
        # step (include/easykv_hip.h).  Every RoPE variant is (linear / NTK / llama3 / yarn only change theta_f); the tables' own fp32
        # rounding of the angle (6e-8 * j * theta_f) is the only deviation allowed for.
        if self.rope_cos.shape[0] > 2:
            c, s_ = self.rope_cos[:, :half].double(), self.rope_sin[:, :half].double()
            dev_c = (c[:-1] * c[1] - s_[:-1] * s_[1] - c[1:]).abs().max()
            dev_s = (s_[:-1] * c[1] + c[:-1] * s_[1] - s_[1:]).abs().max()
            if float(torch.maximum(dev_c, dev_s)) > 1e-4 + 4e-7 * self.rope_cos.shape[0]:
                raise _lib.EkvError("rope tables must be rotations linear in the position: row j = (cos(j * theta), sin(j * theta)) per frequency")

    # -- data movement at the boundary -------------------------------------------------------------
    def load_rows(self, k, v, pos_begin=None, layer_begin=0, tok_pos=None):
        """Append ordered rows ``[layers, H, n, D]`` at positions [pos_begin, pos_begin+n).  A window bank stamps the rows' token
        positions: ``tok_pos=None`` the ``n`` positions after the tokens the layers have seen, or a given int ``[layers, H, n]``,
        increasing along ``n`` (a cache with gaps, different per head); the layers have then seen ``max + 1`` tokens."""
        lc, n = k.shape[0], k.shape[2]
        self._quant_refuse(True, "load_rows")
        if tok_pos is not None and self.windows is None:
            raise _lib.EkvError("load_rows(tok_pos=...): the bank was created without windows")
        if self.windows is not None:      # (before anything is written)
            if tok_pos is None:
                base = self._tokens[layer_begin]
                tok_pos = (base + torch.arange(n, dtype=torch.int32, device=self.device)).expand(lc, self.n_kv_heads, n)
                seen = base + n
            else:
                tok_pos = torch.as_tensor(tok_pos).to(self.device, torch.int32)
                if tuple(tok_pos.shape) != (lc, self.n_kv_heads, n) or bool((tok_pos[..., 1:] <= tok_pos[..., :-1]).any()) or bool((tok_pos < 0).any()):
                    raise ValueError(f"load_rows(tok_pos=...) must be [layers, H, n] = [{lc}, {self.n_kv_heads}, {n}], >= 0 and increasing along n")
                seen = int(tok_pos.max()) + 1
        self._ensure_ordered(layer_begin, lc)
        pos = self.n_slots[layer_begin] if pos_begin is None else pos_begin
        k = k.to(self.device, self.dtype).contiguous()
        v = v.to(self.device, self.dtype).contiguous()
        check(self.lib.ekv_scatter_rows(C.byref(self._bank), layer_begin, lc, pos, n, _ptr(k), _ptr(v), self._stream()), "ekv_scatter_rows")
        for l in range(layer_begin, layer_begin + lc):
            self.n_slots[l] = pos + n
            self.extent[l] = max(self.extent[l], pos + n)
        if self.windows is not None:      # (rows never move: the position goes where the slot map sent the row)
            slots = self._slot_of_pos[layer_begin:layer_begin + lc, :, pos:pos + n].long()
            self.tok_pos[layer_begin:layer_begin + lc].scatter_(2, slots, tok_pos.contiguous())
            for l in range(layer_begin, layer_begin + lc):
                self._tokens[l] = max(self._tokens[l], seen)

    def ordered_kv(self, layer_begin=0, layer_count=None):
        """The ordered ``[layers, H, T, D]`` view the HF legacy tuple needs (birth order)."""
        lc = self.n_layers - layer_begin if layer_count is None else layer_count
        self._quant_refuse(True, "ordered_kv (a row move)")
        self._ensure_ordered(layer_begin, lc)
        # (after an adaptive step: the longest head of these layers; a shorter head's rows [head_slots, t) are its evicted ones)
        t = self.n_slots[layer_begin] if self.head_slots is None else max(self.n_slots[layer_begin:layer_begin + lc])
        k = torch.empty(lc, self.n_kv_heads, t, self.head_dim, dtype=self.dtype, device=self.device)
        v = torch.empty_like(k)
        check(self.lib.ekv_gather_ordered(C.byref(self._bank), layer_begin, lc, t, _ptr(k), _ptr(v), self._stream()), "ekv_gather_ordered")
        return k, v

    def hand_over(self, cap):
        """A new bank of capacity ``cap`` that holds this bank's live rows and nothing else: step 4 of the one-shot prefill
        (include/easykv_hip.h), where a prompt-sized bank has just been cut to the budget in one step and its ``T`` retained rows lie
        scattered over ``extent`` = the prompt's physical rows.  In the new bank the rows of every head sit in logical order in the physical
        rows ``[0, T)`` (``ekv_gather_ordered`` out of this bank, ``load_rows`` into the fresh one, whose slot map is the identity), so
        ``extent == T`` and a one-launch decode step streams ``T`` rows, not the prompt's.  The score rows' first ``T`` columns, the
        softmax scale / cap / sinks and — a window bank — the rows' token positions and the tokens seen are carried over.  Every layer must
        hold the same number of rows — unless an adaptive step left the heads with different lengths: then ``T`` is the longest head's
        count, every head's first ``T`` positions are gathered (a shorter head's live rows come first, its free tail behind them) and
        ``head_slots`` is carried over; a quantised bank, a bank on the slot-indexed layout mid-capture or with an open deferred step
        raises.  This bank is left as it is: the caller drops it."""
        self._quant_refuse(True, "hand_over (a row move)")
        if self._defer is not None and self._defer["pending"]:
            raise _lib.EkvError("hand_over(): a deferred token step is open (flush() first)")
        ragged = self._ragged(0, self.n_layers)      # (after an adaptive step: the longest head's count, of every head)
        t = max(self.n_slots) if ragged else self.n_slots[0]
        if not ragged and any(n != t for n in self.n_slots):
            raise _lib.EkvError(f"hand_over(): the layers hold different numbers of rows {sorted(set(self.n_slots))}")
        if t < 1 or cap < t:
            raise ValueError(f"hand_over(cap={cap}): the bank holds {t} rows per head")
        self.join()
        scored = self._score_sum is not None
        extra = {k: v for k, v in (("logit_cap", self.logit_cap), ("sm_scale", self.sm_scale), ("sinks", self.sinks),
                                   ("windows", None if self.windows is None else list(self.windows))) if v is not None}
        new = KVBank(self.n_layers, self.n_q_heads, self.n_kv_heads, self.head_dim, cap, device=self.device, scored=scored, dtype=self.dtype,
                     long_rows=self.long_rows, **extra)
        new.resident_bytes = self.resident_bytes
        k, v = self.ordered_kv()
        new.load_rows(k, v, 0, tok_pos=None if self.windows is None else self.ordered_tok_pos())
        if scored:
            for name in ("_score_sum", "_score_sq", "_score_cnt"):      # (ordered layout: ordered_kv brought this bank back to it)
                getattr(new, name)[:, :, :t].copy_(getattr(self, name)[:, :, :t])
        new._tokens = list(self._tokens)
        if ragged:      # (identity slot map: head h's live rows are [0, T_h), its free tail starts at T_h; the score columns past T_h are zero)
            new.head_slots = [list(r) if r is not None else [self.n_slots[l]] * self.n_kv_heads for l, r in enumerate(self.head_slots)]
            new.n_slots = [max(r) for r in new.head_slots]
        return new

    def compact_inplace(self, evict_ids, layer_begin=0):
        """Reference-shaped physical compaction for a bank kept in identity layout."""
        lc, _, kk = evict_ids.shape
        self._quant_refuse(True, "compact_inplace (a row move)")
        if self.windows is not None:
            raise _lib.EkvError("compact_inplace(): a bank created with windows keeps the token position of a row with the row; rows do not move")
        self._ensure_ordered(layer_begin, lc)
        t = self.n_slots[layer_begin]
        ids = evict_ids.to(self.device, torch.int32).contiguous()
        check(self.lib.ekv_compact_inplace(C.byref(self._bank), layer_begin, lc, t, kk, _ptr(ids), self._stream()), "ekv_compact_inplace")
        for l in range(layer_begin, layer_begin + lc):
            self.n_slots[l] = t - kk

    # -- the fused step -----------------------------------------------------------------------------
    def make_step(self, plan: StepPlan, q_len, layer_begin, layer_count) -> Step:
        t = self.n_slots[layer_begin] + q_len
        st = Step()
        st.layer_begin, st.layer_count, st.q_len, st.n_slots = layer_begin, layer_count, q_len, t
        st.score_off = plan.score_off
        st.policy = _lib.POLICY_CODES.get(plan.policy, _lib.POLICY_NONE)   # unknown string = no-op, as in the reference
        st.accumulate = int(plan.accumulate)
        st.causal = 1
        st.rope_on_read = int(plan.streaming)
        st.n_split = plan.n_split
        st.two_pass = plan.two_pass or KVBank.default_two_pass
        st.sm_div = math.sqrt(self.head_dim) if self.sm_scale is None else 1.0 / self.sm_scale
        st.tova_head_mean = int(plan.tova_head_mean)
        st.roco_tail = ROCO_TAIL
        st.range_start = -1
        st.phys_extent = max(max(self.extent[layer_begin:layer_begin + layer_count]), t)
        if plan.evict and st.policy != _lib.POLICY_NONE:
            if plan.phase == "decode":
                rw = int(plan.budget * DECODE_RECENT_RATIO)
                st.n_evict = 1
                st.win_lo, st.win_tail = (0, rw) if plan.policy == "h2o_head" else (0, 0)
                st.roco_k1 = plan.budget - rw
                st.count_add, st.count_tail_step = 1.0, 0.0
            else:
                st.n_evict = plan.stride if plan.n_evict is None else plan.n_evict
                st.win_lo, st.win_tail = plan.sink, plan.recent
                st.roco_k1 = max(plan.budget - plan.recent - plan.sink, st.n_evict)
                st.count_add, st.count_tail_step = float(plan.stride), -1.0
            if st.policy == _lib.POLICY_RANGE:
                st.range_start = plan.range_start
        return st

    def step_plan(self, plan: StepPlan, q_len, layer_begin=0, layer_count=None, phases=0):
        """(n_split, fused) the library will use for this step."""
        st = self.make_step(plan, q_len, layer_begin, self.n_layers - layer_begin if layer_count is None else layer_count)
        st.phases = phases
        if self._fmt is not None or self.long_rows or self.logit_cap is not None or self.sinks is not None or self.windows is not None or plan.pool != 1 or plan.head_adaptive is not None:      # (the dry run of the bank's own family / the step's: a step it refuses plans as not fused)
            info = self.step_info(plan, q_len, layer_begin, layer_count, phases)
            return info["n_split"], bool(info["fused"])
        ns, fu = C.c_int32(0), C.c_int32(0)
        check(self.lib.ekv_step_plan(C.byref(self._bank), C.byref(st), C.byref(ns), C.byref(fu)), "ekv_step_plan")
        return ns.value, bool(fu.value)

    def step_info(self, plan: StepPlan, q_len, layer_begin=0, layer_count=None, phases=0) -> dict:
        """The library's dispatch decisions for this step (ekv_step_info): n_split, fused, two_pass, wide, n_qblocks, ..."""
        st = self.make_step(plan, q_len, layer_begin, self.n_layers - layer_begin if layer_count is None else layer_count)
        st.phases = phases
        n_info = _lib.LONG_INFO_N if self.long_rows else 10
        info = (C.c_int32 * n_info)()
        fam = self._family(plan)
        check(fam[1](C.byref(self._bank), C.byref(st), self._dt, *fam[4], info, n_info), fam[1].__name__)
        keys = ("n_split", "fused", "two_pass", "wide", "n_qblocks", "qb_rows", "n_col_parts", "fold_in_kernel", "n_launches", "fused_order",
                "long_scorer", "long_tiles")      # (the last two: a long_rows bank only)
        return dict(zip(keys, (int(x) for x in info)))

    def resident_rows(self, plan: StepPlan, q_len=1, layer_begin=0, layer_count=None, phases=0) -> int:
        """Resident rows the library plans this step's launch with (ekv_step_resident_rows) under this bank's ``resident_bytes``;
        0 for a quantised bank."""
        if self._fmt is not None or self.sinks is not None or self.windows is not None:      # (the sink and the window instances are built without resident rows, as the kv164 ones)
            return 0
        st = self.make_step(plan, q_len, layer_begin, self.n_layers - layer_begin if layer_count is None else layer_count)
        st.phases = phases
        _lib.set_resident_bytes(self.resident_bytes)
        rows = self.lib.ekv_step_resident_rows(C.byref(self._bank), C.byref(st), self._dt)
        if rows < 0:
            check(rows, "ekv_step_resident_rows")
        return rows

    def join(self):
        """Make the current stream wait for every scorer still running on a side stream."""
        cur = torch.cuda.current_stream(self.device)
        for l, ev in enumerate(self._score_done):
            if ev is not None:
                cur.wait_event(ev)
                self._score_done[l] = None
        self._ws_free = [None] * len(self._ws_free)     # every scorer joined: all workspace slots are free again

    def _attend_overlapped(self, st, q, k_new, v_new, out, evict_ids, lc, layer_begin):
        """Attention + fold on the current stream (the attention output is ready as early as possible); the scorer
        (accumulate / select / compaction) on a side stream.  The next attention of these layers waits for it."""
        if self._side is None:
            self._side = [torch.cuda.Stream(self.device) for _ in range(4)]
        main = torch.cuda.current_stream(self.device)
        need = self._step_ws_bytes(st)
        if not self._ws_ring or self._ws_ring[0].numel() < need:
            self._ws_ring = [torch.empty(int(need * 1.25) + 4096, dtype=torch.uint8, device=self.device) for _ in range(8)]
            self._ws_free = [None] * 8
        slot = self._ring_pos
        self._ring_pos = (slot + 1) % len(self._ws_ring)
        ws = self._ws_ring[slot]
        for ev in [self._ws_free[slot]] + self._score_done[layer_begin:layer_begin + lc]:
            if ev is not None:
                main.wait_event(ev)      # workspace slot free again; slot map / score rows of these layers up to date
        args = (_ptr(q), _ptr(k_new), _ptr(v_new), _ptr(out), _ptr(evict_ids) if st.n_evict > 0 else None,
                _ptr(self.rope_cos), _ptr(self.rope_sin), _ptr(ws), ws.numel())
        st.phases = 1 | 4
        check(self._step_attend(st, *args, C.c_void_p(main.cuda_stream)), "ekv_step_attend")
        ready = torch.cuda.Event()
        ready.record(main)
        side = self._side[slot % len(self._side)]
        side.wait_event(ready)
        st.phases = 8
        check(self._step_attend(st, *args, C.c_void_p(side.cuda_stream)), "ekv_step_attend")
        done = torch.cuda.Event()
        done.record(side)
        self._ws_free[slot] = done
        for l in range(layer_begin, layer_begin + lc):
            self._score_done[l] = done

    # -- one layer per call (a real decoder stack): attention now, scoring / eviction once per token ------------------------
    def _attend_deferred(self, plan: StepPlan, q, k_new, v_new, layer, out, q_pos=None):
        """Step of ONE layer with the scorer deferred (ekv_step.defer_layers): attention + fold of this layer now — its output is
        what the next layer waits for — and one scorer launch over all layers of the bank at :meth:`flush`, instead of a
        latency-bound scorer kernel of 32 workgroups on the critical path of every layer (decode: 15 us of a 25 us layer; a
        96-row chunk step of the Llama2-7B shape: 66 us of a 124 us layer).  Decode steps and, since round 4, chunk steps."""
        d = self._defer
        n = q.shape[2]
        self._quant_refuse(n > 1, "a chunk step (q_len > 1)")
        self._refuse_ragged(layer, 1)
        t = self.n_slots[layer] + n
        if self._slot_rows[layer]:
            self._ensure_ordered()      # (all layers in one launch: the conversion ranks births by counting, ~0.2 ms per launch of <= 256 heads)
        if d is None or d["plan"] is not plan or d["t"] != t or d["n"] != n:
            if d is not None and d["pending"]:
                raise _lib.EkvError("attend(defer=True): the previous step was not flushed")
            st = self.make_step(plan, n, 0, 1)
            fam = self._family(plan)
            if plan.n_split <= 0:      # the split count of a one-layer launch, fixed for both halves of the step
                st.phases = 1
                st.n_split = self._planned_split(st, fam)
            st.defer_layers = self.n_layers
            # the scorer shape of the flush() call (phases = 8 over all layers) is validated NOW, before the first layer's
            # attention appends a row: a shape only the last call of the token would refuse must not leave the bank half-stepped
            st.layer_begin, st.layer_count, st.defer_index, st.phases = 0, self.n_layers, 0, 8
            check(self._step_check(st, fam), "ekv_step_check (deferred scorer)")
            need = self._step_ws_bytes(st, fam)
            ids = torch.empty(self.n_layers, self.n_kv_heads, st.n_evict, dtype=torch.int32, device=self.device) if st.n_evict > 0 else None
            if ids is not None and plan.head_adaptive is not None:
                ids = self._ada_ids(plan, self.n_layers, None)
            ws = self._workspace(need)
            # everything that is the same for all layers of the token step is resolved once: the per-layer call below is on the
            # critical path of the decoder stack (host cost per layer ~ GPU cost per layer in this regime)
            d = self._defer = dict(plan=plan, t=t, n=n, st=st, ws=ws, ids=ids, pending=0, rope=(_ptr(self.rope_cos), _ptr(self.rope_sin)),
                                   st_ref=C.byref(st), bank_ref=C.byref(self._bank), ws_ptr=ws.data_ptr(), ws_len=ws.numel(),
                                   stream=self._stream())
            # (the call and its leading arguments: the step of the bank's row format, a quantised one with the descriptor behind the dtype)
            d["call"], d["head"], d["fam"] = fam[3], (d["bank_ref"], d["st_ref"], self._dt, *fam[4]), fam
        st = d["st"]
        st.layer_begin = st.defer_index = layer
        st.layer_count, st.phases = 1, 5
        ext = self.extent[layer]
        st.phys_extent = ext if ext > t else t
        if out is None:
            out = torch.empty(1, self.n_q_heads, n, self.head_dim, dtype=self.dtype, device=self.device)
        q, k_new, v_new = _stride_rows(st, q, k_new, v_new, out, self.dtype)
        self._set_q_pos(layer, 1, q_pos)
        rc = d["call"](*d["head"], q.data_ptr(), k_new.data_ptr(), v_new.data_ptr(), out.data_ptr(), None,
                       d["rope"][0], d["rope"][1], d["ws_ptr"], d["ws_len"], d["stream"])
        if rc != 0:
            check(rc, "ekv_step_attend")
        self.extent[layer] = st.phys_extent
        self._tokens[layer] += n
        d["pending"] += 1
        return out

    def _planned_split(self, st, fam=None) -> int:
        """The split count the library plans for ``st`` (a capped bank: by its own family — a capped chunk step is tiled in narrower
        blocks than the plain call's; a pooled step: by the pooled family)."""
        fam = fam or self._family()
        if self.logit_cap is not None or self.sinks is not None or self.windows is not None or fam[1] is not self._info_fn:
            info = (C.c_int32 * 10)()
            check(fam[1](C.byref(self._bank), C.byref(st), self._dt, *fam[4], info, 10), fam[1].__name__)
            return int(info[0])
        ns, fu = C.c_int32(0), C.c_int32(0)
        check(self.lib.ekv_step_plan(C.byref(self._bank), C.byref(st), C.byref(ns), C.byref(fu)), "ekv_step_plan")
        return ns.value

    def deferred_workspace_bytes(self, plan: StepPlan, q_len: int) -> int:
        """Scratch a step of ``q_len`` queries needs when the scorers of all layers are deferred to :meth:`flush` (the logits / column
        sums of every layer stay alive until then)."""
        st = self.make_step(plan, q_len, 0, 1)
        fam = self._family(plan)
        if plan.n_split <= 0:
            st.phases = 1
            st.n_split = self._planned_split(st, fam)
        st.defer_layers, st.layer_begin, st.layer_count, st.defer_index, st.phases = self.n_layers, 0, self.n_layers, 0, 8
        return int(self._step_ws_bytes(st, fam))

    def flush(self):
        """Scorer of every layer of the token step opened by ``attend(..., defer=True)``: accumulate, select, compact — one
        launch.  Returns the evicted positions ``[layers, H, 1]`` (or None)."""
        d = self._defer
        if d is None or d["pending"] == 0:
            return None
        if d["pending"] != self.n_layers:
            raise _lib.EkvError(f"flush(): {d['pending']} of {self.n_layers} layers attended in this token step")
        if d.get("heads") is not None:
            return self._flush_heads(d)
        st, ws = d["st"], d["ws"]
        st.layer_begin, st.layer_count, st.defer_index, st.phases = 0, self.n_layers, 0, 8
        st.q_token_stride = st.q_head_stride = st.kv_token_stride = st.kv_head_stride = st.out_token_stride = st.out_head_stride = 0      # (no caller tensors in this call)
        st.phys_extent = max(max(self.extent), d["t"])
        adaptive = d["plan"].head_adaptive is not None
        if adaptive:
            self._ada_row(d["plan"], 0)
        check(self._step_attend(st, ws.data_ptr(), ws.data_ptr(), ws.data_ptr(), ws.data_ptr(),
                                _ptr(d["ids"]), d["rope"][0], d["rope"][1], ws.data_ptr(), ws.numel(), d["stream"], fam=d["fam"]), "ekv_step_attend")
        for l in range(self.n_layers):
            self.n_slots[l] = d["t"] - st.n_evict
        if adaptive:
            self._ada_finish(0, self.n_layers, d["t"])
        d["pending"] = 0
        d["t"] = -1
        return d["ids"] if st.n_evict > 0 else None

    def attend(self, plan: StepPlan, q, k_new, v_new, layer_begin=0, out=None, evict_ids=None, phases=0, overlap_scorer=False, defer=False,
               q_pos=None):
        """q ``[layers, Hq, n, D]``, k_new/v_new ``[layers, H, n, D]`` (the bank's dtype, device; dense or strided views whose rows are
        read in place — ekv_step.*_stride, see :func:`_row_strides`; anything else is converted / copied dense first).
        Returns (out ``[layers, Hq, n, D]`` in the bank's dtype, evict_ids ``[layers, H, k]`` int32 or None).
        ``defer=True`` (one layer per call): attention + fold only; the scorers of all layers run at :meth:`flush`.
        ``evict_ids=False``: the caller has no use for the evicted cache indices (none are returned; on the slot-indexed layout the
        step then skips ranking the victim's birth).
        ``q_pos`` (a window bank): the token position of the (first) query; None: the tokens these layers have seen, which the call advances."""
        if defer:
            if q.shape[0] != 1 or phases != 0:
                raise ValueError("defer=True is for one-layer calls")
            if self._ragged(0, self.n_layers):      # (a bank with a ragged layer steps through the heads family, all layers: one flush)
                return self._attend_heads(plan, q, k_new, v_new, layer_begin, out), None
            return self._attend_deferred(plan, q, k_new, v_new, layer_begin, out, q_pos), None
        lc, _, n, _ = q.shape
        self._quant_refuse(n > 1, "a chunk step (q_len > 1)")
        if self._ragged(layer_begin, lc):
            if not (n == 1 and plan.phase == "decode" and phases == 0 and not overlap_scorer and plan.head_adaptive is None and plan.pool == 1
                    and not plan.streaming):
                self._refuse_ragged(layer_begin, lc)
            return self._attend_ragged(plan, q, k_new, v_new, layer_begin, out, evict_ids)
        fam = self._family(plan)      # (a pooled step on a bank that has no pooled call raises here, before anything is written)
        pooled = fam[3] is not self._attend_fn
        adaptive = plan.head_adaptive is not None
        if adaptive:
            self._ada_row(plan, layer_begin)
        self._set_q_pos(layer_begin, lc, q_pos)
        st = self.make_step(plan, n, layer_begin, lc)
        # one-launch decode steps run on the slot-indexed layout of the score rows (nothing moves on an eviction); everything else
        # on the ordered one
        slot = n == 1 and phases == 0 and not overlap_scorer and not pooled and self._enter_slot_rows(st)
        if not slot and any(self._slot_rows[layer_begin:layer_begin + lc]):
            self._ensure_ordered()      # (all layers in one launch: a layer-per-call caller would otherwise convert 32 times)
        st.phases = phases | (_lib.PHASE_SLOT_ROWS if slot else 0)
        if slot and st.n_evict > 0:
            roco = st.policy == _lib.POLICY_ROCO
            tail = st.roco_tail if roco else st.win_tail
            # roco protects its newest entries by std = 1e9 sentinels only (easykv/easykv.py:318-321): when the feasible set has to
            # reach into them (k1 > T - tail: budgets below ~30) the arg-min over the mean may evict one of the newest `tail`
            # entries, and their births are no longer consecutive.  Such a step — and every step after it, until the next
            # conversion — leaves the proof to the kernel's counting check (exact bisection when it fails).
            breaks_tail = roco and st.roco_k1 > st.n_slots - st.roco_tail
            if not breaks_tail and all(tail <= self._slot_min_tail[l] for l in range(layer_begin, layer_begin + lc)):
                st.phases |= _lib.PHASE_SLOT_TAIL_OK
            for l in range(layer_begin, layer_begin + lc):
                self._slot_min_tail[l] = 0 if breaks_tail else min(self._slot_min_tail[l], tail)
        if out is None:
            out = torch.empty(lc, self.n_q_heads, n, self.head_dim, dtype=self.dtype, device=self.device)
        q, k_new, v_new = _stride_rows(st, q, k_new, v_new, out, self.dtype)
        want_ids = evict_ids is not False
        if adaptive and st.n_evict > 0:
            evict_ids = self._ada_ids(plan, lc, evict_ids)
        elif evict_ids is False:      # the caller has no use for the evicted order indices (the slot-indexed layout then skips ranking the victim)
            evict_ids = None if slot else torch.empty(lc, self.n_kv_heads, max(st.n_evict, 1), dtype=torch.int32, device=self.device)
        elif st.n_evict > 0 and evict_ids is None:
            evict_ids = torch.empty(lc, self.n_kv_heads, st.n_evict, dtype=torch.int32, device=self.device)
        if overlap_scorer and phases == 0 and not pooled and not self.step_plan(plan, n, layer_begin, lc)[1]:
            self._attend_overlapped(st, q, k_new, v_new, out, evict_ids, lc, layer_begin)
            for l in range(layer_begin, layer_begin + lc):
                self.n_slots[l] = st.n_slots - st.n_evict
                self.extent[l] = st.phys_extent
                self._tokens[l] += n
            return out, (evict_ids if (st.n_evict > 0 and want_ids) else None)
        if any(ev is not None for ev in self._score_done[layer_begin:layer_begin + lc]):
            self.join()
        need = self._step_ws_bytes(st, fam)
        ws = self._workspace(need)
        check(self._step_attend(st, _ptr(q), _ptr(k_new), _ptr(v_new), _ptr(out),
                                _ptr(evict_ids) if (st.n_evict > 0 and evict_ids is not None) else None, _ptr(self.rope_cos), _ptr(self.rope_sin),
                                _ptr(ws), ws.numel(), self._stream(), fam=fam), "ekv_step_attend")
        if phases != 1:     # phases == 1 launches the attention kernel only; the slot map is untouched
            for l in range(layer_begin, layer_begin + lc):
                self.n_slots[l] = st.n_slots - st.n_evict
            if adaptive and (phases == 0 or phases & (2 | 8)):
                self._ada_finish(layer_begin, lc, st.n_slots)
        for l in range(layer_begin, layer_begin + lc):      # the new rows are written by the attention kernel
            self.extent[l] = st.phys_extent
            if phases == 0 or phases & 1:      # (the calls that run the attention kernel, which appends the token's row)
                self._tokens[l] += n
        return out, (evict_ids if (st.n_evict > 0 and want_ids) else None)


class _BankSlice:
    """Layers ``[begin, begin + n_layers)`` of a bank as a bank of their own: the single-sequence calls of :class:`KVBank` with the
    layer arguments shifted.  It owns nothing: rows, slot maps, score rows, ``n_slots`` / ``extent`` and the layout bookkeeping
    (which layers hold the slot-indexed score rows) are the parent's, so a step taken through a slice is seen by every other user
    of the storage."""

    def __init__(self, bank: KVBank, begin: int, n_layers: int):
        self.bank, self.begin, self.n_layers = bank, begin, n_layers
        for name in ("n_q_heads", "n_kv_heads", "head_dim", "cap", "device", "dtype"):
            setattr(self, name, getattr(bank, name))

    def _rows(self, t):
        return t[self.begin:self.begin + self.n_layers]

    # (read-only snapshots: the bookkeeping is the shared bank's, advanced by the calls below)
    n_slots = property(lambda self: tuple(self._rows(self.bank.n_slots)))
    extent = property(lambda self: tuple(self._rows(self.bank.extent)))
    slot_of_pos = property(lambda self: self._rows(self.bank.slot_of_pos))
    score_sum = property(lambda self: self._rows(self.bank.score_sum))
    score_sq = property(lambda self: self._rows(self.bank.score_sq))
    score_cnt = property(lambda self: self._rows(self.bank.score_cnt))

    def _span(self, layer_begin, layer_count):
        lc = self.n_layers - layer_begin if layer_count is None else layer_count
        if layer_begin < 0 or lc < 1 or layer_begin + lc > self.n_layers:
            raise ValueError(f"layers [{layer_begin}, {layer_begin + lc}) are outside this {self.n_layers}-layer sequence")
        return self.begin + layer_begin, lc

    def state_init(self, width, mode, stride=1, layer_begin=0, layer_count=None):
        lb, lc = self._span(layer_begin, layer_count)
        self.bank.state_init(width, mode, stride, lb, lc)

    def load_rows(self, k, v, pos_begin=None, layer_begin=0):
        lb, _ = self._span(layer_begin, k.shape[0])
        self.bank.load_rows(k, v, pos_begin, lb)

    def ordered_kv(self, layer_begin=0, layer_count=None):
        return self.bank.ordered_kv(*self._span(layer_begin, layer_count))

    def attend(self, plan, q, k_new, v_new, layer_begin=0, out=None, evict_ids=None, phases=0):
        lb, _ = self._span(layer_begin, q.shape[0])
        return self.bank.attend(plan, q, k_new, v_new, lb, out, evict_ids, phases)


class KVBankBatch:
    """One bank of ``n_seq * n_layers`` layers laid out ``[sequence][layer]`` for the ragged decode batch (include/easykv_hip.h,
    ekv_seq): :meth:`sequence` hands out sequence ``i``'s contiguous ``n_layers`` as an ordinary bank for its prefill, and
    :meth:`attend` serves model layer ``layer`` of any subset of the sequences — each with its own cache length, score offset and
    eviction geometry — in ONE call: one launch per kernel kind over the layers ``{s * n_layers + layer}``."""

    def __init__(self, n_seq, n_layers, n_q_heads, n_kv_heads, head_dim, cap, device="cuda", scored=True, dtype=torch.float16, kv_quant=None, long_rows=False,
                 logit_cap=None, sm_scale=None, sinks=None, windows=None):
        """``sm_scale``: the softmax scale of every sequence (:class:`KVBank`; None: ``1 / sqrt(head_dim)``).  ``logit_cap`` raises: there is
        no capped batch call.  ``sinks`` raises: there is no sink batch call.
        ``kv_quant='fp8'``: the shared bank holds FP8 planes only from the start (the 16-bit rows of ``n_seq`` sequences are never
        allocated); its sequences are filled by :meth:`adopt` from banks quantised by :meth:`KVBank.quantize_fp8`.
        ``kv_quant='mxfp4'``: likewise with MXFP4 planes, filled from banks quantised by :meth:`KVBank.quantize_mxfp4`.
        ``kv_quant='mxfp6'``: likewise with MXFP6 planes (:meth:`KVBank.quantize_mxfp6`).
        ``kv_quant='fp8_mxfp4'``: likewise with FP8 key and MXFP4 value planes (:meth:`KVBank.quantize_fp8_mxfp4`).
        ``kv_quant='k16_mxfp4'``: the 16-bit K rows with MXFP4 value planes (:meth:`KVBank.quantize_k16_mxfp4`); no 16-bit V."""
        if long_rows:
            raise _lib.EkvError("KVBankBatch(long_rows=True): the long-row scorer is built for single sequences, not for decode batches: "
                                "the batched calls have no long form (what a batch leaves to the generic scorer it refuses)")
        if logit_cap is not None:
            raise _lib.EkvError("KVBankBatch(logit_cap=...): soft-capped logits are built for single sequences, not for decode batches: "
                                "there is no capped batch call")
        if sinks is not None:
            raise _lib.EkvError("KVBankBatch(sinks=...): attention sinks are built for single sequences, not for decode batches: "
                                "there is no sink batch call")
        if windows is not None:
            raise _lib.EkvError("KVBankBatch(windows=...): sliding windows are built for single sequences, not for decode batches: "
                                "there is no window batch call")
        if not 1 <= n_seq <= _lib.MAX_SEQS:
            raise ValueError(f"a decode batch holds 1..{_lib.MAX_SEQS} sequences, not {n_seq}")
        self.n_seq, self.n_layers = n_seq, n_layers
        self.bank = KVBank(n_seq * n_layers, n_q_heads, n_kv_heads, head_dim, cap, device, scored, dtype, kv_quant, sm_scale=sm_scale)
        self.lib, self.dtype = self.bank.lib, dtype
        self.n_q_heads, self.n_kv_heads, self.head_dim, self.cap, self.device = n_q_heads, n_kv_heads, head_dim, self.bank.cap, self.bank.device
        self.n_calls = 0      # batched attend calls issued (one per layer and decode forward)

    def sequence(self, i) -> _BankSlice:
        if not 0 <= i < self.n_seq:
            raise ValueError(f"sequence {i} of a batch of {self.n_seq}")
        return _BankSlice(self.bank, i * self.n_layers, self.n_layers)

    def n_slots(self, i, layer=0):
        return self.bank.n_slots[i * self.n_layers + layer]

    kv_quant = property(lambda self: self.bank.kv_quant)

    def quantize(self, kind):
        """:meth:`KVBank.quantize` of the shared bank: the rows ``[0, max extent)`` of every layer become codes + scales / exponents at
        their physical indices (slot maps, score rows, lengths and extents of every sequence carry over), the 16-bit tensors are
        released and :meth:`attend` / :meth:`step_info` go to that format's batch calls.  ``sequence(i)`` then behaves as a quantised
        :class:`KVBank`: decode steps only."""
        self.bank.quantize(kind)
        return self

    def quantize_fp8(self):
        """:meth:`quantize` to FP8 rows (:meth:`KVBank.quantize_fp8`)."""
        self.bank.quantize_fp8()
        return self

    def quantize_mxfp4(self):
        """:meth:`quantize` to MXFP4 rows (:meth:`KVBank.quantize_mxfp4`: head_dim 128, GQA factors up to 4)."""
        return self.quantize("mxfp4")

    def quantize_mxfp6(self):
        """:meth:`quantize` to MXFP6 rows (:meth:`KVBank.quantize_mxfp6`: head_dim 128, GQA factors up to 4)."""
        return self.quantize("mxfp6")

    def quantize_fp8_mxfp4(self):
        """:meth:`quantize` to FP8 keys with MXFP4 values (:meth:`KVBank.quantize_fp8_mxfp4`: head_dim 128)."""
        return self.quantize("fp8_mxfp4")

    def quantize_k16_mxfp4(self):
        """:meth:`quantize` to 16-bit keys with MXFP4 values (:meth:`KVBank.quantize_k16_mxfp4`: head_dim 128)."""
        return self.quantize("k16_mxfp4")

    def _quant_call(self, what):
        """(the batched call `what` of this bank's row format, its leading descriptor arguments), as the bank resolved them."""
        return self.bank._calls[True, what], self.bank._desc_ref

    def kv_bytes(self) -> int:
        """Bytes held for the K/V rows of all sequences (:meth:`KVBank.kv_bytes` of the shared bank)."""
        return self.bank.kv_bytes()

    def adopt(self, i, src: KVBank):
        """Sequence ``i`` takes over the state of ``src``, a bank of this batch's layer count and head shape that one sequence was
        prefilled on alone: K/V rows at their physical indices, slot maps, score rows (ordered layout), lengths and extents.  The
        rows behind ``src.cap`` keep this bank's own free list, so a shorter ``src.cap`` is fine.  A quantised batch takes a quantised
        source of the same kind (codes and row scales / block exponents are copied as they are); 16-bit, FP8, MXFP4, MXFP6, FP8-key / MXFP4-value
        and 16-bit-key / MXFP4-value rows do not mix (the last: ``k``, ``v4`` and ``v_exp`` are copied)."""
        b = self.bank
        if (src.n_layers, src.n_q_heads, src.n_kv_heads, src.head_dim, src.dtype) != (self.n_layers, b.n_q_heads, b.n_kv_heads, b.head_dim, b.dtype) \
                or src.cap > b.cap or not 0 <= i < self.n_seq:
            raise ValueError("adopt(): the source bank must have this batch's layers, heads, head_dim and dtype, and cap <= the batch's")
        if src.kv_quant != b.kv_quant:
            raise ValueError(f"adopt(): the source bank's rows (kv_quant={src.kv_quant!r}) are not this batch's (kv_quant={b.kv_quant!r}): "
                             "quantize_fp8() both or neither, or quantize_mxfp4() both")
        src.join()
        l0, l1, c = i * self.n_layers, (i + 1) * self.n_layers, src.cap
        b._ensure_ordered(l0, self.n_layers)
        rows = ("k", "v") if b._fmt is None else tuple(b._fmt.get("keeps", ())) + tuple(name for name, *_ in b._fmt["planes"])
        for name in rows + ("slot_of_pos", "score_sum", "score_sq", "score_cnt"):      # (the properties hand out the ordered layout)
            t = getattr(src, name)
            if t is not None:
                getattr(b, name)[l0:l1, :, :c].copy_(t)
        b.n_slots[l0:l1] = src.n_slots
        b.extent[l0:l1] = src.extent

    def make_table(self, plans, layer, active=None, n_split=0):
        """(shared ekv_step, ekv_seq table) of the batched call for model layer ``layer`` over the sequences ``active`` (default:
        all), one :class:`StepPlan` each: every entry by the arithmetic :meth:`KVBank.make_step` applies to that sequence alone."""
        b = self.bank
        seqs = list(range(self.n_seq)) if active is None else list(active)
        if len(seqs) != len(plans) or not seqs:
            raise ValueError(f"{len(plans)} plans for {len(seqs)} sequences")
        if not 0 <= layer < self.n_layers or any(not 0 <= s < self.n_seq for s in seqs):
            raise ValueError("layer or sequence index outside the batch")
        tb = (_lib.Seq * len(seqs))()
        shared = None
        for e, s, plan in zip(tb, seqs, plans):
            if plan.phase != "decode" or plan.streaming:
                raise ValueError("a batched step is a decode step with plain keys")
            l = s * self.n_layers + layer
            st = b.make_step(plan, 1, l, 1)
            e.layer, e.n_slots, e.score_off, e.n_evict, e.phys_extent = l, st.n_slots, st.score_off, st.n_evict, st.phys_extent
            e.win_lo, e.win_tail, e.roco_k1, e.range_start = st.win_lo, st.win_tail, st.roco_k1, st.range_start
            if shared is None:
                shared = st
            elif (st.policy, st.accumulate, st.tova_head_mean) != (shared.policy, shared.accumulate, shared.tova_head_mean):
                raise ValueError("the sequences of a batched step share the policy and whether scores accumulate")
            if st.n_evict:      # (read only by entries that evict: the reference adds the count inside its eviction branch)
                shared.count_add, shared.count_tail_step = st.count_add, st.count_tail_step
        shared.n_split = n_split
        return shared, tb, seqs

    def step_info(self, plans, layer, active=None, n_split=0) -> dict:
        st, tb, _ = self.make_table(plans, layer, active, n_split)
        info = (C.c_int32 * 10)()
        b = self.bank
        fn, desc = self._quant_call("step_info")      # (FP8 / MXFP4 / MXFP6 rows: the kv8 / kv4 / kv6 batch call, the descriptor behind the dtype)
        check(fn(C.byref(b._bank), C.byref(st), b._dt, *desc, tb, len(tb), info, 10), fn.__name__)
        keys = ("n_split", "fused", "two_pass", "wide", "n_qblocks", "qb_rows", "n_col_parts", "fold_in_kernel", "n_launches", "fused_order")
        return dict(zip(keys, (int(x) for x in info)))

    def workspace_bytes(self, st, tb) -> int:
        """Workspace of the batched call of (shared step, table) as :meth:`make_table` returns them."""
        b = self.bank
        fn, desc = self._quant_call("workspace_bytes")
        return fn(C.byref(b._bank), C.byref(st), b._dt, *desc, tb, len(tb))

    def attend(self, plans, q, k_new, v_new, layer, active=None, out=None, evict_ids=None, n_split=0):
        """q / out ``[B', Hq, 1, D]``, k_new / v_new ``[B', H, 1, D]``: row i belongs to ``active[i]`` (default: every sequence).
        Returns (out, evict_ids ``[B', H, 1]`` int32 or None when no sequence evicts; rows of sequences that keep everything are
        left as they are)."""
        b = self.bank
        st, tb, seqs = self.make_table(plans, layer, active, n_split)
        n = len(seqs)
        if q.shape[0] != n or q.shape[2] != 1:
            raise ValueError(f"q must be [{n}, Hq, 1, D] for {n} sequences, not {tuple(q.shape)}")
        for e in tb:
            if b._slot_rows[e.layer]:
                b._ensure_ordered(e.layer, 1)
        if any(b._score_done[e.layer] is not None for e in tb):
            b.join()
        if out is None:
            out = torch.empty(n, self.n_q_heads, 1, self.head_dim, dtype=self.dtype, device=self.device)
        q, k_new, v_new = _stride_rows(st, q, k_new, v_new, out, self.dtype)
        k_max = max(e.n_evict for e in tb)
        if k_max > 0 and evict_ids is None:
            evict_ids = torch.empty(n, self.n_kv_heads, k_max, dtype=torch.int32, device=self.device)
        bank_ref, st_ref = C.byref(b._bank), C.byref(st)
        ws = b._workspace(self.workspace_bytes(st, tb))
        tensors = (_ptr(q), _ptr(k_new), _ptr(v_new), _ptr(out), _ptr(evict_ids) if k_max > 0 else None, _ptr(ws), ws.numel(), b._stream())
        fn, desc = self._quant_call("step_attend")
        check(fn(bank_ref, st_ref, b._dt, *desc, tb, n, *tensors), fn.__name__)
        for e in tb:
            b.n_slots[e.layer] = e.n_slots - e.n_evict
            b.extent[e.layer] = e.phys_extent
        self.n_calls += 1
        return out, (evict_ids if k_max > 0 else None)
