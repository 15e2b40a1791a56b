"""Host-side mirror of the reference's public surface for the budgeted-KV path.

    from easykv_amd import enable_fixed_kv
    enable_fixed_kv(model, tokenizer, mode='auto', stride=8)
    text = model.easykv_generate(input_ids=ids, generation_config=dict(budget=2048, kv_policy='roco'))

Same names, argument meaning, generation_config keys/defaults, kv_policy strings, return types and
printed lines as the reference (easykv/easykv.py:199-210, :903-908).  What differs is WHERE the work
happens: the reference asks the model for every layer's probability matrix and scores / selects /
compacts in Python (easykv/easykv.py:264-362); here the driver only decides the per-forward
:class:`StepPlan` and every layer's attention call runs the fused HIP step on a device-resident
:class:`KVBank` — no attention map, no host sync, no K/V copy per step.

Model contract (what ``self`` must provide; the reference's is SURVEY.md §8b):
  * ``self.config.{num_hidden_layers, num_attention_heads[, num_key_value_heads][, head_dim | hidden_size]}``,
    ``self.device`` (a GPU), ``self.tokenizer.{eos_token_id, decode}``;
  * ``self(input_ids=, past_key_values=<BudgetedKVCache>, position_ids=, use_cache=True)`` returning an object
    with ``.logits [1, n, V]``; inside, every attention layer calls
    ``past_key_values.attend(layer_idx, q [1,Hq,n,D], k [1,H,n,D], v [1,H,n,D]) -> [1,Hq,n,D]`` with keys already
    rotated by their TRUE positions (un-rotated when ``generation_config['streaming']``: the kernel then rotates at
    read time by slot index, easykv/llama_patch.py:310-327).
  ``easykv_amd.hf`` adapts HF transformers >= 5 Llama/Mistral models to this contract.

Shape of the driver: ``generate`` = :class:`_Run` (generation_config read once, with every refusal) -> :func:`_prefill` (one prompt up
to the decode phase, as a :class:`Prefilled`) -> :func:`_decode` (one loop; each step's plan from the sequence's
:class:`DecodePlanner`) -> :func:`_print_budget_line`.  ``generate_batch`` runs the same ``_Run`` and ``_prefill`` per prompt and steps one
``DecodePlanner`` per sequence.  All of it runs without a GPU over stub caches: tests/test_driver_cpu.py.
"""
from __future__ import annotations

import contextlib
import contextvars
import dataclasses
import functools
import math
import statistics
import time
from typing import List, Optional

import torch

from . import _lib
from .engine import CAPPED_HEAD_DIMS, PLAIN_KEYS_HEAD_DIMS, SINK_HEAD_DIMS, WINDOW_HEAD_DIM, KVBank, KVBankBatch, StepPlan, row_format

KNOWN_POLICIES = ("roco", "h2o_head", "tova", "recency", "random", "full")
SCORED = ("roco", "h2o_head", "tova")
PREFIX_BLOCK = 64   # queries per launch when the prefix must be scored (keep_attention)


# ------------------------------------------------------------------------------------------------
# budget geometry (easykv/easykv.py:385-392, :544-552, :773-780)
# ------------------------------------------------------------------------------------------------
def _idx_for(length: int, budget_p: int, stride: int) -> int:
    return next(i for i in range(budget_p, -1, -1) if (length - i) % stride == 0)


def geometry(mode: str, length: int, budget, stride: int):
    """-> (budget', idx, r_idx).  ``idx`` = retained slots after the strided prefill, ``r_idx`` = dense prefix."""
    if isinstance(budget, float):
        budget_p = int(length * budget) + stride
    else:
        budget_p = budget + stride
        if mode == "auto" and budget_p >= length:
            budget_p -= stride
    idx = _idx_for(length, budget_p, stride)
    if mode == "encoding":      # largest r_idx < idx on the stride grid (:391-392)
        r_idx = next((r for r in range(idx - 1, -1, -1) if (idx - r) % stride == 0), None)
    else:                       # auto / ppl: smallest r_idx >= 1 (:551-552, :779-780)
        r_idx = next((r for r in range(1, idx) if (idx - r) % stride == 0), None)
    return budget_p, idx, r_idx


# ------------------------------------------------------------------------------------------------
# the cache object handed to the model
# ------------------------------------------------------------------------------------------------
# The cache of the model forward in flight, for attention seams that are not handed ``past_key_values`` (easykv_amd.hf's
# AttentionInterface function).  A context variable, set around every forward by :func:`generate` and reset afterwards: two
# models, nested or interleaved generates and threads cannot see each other's cache, and a forward outside easykv_generate()
# finds nothing (the seam then raises instead of appending into a stale bank).
_ACTIVE: contextvars.ContextVar = contextvars.ContextVar("easykv_amd_active_cache", default=None)


def active_cache():
    """The :class:`BudgetedKVCache` of the forward in flight in this context, or None."""
    return _ACTIVE.get()


class BudgetedKVCache:
    """Device-resident budgeted cache of one sequence.  The driver sets :attr:`plan` before each model
    forward; every attention layer then calls :meth:`attend`.  It also duck-types the two ``Cache`` methods HF
    transformers >= 5 calls on ``past_key_values`` (``update`` hands the new rows straight back: the bank appends them
    inside :meth:`attend`).

    ``layer_begin`` / ``layer_count``: the contiguous block of the model's layers THIS process owns (layer sharding,
    SURVEY.md §8e: the reference spreads layers over GPUs with ``device_map='auto'``, test_passkey.py:25-35; here one process
    per GPU owns a block, easykv_amd/dist.py).  The bank holds only those layers; :meth:`attend` takes GLOBAL layer indices.

    ``dtype``: element type of the K/V bank, torch.float16 (None = the default) or torch.bfloat16; q / k / v of another dtype are
    converted to it and the attention output comes back in it.  A bf16 bank has no RoPE-on-read build (``streaming``).

    ``sm_scale``: the softmax scale (None: ``1 / sqrt(head_dim)``); ``logit_cap``: attention-logit soft-capping (None: off).  Both are
    the bank's (:class:`~easykv_amd.engine.KVBank`) and are kept as attributes: the HF seam holds the attention module's own
    ``scaling`` / ``softcap`` against them.

    ``sinks``: learned attention sinks ``[n_layers, n_q_heads]`` of the layers this cache owns (None: off; gpt-oss), the bank's likewise
    and kept as an attribute (fp32, on the device): the seam holds the module's ``s_aux`` against the row of its layer."""

    def __init__(self, n_layers, n_q_heads, n_kv_heads, head_dim, cap, device, streaming=False, rope=None,
                 record=False, layer_begin=0, layer_count=None, rope_base=10000.0, dtype=None, long_rows=False, logit_cap=None, sm_scale=None,
                 sinks=None, windows=None):
        self.layer_begin = layer_begin
        self.layer_count = n_layers - layer_begin if layer_count is None else layer_count
        if not (0 <= self.layer_begin and self.layer_count >= 1 and self.layer_begin + self.layer_count <= n_layers):
            raise ValueError(f"layer block [{layer_begin}, {layer_begin}+{layer_count}) outside the model's {n_layers} layers")
        self.n_model_layers = n_layers
        dtype = torch.float16 if dtype is None else dtype
        if dtype is torch.bfloat16 and streaming:
            raise ValueError("a bf16 K/V bank has no RoPE-on-read build: streaming=True needs kv_dtype='float16'")
        # long_rows: the bank's steps go to the long-row call family (KVBank(long_rows=True): score rows of any width up to cap)
        if logit_cap is not None and streaming:
            raise ValueError("a soft-capped cache (logit_cap) has no RoPE-on-read build: streaming=True needs logit_cap=None")
        if sinks is not None and streaming:
            raise ValueError("a cache with attention sinks has no RoPE-on-read build: streaming=True needs sinks=None")
        self.logit_cap, self.sm_scale = logit_cap, sm_scale
        if windows is not None and streaming:
            raise ValueError("a cache with sliding windows has no RoPE-on-read build: streaming=True needs windows=None")
        extra = {k: v for k, v in (("logit_cap", logit_cap), ("sm_scale", sm_scale), ("sinks", sinks), ("windows", windows)) if v is not None}      # (opt-in: named only when set)
        self.bank = KVBank(self.layer_count, n_q_heads, n_kv_heads, head_dim, cap, device=device, dtype=dtype, long_rows=long_rows, **extra)
        self.sinks = self.bank.sinks      # (fp32 on the device, or None)
        self.windows = self.bank.windows      # (the windows of the layers this cache owns, a tuple, or None)
        self._windows_checked = set()      # layers whose module's sliding_window the seam has held against it (hf._easykv_attention)
        self._sinks_checked = set()       # layers whose module's s_aux the seam has held against the row (hf._easykv_attention)
        # no resident rows behind a model: its weights (gigabytes) stream through the Infinity Cache between two attention launches
        # of a layer, and plain loads that miss cost more than non-temporal ones ("resident rows": the harm run)
        self.bank.resident_bytes = 0
        self.plan = StepPlan(policy="full", phase="prefill", accumulate=False)
        self.streaming = streaming
        self.positions = None    # true position ids of the forward in flight (set by the driver)
        self.unrotate = None     # HF seam + streaming: (cos, sin) fp32 [>= max position, D] to take the model's RoPE off q/k
        if streaming:
            cos, sin = rope[:2] if rope is not None else rope_tables(cap, head_dim, rope_base)
            self.bank.set_rope(cos, sin)
        self.record = record
        self.evictions = []      # record=True: per forward with eviction: list over OWNED layers of int32 [H,k] (device)
        self._cur = None
        self.score_prefix = False
        self.n_attend = 0        # attend() calls of the forward in flight (checked by the driver after every forward)
        self._defer_this_forward = None
        self.defer_chunk_scorer = True     # scored chunk steps of a layer-per-call model: one scorer launch per forward (round 4)
        self.head_decode = None            # 'deferred': decode layers over heads of different lengths go through attend(defer=True) + one flush (generation_config['head_decode'])

    @property
    def kv_quant(self):
        """None, "fp8" once the bank's K/V rows are FP8 codes with per-row scales (KVBank.quantize_fp8), or "mxfp4" once they are
        MXFP4 codes with block exponents (KVBank.quantize_mxfp4), or "mxfp6" (MXFP6 codes, KVBank.quantize_mxfp6), or "fp8_mxfp4"
        (FP8 keys with MXFP4 values, KVBank.quantize_fp8_mxfp4), or "k16_mxfp4" (the 16-bit keys with MXFP4 values,
        KVBank.quantize_k16_mxfp4)."""
        return self.bank.kv_quant

    def kv_bytes(self) -> int:
        """Bytes the bank holds for K/V rows."""
        return self.bank.kv_bytes()

    def owns(self, layer_idx: int) -> bool:
        return self.layer_begin <= layer_idx < self.layer_begin + self.layer_count

    def get_seq_length(self, layer_idx: Optional[int] = None) -> int:
        """Live slots (every owned layer holds the same number, as in the reference).  After adaptive head budgets: the mean over the
        layer's heads, which is the uniform run's number (the heads' evictions sum to H * n_evict)."""
        l = 0 if layer_idx is None or not self.owns(layer_idx) else layer_idx - self.layer_begin
        heads = self.bank.head_slots[l] if self.bank.head_slots is not None else None
        return self.bank.n_slots[l] if heads is None else sum(heads) // len(heads)

    def update(self, key_states, value_states, layer_idx, cache_kwargs=None):
        return key_states, value_states

    def begin_forward(self, plan: StepPlan, positions=None):
        self.bank.abort_step()     # a previous forward that raised between two layers leaves a half-open deferred token step
        self.plan = plan
        self.positions = positions
        self.n_attend = 0
        self._defer_this_forward = None      # decided by the forward's first attend() (all owned layers still hold the same length)
        self._cur = [] if (self.record and plan.evict) else None
        if self._cur is not None:
            self.evictions.append(self._cur)

    @contextlib.contextmanager
    def active(self, plan: StepPlan, positions=None):
        """Scope of ONE model forward driven by hand (generate() does this around every forward it issues): sets the plan
        and makes this cache the one attention seams without a ``past_key_values`` argument (easykv_amd.hf) find."""
        self.begin_forward(plan, positions)
        tok = _ACTIVE.set(self)
        try:
            yield self
        finally:
            _ACTIVE.reset(tok)

    def _prefix_in_one_step(self, plan, n, layer_idx) -> bool:
        key = (plan.policy, plan.accumulate, plan.two_pass, type(self.bank).default_two_pass, self.streaming, n)
        if getattr(self, "_prefix_rule", (None, None))[0] != key:
            info = self.bank.step_info(plan, n, layer_idx, 1)
            self._prefix_rule = (key, bool(info["two_pass"] and info["wide"]))
        return self._prefix_rule[1]

    DEFER_WORKSPACE_LIMIT = 1 << 30      # bytes of logits / column sums of all layers a deferred chunk step may keep alive ...
    DEFER_WORKSPACE_FRACTION = 1 / 8     # ... and never more than this share of the device memory that is free when the rule is made

    def _defer_fits(self, plan, n) -> bool:
        """Does this scored chunk step run with the scorers of all owned layers deferred to one launch per forward?  Not when the
        immediate form is ONE launch already (the logits-in-LDS kernel, a chunk step with the scorer as its kernel tail — ekv_step_info
        ``fused``: deferral would take the step off that kernel, whose arithmetic and speed differ), and not when every layer's logits /
        column sums kept until the flush would pin too much HBM (one-pass shapes of long caches)."""
        key = (plan.policy, plan.accumulate, plan.evict, plan.two_pass, type(self.bank).default_two_pass, self.streaming, n, self.bank.n_slots[0])
        if getattr(self, "_defer_rule", (None, None))[0] != key:
            one_launch = bool(self.bank.step_info(plan, n, 0, 1)["fused"])
            limit = min(self.DEFER_WORKSPACE_LIMIT, int(torch.cuda.mem_get_info(self.bank.device)[0] * self.DEFER_WORKSPACE_FRACTION))
            self._defer_rule = (key, (not one_launch) and self.bank.deferred_workspace_bytes(plan, n) <= limit)
        return self._defer_rule[1]

    def attend(self, layer_idx: int, q, k, v):
        """One layer of one forward: append + attention + score + select + compaction, all on device.
        ``layer_idx`` is the layer's index in the MODEL; it must lie in this cache's block."""
        if not self.owns(layer_idx):
            raise ValueError(f"layer {layer_idx} is not in this rank's block [{self.layer_begin}, {self.layer_begin + self.layer_count})")
        if q.shape[0] != 1 or k.shape[0] != 1 or v.shape[0] != 1:
            raise ValueError("the budgeted-KV path is batch-size 1 (as the reference: easykv/easykv.py asserts nothing but indexes [0])")
        layer_idx -= self.layer_begin
        self.n_attend += 1
        plan = self.plan
        n = q.shape[2]
        # rows of the bank's dtype are read IN PLACE at their strides (ABI 8): HF hands over [1, H, n, D] transposed views of the
        # projections' [1, n, H * D] output — three copy kernels per layer in front of every chunk step until round 5.  Other dtypes are
        # converted; layouts the kernels cannot address are copied dense by KVBank.attend.
        dt = self.bank.dtype
        q, k, v = (t if t.dtype == dt else t.to(dt) for t in (q, k, v))
        # the output is written token-major ([1, n, Hq, D]) and returned as its [1, Hq, n, D] view: the transpose(1, 2) every caller
        # applies next (easykv_amd.hf, llama_patch.py:230-232) is then a dense tensor, no copy in front of o_proj
        out = torch.empty(1, n, q.shape[1], q.shape[3], dtype=dt, device=q.device).transpose(1, 2) if n > 1 else None
        if self.score_prefix and n > PREFIX_BLOCK and not self._prefix_in_one_step(plan, n, layer_idx):
            # keep_attention: the dense prefix must also feed the score rows (easykv/easykv.py:173-186).  ONE launch pair per layer
            # when the LIBRARY says the step runs as the two-pass scheme on the wide-block kernel (ekv_step_info: the query blocks
            # are walked inside the launch and nothing of size r x r exists anywhere); every other dispatch (RoPE-on-read,
            # head_dim 32, odd GQA factors, EKV_NO_WIDE, a forced one-pass scheme) exports logits or one column-sum row per query
            # block to a workspace, so there the prefix is cut into query blocks here
            outs = []
            for i0 in range(0, n, PREFIX_BLOCK):
                self.bank.attend(plan, q[:, :, i0:i0 + PREFIX_BLOCK], k[:, :, i0:i0 + PREFIX_BLOCK], v[:, :, i0:i0 + PREFIX_BLOCK],
                                 layer_begin=layer_idx, out=out[:, :, i0:i0 + PREFIX_BLOCK])
            return out
        if self._defer_this_forward is None:      # one decision per forward: an immediate step advances its layer's length at once
            self._defer_this_forward = bool(n > 1 and plan.phase == "prefill" and plan.policy in ("roco", "h2o_head", "tova") and (plan.accumulate or plan.evict)
                                            and self.defer_chunk_scorer and self._defer_fits(plan, n))
        deferable_chunk = self._defer_this_forward
        if n == 1 and plan.phase == "decode" and self.head_decode == "deferred" and self.bank.head_slots is not None:
            # heads of different lengths, deferred (generation_config['head_decode'] = 'deferred'): exactly like a uniform bank below —
            # attention + fold of this layer now through the heads family (ekv_heads_*), ONE scorer launch over all owned layers and
            # heads after the last one
            out, _ = self.bank.attend(plan, q, k, v, layer_begin=layer_idx, defer=True, out=out)
            if self.n_attend == self.layer_count:
                ids = self.bank.flush()
                if self._cur is not None and ids is not None:
                    self._cur.extend(ids[l] for l in range(self.layer_count))
            return out
        if n == 1 and plan.phase == "decode" and self.bank.ragged(layer_idx):
            # heads of different lengths (adaptive head budgets): the layer's step is the batched call on the one-head view, whole
            # (head_decode = 'view', the default)
            out, ids = self.bank.attend(plan, q, k, v, layer_begin=layer_idx, evict_ids=None if self._cur is not None else False)
            if self._cur is not None and ids is not None:
                self._cur.append(ids[0])
            return out
        if ((n == 1 and plan.phase == "decode") or deferable_chunk) and self.layer_count > 1:
            # one layer per call (a decoder stack): attention + fold of this layer now, the scorers of all owned layers in ONE
            # launch after the last layer (KVBank.flush) — off the critical path of the stack.  Decode steps, and since round 4 the
            # scored chunk steps of a strided prefill (their scorer launch — 32 workgroups, latency-bound, folds the key-range
            # partials too — was more than half of a layer's time)
            out, _ = self.bank.attend(plan, q, k, v, layer_begin=layer_idx, defer=True, out=out)
            if self.n_attend == self.layer_count:
                ids = self.bank.flush()
                if self._cur is not None and ids is not None:
                    self._cur.extend(ids[l] for l in range(self.layer_count))
            return out
        # (the evicted cache indices are only wanted when a caller records them: _record_evictions)
        out, ids = self.bank.attend(plan, q, k, v, layer_begin=layer_idx, evict_ids=None if self._cur is not None else False, out=out)
        if self._cur is not None and ids is not None:
            self._cur.append(ids[0])
        return out


class BudgetedKVCacheBatch:
    """What the attention seam sees during the decode phase of :func:`generate_batch`: the caches of the live sequences of one
    :class:`KVBankBatch`.  The driver sets one :class:`StepPlan` per live sequence before each forward; every attention layer then
    calls :meth:`attend` ONCE with ``[B', Hq, 1, D]`` queries — row i belongs to ``live[i]`` — which is one batched step of the
    library (one launch per kernel kind) for that layer."""

    streaming, unrotate = False, None      # (a batch has no RoPE-on-read form)
    logit_cap = None                        # (... and no soft-capped one; the softmax scale is the shared bank's)
    sinks = None                            # (... and no sink one)
    windows = None                          # (... and no window one)

    def __init__(self, bat: KVBankBatch, record=False):
        self.bat = bat
        self.sm_scale = bat.bank.sm_scale
        self.plans, self.live, self.positions = [], [], None
        self.record = record
        self.evictions = [[] for _ in range(bat.n_seq)]      # record=True, per sequence: per evicting forward, per layer, int32 [H, 1]
        self._cur = {}
        self.n_attend = 0

    def get_seq_length(self, layer_idx: Optional[int] = None) -> int:
        return max((self.bat.n_slots(s) for s in self.live), default=0)

    def update(self, key_states, value_states, layer_idx, cache_kwargs=None):
        return key_states, value_states

    @contextlib.contextmanager
    def active(self, plans, live, positions=None):
        """Scope of ONE batched decode forward over the sequences ``live`` (one plan each)."""
        self.plans, self.live, self.positions, self.n_attend = list(plans), list(live), positions, 0
        self._cur = {}
        if self.record:
            for s, plan in zip(self.live, self.plans):
                if plan.evict:
                    self._cur[s] = []
                    self.evictions[s].append(self._cur[s])
        tok = _ACTIVE.set(self)
        try:
            yield self
        finally:
            _ACTIVE.reset(tok)

    def attend(self, layer_idx: int, q, k, v):
        n = len(self.live)
        if q.shape[0] != n or k.shape[0] != n or v.shape[0] != n or q.shape[2] != 1:
            raise ValueError(f"a batched decode forward hands over [{n}, heads, 1, head_dim] rows for its {n} live sequences; got q {tuple(q.shape)}")
        self.n_attend += 1
        dt = self.bat.dtype
        q, k, v = (t if t.dtype == dt else t.to(dt) for t in (q, k, v))
        out, ids = self.bat.attend(self.plans, q, k, v, layer_idx, active=self.live)
        for row, s in enumerate(self.live):
            if s in self._cur:
                self._cur[s].append(ids[row])
        return out


def rope_tables(seq_len: int, dim: int, base: float = 10000.0):
    """fp32 cos/sin ``[seq_len, dim]`` with the HF layout ``cat(freqs, freqs)``."""
    inv_freq = 1.0 / (base ** (torch.arange(0, dim, 2, dtype=torch.float32) / dim))
    freqs = torch.outer(torch.arange(seq_len, dtype=torch.float32), inv_freq)
    emb = torch.cat((freqs, freqs), dim=-1)
    return emb.cos(), emb.sin()


# ------------------------------------------------------------------------------------------------
# sampler (easykv/easykv.py:115-134) — vocab-sized torch ops, not part of the KV path
# ------------------------------------------------------------------------------------------------
def logits_adapter(logits: torch.Tensor, temperature: float, top_p: float):
    prob = torch.softmax(logits / temperature, dim=-1)
    sorted_prob, order = torch.sort(prob, descending=True, dim=-1)
    keep = (torch.cumsum(sorted_prob, dim=-1) - sorted_prob) <= top_p
    sorted_prob = sorted_prob * keep
    sorted_prob = sorted_prob / sorted_prob.sum(dim=-1, keepdim=True)
    final = torch.zeros_like(prob).scatter(-1, order, sorted_prob)
    return final, torch.softmax(logits, dim=-1)


def _dims(self):
    cfg = self.config
    n_layers = cfg.num_hidden_layers
    hq = cfg.num_attention_heads
    h = getattr(cfg, "num_key_value_heads", None) or hq
    d = getattr(cfg, "head_dim", None) or (cfg.hidden_size // hq)
    return n_layers, hq, h, d


def _collect_sinks(model, cfg, n_layers, hq):
    """The attention sinks of a model as one fp32 tensor ``[n_layers, n_q_heads]``, or None for a model without them.  Either
    ``generation_config['attention_sinks']`` (anything ``torch.as_tensor`` takes, of that shape), or — what a stock gpt-oss has — every
    module of the model that carries a ``sinks`` tensor of ``num_attention_heads`` elements and an integer ``layer_idx``: each layer must
    then have exactly one."""
    given = cfg.get("attention_sinks", None)
    if given is not None:
        t = torch.as_tensor(given).detach().float().cpu()
        if tuple(t.shape) != (n_layers, hq):
            raise ValueError(f"generation_config['attention_sinks'] must have shape [num_hidden_layers, num_attention_heads] = "
                             f"[{n_layers}, {hq}], not {tuple(t.shape)}")
        return t
    modules = getattr(model, "modules", None)
    rows = {}
    for m in (modules() if callable(modules) else ()):
        s, li = getattr(m, "sinks", None), getattr(m, "layer_idx", None)
        if torch.is_tensor(s) and s.numel() == hq and isinstance(li, int) and not isinstance(li, bool):
            if li in rows or not 0 <= li < n_layers:
                raise ValueError(f"attention sinks: layer_idx {li} occurs twice among the model's modules or lies outside its {n_layers} layers")
            rows[li] = s.detach().float().reshape(hq).cpu()
    if not rows:
        return None
    if len(rows) != n_layers:
        raise ValueError(f"attention sinks: {len(rows)} of the model's {n_layers} layers carry a `sinks` parameter; all or none must")
    return torch.stack([rows[i] for i in range(n_layers)])


def _collect_windows(model, cfg, n_layers):
    """generation_config['sliding_window'] -> the per-layer windows as a list of ``n_layers`` ints, or None (absent / None: today's
    behaviour, the window is ignored).  ``'model'``: ``config.sliding_window`` on the layers whose ``config.layer_types`` entry is
    ``'sliding_attention'`` (every layer when the config has no ``layer_types``), 0 elsewhere.  Or an explicit list of ``n_layers``
    integers >= 0."""
    given = cfg.get("sliding_window", None)
    if given is None:
        return None
    if isinstance(given, str):
        if given != "model":
            raise ValueError(f"generation_config['sliding_window'] must be None, 'model' or a list of {n_layers} integers, not {given!r}")
        w = getattr(model.config, "sliding_window", None)
        if not (isinstance(w, int) and not isinstance(w, bool) and w > 0):
            raise ValueError(f"generation_config['sliding_window'] = 'model': the model's config.sliding_window is {w!r}")
        types = getattr(model.config, "layer_types", None)
        if types is None:
            return [w] * n_layers
        if len(types) != n_layers:
            raise ValueError(f"generation_config['sliding_window'] = 'model': config.layer_types has {len(types)} entries for {n_layers} layers")
        return [w if t == "sliding_attention" else 0 for t in types]
    try:
        wl = given.tolist() if torch.is_tensor(given) else list(given)
    except TypeError:
        wl = None
    if not (isinstance(wl, list) and len(wl) == n_layers and all(isinstance(x, int) and not isinstance(x, bool) and x >= 0 for x in wl)):
        raise ValueError(f"generation_config['sliding_window'] must be None, 'model' or a list of {n_layers} integers >= 0, not {given!r}")
    return wl


def _kv_dtype(model, key):
    """generation_config['kv_dtype'] -> torch dtype of the K/V bank."""
    if key == "float16":
        return torch.float16
    if key == "bfloat16":
        return torch.bfloat16
    if key == "auto":
        params = getattr(model, "parameters", None)
        p = next(iter(params()), None) if callable(params) else None
        return torch.bfloat16 if p is not None and p.dtype == torch.bfloat16 else torch.float16
    raise ValueError(f"generation_config['kv_dtype'] must be 'float16', 'bfloat16' or 'auto', not {key!r}")


# ------------------------------------------------------------------------------------------------
# the driver: what one call fixes (_Run), the token log, the captured forward, the per-token decode rule
# ------------------------------------------------------------------------------------------------
def _dist():
    """easykv_amd.dist, imported on first use: only a layer-sharded run pays for torch.distributed."""
    from . import dist
    return dist


class _Run:
    """What one call of :func:`generate` / :func:`generate_batch` fixes for all of its forwards.  ``generation_config`` is read HERE and
    nowhere else: the reference's keys and defaults (easykv/easykv.py:199-210), the extension keys, and every refusal."""

    def __init__(self, model, cfg, kv_mode, stride, prompts):
        self.model, self.cfg, self.stride = model, cfg, stride
        self.temperature, self.top_p = cfg.get("temperature", 1.0), cfg.get("top_p", 1.0)
        self.max_new_tokens, self.budget = cfg.get("max_new_tokens", 1024), cfg.get("budget", 0.5)
        self.policy = policy = cfg.get("kv_policy", "recency")
        self.sink, self.recent_ratio = cfg.get("temp_length", 4), cfg.get("recent_ratio", 0.1)
        self.keep_attention = cfg.get("keep_attention", False)
        self.eos_token_ids = cfg.get("eos_token_ids", [model.tokenizer.eos_token_id])
        self.streaming = streaming = cfg.get("streaming", False)
        self.record = cfg.get("_record_evictions", False)      # test hook: keep the evicted ids of every forward
        # extension key: capture the steady-state forwards — the evicting decode step and, round 6, the evicting strided chunk of the
        # prefill — in a hipGraph each (GraphedForward)
        self.use_graph = cfg.get("hipgraph", False)
        # extension key: the chunks of the prefill that only grow the cache join the dense prefix (see _strided_prefill)
        self.dense_growth = cfg.get("dense_growth", False)
        # extension key: the host looks at the sampled tokens every N tokens.  Default 1 = the reference's control flow (it tests
        # every token before feeding it, easykv/easykv.py:257-263); N > 1 is opt-in, see TokenLog
        self.eos_poll = max(1, int(cfg.get("eos_poll", 1)))
        # extension key: element type of the K/V bank — "float16" (default), "bfloat16", or "auto" (bf16 when the model's parameters are)
        self.kv_dtype = _kv_dtype(model, cfg.get("kv_dtype", "float16"))
        if self.kv_dtype is torch.bfloat16 and streaming:
            raise ValueError("generation_config['kv_dtype'] = bfloat16 with streaming=True: RoPE-on-read has no bf16 build (use float16)")
        # extension key: storage of the K/V rows during the decode phase — None (the 16-bit rows of kv_dtype) or "fp8": the prefill runs on
        # the 16-bit bank as always and the bank is quantised once at the prefill -> decode boundary (KVBank.quantize(kv_quant): OCP e4m3fn
        # codes + one fp32 scale per row, 2 * head_dim + 8 bytes per row pair), or "mxfp4" (e2m1 codes + one E8M0 exponent per 32 elements,
        # 136 bytes per row pair; no batched form in generate_batch), or "mxfp6" (e2m3 codes, 32 per 24-byte block, + the same exponents: 200 bytes
        # per row pair; batched as well), or "fp8_mxfp4" (the FP8 keys with the MXFP4 values: 200 bytes per row pair and FP8's eviction
        # decisions; head_dim 128, batched as well), or "k16_mxfp4" (the 16-bit keys, untouched, with the MXFP4 values: 324 bytes per row pair
        # and exactly the eviction decisions of the unquantised run; head_dim 128, every GQA factor, batched as well).  The shapes each takes are engine.ROW_FORMATS'.  kv_dtype keeps meaning the 16-bit
        # type of q / k / v / out.
        self.kv_quant = kv_quant = cfg.get("kv_quant", None)
        shard = getattr(model, "layer_shard", None)
        if shard is not None and shard.world == 1:
            shard = None
        fmt = row_format(kv_quant, "generation_config['kv_quant']")
        if kv_quant is not None:
            if streaming:
                raise ValueError(f"generation_config['kv_quant'] = {kv_quant!r} with streaming=True: the quantised decode kernels have no RoPE-on-read build")
            if kv_mode == "ppl":
                raise ValueError(f"generation_config['kv_quant'] = {kv_quant!r} with kv_mode='ppl': there is no decode phase to quantise the bank for")
            if shard is not None:
                raise ValueError(f"generation_config['kv_quant'] = {kv_quant!r} is not supported on a layer-sharded model (model.layer_shard)")
        # extension key: False (default) or True — the steps of the run's bank go to the long-row call family (KVBank(long_rows=True)):
        # scored steps of any width up to the cache's capacity, where the plain family refuses beyond about 38 400 score columns; same
        # tokens and evictions wherever both run.  16-bit rows and single sequences only (generate_batch refuses it).
        self.long_rows = cfg.get("long_rows", False)
        if self.long_rows not in (False, True):
            raise ValueError(f"generation_config['long_rows'] must be False or True, not {self.long_rows!r}")
        if self.long_rows and kv_quant is not None:
            raise ValueError(f"generation_config['long_rows'] = True with kv_quant = {kv_quant!r}: the long-row scorer is built for 16-bit rows, "
                             "and the quantised decode calls have no long form")
        self.dims = n_layers, hq, hkv, d = _dims(model)
        if streaming and d in PLAIN_KEYS_HEAD_DIMS:
            raise ValueError(f"streaming=True: RoPE-on-read has no build for head_dim {d} (plain keys only)")
        if fmt is not None and d not in fmt["head_dims"]:
            raise ValueError(f"generation_config['kv_quant'] = {kv_quant!r} needs head_dim {' or '.join(map(str, fmt['head_dims']))} (this model: {d})")
        if fmt is not None and fmt["max_rep"] is not None and hq // hkv > fmt["max_rep"]:
            raise ValueError(f"generation_config['kv_quant'] = {kv_quant!r} needs a GQA factor of at most {fmt['max_rep']} (this model: {hq // hkv})")
        # the model's own attention arithmetic, read where head_dim is: attn_logit_softcapping (Gemma 2; absent or None = off) becomes the
        # cache's logit_cap, query_pre_attn_scalar (Gemma 2 / 3; absent = head_dim) its softmax scale qpas ** -0.5 (None = 1 / sqrt(head_dim))
        cap_ = getattr(model.config, "attn_logit_softcapping", None)
        self.logit_cap = None if cap_ is None else float(cap_)
        qpas = getattr(model.config, "query_pre_attn_scalar", None)
        self.sm_scale = None if qpas is None or float(qpas) == float(d) else float(qpas) ** -0.5
        if self.logit_cap is not None:      # (before any bank exists)
            what = f"a model with attn_logit_softcapping = {self.logit_cap:g}"
            if not (0.0 < self.logit_cap < float("inf")):
                raise ValueError(f"{what}: the cap must be finite and > 0")
            if streaming:
                raise ValueError(f"{what} with streaming=True: RoPE-on-read has no soft-capped build")
            if kv_quant is not None:
                raise ValueError(f"{what} with generation_config['kv_quant'] = {kv_quant!r}: there is no capped quantised decode step")
            if self.long_rows:
                raise ValueError(f"{what} with generation_config['long_rows'] = True: there is no capped long call")
            if d not in CAPPED_HEAD_DIMS:
                raise ValueError(f"{what}: soft-capped logits are built for head_dim {' and '.join(map(str, CAPPED_HEAD_DIMS))} (this model: {d})")
        # attention sinks (gpt-oss): one learned logit per layer and query head — generation_config['attention_sinks'] ([L, Hq]) or the
        # model's own `sinks` parameters (_collect_sinks) — become the cache's sinks
        self.sinks = _collect_sinks(model, cfg, n_layers, hq)
        if self.sinks is not None:      # (before any bank exists)
            what = "a model with attention sinks"
            if streaming:
                raise ValueError(f"{what} with streaming=True: RoPE-on-read has no sink build")
            if kv_quant is not None:
                raise ValueError(f"{what} with generation_config['kv_quant'] = {kv_quant!r}: there is no quantised sink decode step")
            if self.long_rows:
                raise ValueError(f"{what} with generation_config['long_rows'] = True: there is no long sink call")
            if self.logit_cap is not None:
                raise ValueError(f"{what} and attn_logit_softcapping = {self.logit_cap:g}: there is no capped sink call")
            if shard is not None:
                raise ValueError(f"{what} is not supported on a layer-sharded model (model.layer_shard)")
            if d not in SINK_HEAD_DIMS:
                raise ValueError(f"{what}: the sink kernels are built for head_dim {' and '.join(map(str, SINK_HEAD_DIMS))} (this model: {d})")
        # sliding windows (gpt-oss's local layers): opt-in by generation_config['sliding_window'] (_collect_windows); None: ignored as before
        self.windows = _collect_windows(model, cfg, n_layers)
        if self.windows is not None:      # (before any bank exists)
            what = "generation_config['sliding_window']"
            if streaming:
                raise ValueError(f"{what} with streaming=True: RoPE-on-read has no window build")
            if kv_quant is not None:
                raise ValueError(f"{what} with generation_config['kv_quant'] = {kv_quant!r}: there is no quantised window step")
            if self.long_rows:
                raise ValueError(f"{what} with generation_config['long_rows'] = True: there is no long window call")
            if self.logit_cap is not None:
                raise ValueError(f"{what} and attn_logit_softcapping = {self.logit_cap:g}: there is no capped window call")
            if self.use_graph:
                raise ValueError(f"{what} with generation_config['hipgraph']: the token position of a step's query (q_pos0) is a host scalar of "
                                 "every window call, which a captured graph would freeze")
            if shard is not None:
                raise ValueError(f"{what} is not supported on a layer-sharded model (model.layer_shard)")
            want = WINDOW_HEAD_DIM[self.sinks is not None]
            if d != want:
                raise ValueError(f"{what}: the window kernels {'with' if self.sinks is not None else 'without'} sinks are built for head_dim {want} "
                                 f"(this model: {d})")
        # extension key: 'prefill' — None (default: the reference's strided prefill, byte for byte) or 'one_shot': one-shot prompt
        # compression with pooled observation-window scores (include/easykv_hip.h, "one-shot prefill"; _one_shot_prefill): the prompt is
        # prefilled densely, the keys are scored by the last `obs_window` queries alone, the ranking values are smoothed by a 1-D pooling of
        # kernel size `score_pool` (odd; 1 = off) and op `score_pool_op` ('max' / 'avg'), and the cache is cut to the budget in ONE step.
        self.prefill = cfg.get("prefill", None)
        if self.prefill not in (None, "one_shot"):
            raise ValueError(f"generation_config['prefill'] must be None or 'one_shot', not {self.prefill!r}")
        self.one_shot = self.prefill == "one_shot"
        if self.one_shot:      # (before any bank exists)
            what = "generation_config['prefill'] = 'one_shot'"
            self.obs_window, self.score_pool, self.score_pool_op = cfg.get("obs_window", 32), cfg.get("score_pool", 7), cfg.get("score_pool_op", "max")
            isint = lambda x: isinstance(x, int) and not isinstance(x, bool)
            if not (isint(self.obs_window) and self.obs_window >= 1):
                raise ValueError(f"generation_config['obs_window'] must be an integer >= 1, not {self.obs_window!r}")
            if not (isint(self.score_pool) and self.score_pool >= 1 and self.score_pool % 2 == 1):
                raise ValueError(f"generation_config['score_pool'] is the kernel size of the pooling: an odd integer >= 1 (1 = off), not {self.score_pool!r}")
            if self.score_pool_op not in ("max", "avg"):
                raise ValueError(f"generation_config['score_pool_op'] must be 'max' or 'avg', not {self.score_pool_op!r}")
            if kv_mode not in ("encoding", "auto"):
                raise ValueError(f"{what} serves the modes 'encoding' and 'auto', not {kv_mode!r} (there is no prompt to compress in 'decoding', and 'ppl' "
                                 "needs the logits of every strided forward)")
            if streaming:
                raise ValueError(f"{what} with streaming=True: the observation step would need RoPE-on-read over the whole prompt, which has no pooled form")
            if policy not in SCORED:
                raise ValueError(f"{what} needs a scored policy ('roco', 'h2o_head', 'tova'), not {policy!r}: recency / random score nothing to select by")
            pooled = self.score_pool > 1
            if pooled and policy == "roco":
                raise ValueError(f"{what} with kv_policy='roco' and score_pool = {self.score_pool}: roco's two-stage rule has no single row to pool "
                                 "(score_pool = 1 runs it unpooled)")
            if pooled and policy == "tova" and kv_mode == "encoding":
                raise ValueError(f"{what} with kv_policy='tova' in mode 'encoding' and score_pool = {self.score_pool}: encoding mode ranks one "
                                 "head-averaged row, which has no pooled form (score_pool = 1, or mode 'auto')")
            for name, on in (("attention sinks", self.sinks is not None), ("generation_config['sliding_window']", self.windows is not None),
                             (f"attn_logit_softcapping = {self.logit_cap}", self.logit_cap is not None),
                             ("generation_config['long_rows'] = True", bool(self.long_rows))):
                if pooled and on:
                    raise ValueError(f"{what} with score_pool = {self.score_pool} on a model with {name}: there is no pooled sink, window, capped or "
                                     "long call (score_pool = 1 runs the observation step through the model's own call family)")
            # The observation step is one chunk step of obs_window queries: its GQA-folded rows are cut into query blocks of at most 128
            # rows (32 at head_dim 256 and on capped / sink / window models), so the GQA factor must fit a block; and the generic scorer keeps
            # (max, 1 / sum) of every folded row in LDS next to its score rows: 4096 rows (32 KB) leave the key row its full width.
            rep, block = hq // hkv, 32 if (d in PLAIN_KEYS_HEAD_DIMS or self.logit_cap is not None or self.sinks is not None or self.windows is not None) else 128
            self.obs_max = 0 if rep > block else 4096 // rep
            if self.obs_window > self.obs_max:
                raise ValueError(f"{what}: obs_window = {self.obs_window} is more than one chunk step takes at this model's GQA factor {rep}; the largest "
                                 f"that works is {self.obs_max}")
        # extension key: 'head_budgets' — None / 'uniform' (default: every KV head keeps the same number of rows, today's plans) or
        # 'adaptive': the one-shot observation step shares a layer's H * n_evict evictions out among its heads by their pooled ranking
        # values (include/easykv_hip.h, "adaptive head budgets"), between a floor and a ceiling of a head's keep, fractions of the
        # uniform candidate keep K = C - n_evict: evict_max = C - floor(head_budget_floor * K), evict_min = max(0, C - ceil(head_budget_ceil * K)).
        self.head_budgets = cfg.get("head_budgets", None)
        if self.head_budgets not in (None, "uniform", "adaptive"):
            raise ValueError(f"generation_config['head_budgets'] must be None, 'uniform' or 'adaptive', not {self.head_budgets!r}")
        self.adaptive = self.head_budgets == "adaptive"
        if self.adaptive:      # (before any bank exists)
            what = "generation_config['head_budgets'] = 'adaptive'"
            self.head_floor, self.head_ceil = cfg.get("head_budget_floor", 0.2), cfg.get("head_budget_ceil", 2.0)
            isnum = lambda x: isinstance(x, (int, float)) and not isinstance(x, bool)
            if not (isnum(self.head_floor) and 0.0 <= self.head_floor <= 1.0):
                raise ValueError(f"generation_config['head_budget_floor'] must be a number in [0, 1], not {self.head_floor!r}")
            if not (isnum(self.head_ceil) and self.head_ceil >= 1.0):
                raise ValueError(f"generation_config['head_budget_ceil'] must be a number >= 1, not {self.head_ceil!r}")
            if not self.one_shot:
                raise ValueError(f"{what} needs generation_config['prefill'] = 'one_shot': the heads' shares are decided in the one observation step")
            if len(prompts) != 1:
                raise ValueError(f"{what} is not supported by generate_batch: a batch has no entries for heads of different lengths")
            if policy not in ("h2o_head", "tova"):
                raise ValueError(f"{what} serves kv_policy 'h2o_head' and 'tova', not {policy!r}")
            if policy == "tova" and kv_mode == "encoding":
                raise ValueError(f"{what} with kv_policy='tova' in mode 'encoding': encoding mode ranks one head-averaged row, the same for every head "
                                 "(mode 'auto')")
            for name, on in (("attention sinks", self.sinks is not None), ("generation_config['sliding_window']", self.windows is not None),
                             (f"attn_logit_softcapping = {self.logit_cap}", self.logit_cap is not None),
                             ("generation_config['long_rows'] = True", bool(self.long_rows)), (f"generation_config['kv_quant'] = {self.kv_quant!r}", self.kv_quant is not None),
                             ("generation_config['hipgraph']", bool(self.use_graph)), ("a layer-sharded model (model.layer_shard)", shard is not None)):
                if on:
                    raise ValueError(f"{what} with {name}: there is no adaptive sink, window, capped, long or quantised call, and the decode steps over "
                                     "heads of different lengths are neither captured nor sharded")
            if hkv > 64 or hq // hkv > 8:
                raise ValueError(f"{what}: the decode steps over heads of different lengths serve at most 64 KV heads and GQA factors up to 8 "
                                 f"(this model: {hkv} KV heads, GQA factor {hq // hkv})")
        # extension key: 'head_decode' — None / 'view' (default: the decode steps of a bank whose heads differ run whole, layer by layer, through
        # the batched call on the one-head view, KVBank._attend_ragged) or 'deferred': they run like a uniform bank's — attention + fold
        # per layer, one scorer launch per token — through the heads family (include/easykv_hip.h, "heads").  Opt-in: other kernel kinds
        # run, so rounding may differ.
        self.head_decode = cfg.get("head_decode", None)
        if self.head_decode not in (None, "view", "deferred"):
            raise ValueError(f"generation_config['head_decode'] must be None, 'view' or 'deferred', not {self.head_decode!r}")
        if self.head_decode is not None and not self.adaptive:      # (before any bank exists)
            raise ValueError("generation_config['head_decode'] needs generation_config['head_budgets'] = 'adaptive': only adaptive head budgets "
                             "leave heads of different lengths")
        self.dev = torch.device(model.device)
        for p in prompts:
            if p.dim() != 2 or p.shape[0] != 1:
                raise ValueError(f"input_ids must be [1, S] (batch size 1, as the reference); got {tuple(p.shape)}")
        self.scored = policy in SCORED
        self.evicting = policy in KNOWN_POLICIES and policy != "full"   # unknown strings evict nothing
        # Layer sharding: a model that carries ``layer_shard`` (easykv_amd.dist.LayerShard) runs only its own
        # block of layers in this process; every rank drives the same loop (the plans depend on lengths only), the bank of a
        # rank holds its layers only, the model's forward moves the stage output to the next rank, and the sampled token comes
        # from the last stage.
        self.shard = shard
        if shard is not None:
            if shard.world > n_layers or shard.count < 1:
                raise ValueError(f"layer sharding over {shard.world} ranks needs at least one of the model's {n_layers} layers per rank")
            if self.use_graph:
                # a captured forward would contain the stage hand-off (dist.send / dist.recv and, on gloo, host staging)
                raise ValueError("generation_config['hipgraph'] is not supported on a layer-sharded model (model.layer_shard)")
        self.layers = (shard.begin, shard.count) if shard is not None else (0, n_layers)
        if kv_mode == "auto":                                      # easykv/easykv.py:220-227 (resolved per prompt by _prefill)
            assert type(self.budget) == int
        # HF seam + streaming: the stock attention module hands over q/k already rotated by the TRUE positions, while the
        # streaming variant caches un-rotated keys and rotates by slot index on every read (llama_patch.py:310-327).  The
        # model's own rotary module supplies both the tables for the read-time rotation and the ones to take its rotation off.
        self.hf_stream = streaming and getattr(model.config, "_attn_implementation", None) == "easykv_amd"
        rp = getattr(model.config, "rope_parameters", None) or {}
        if streaming and not self.hf_stream:
            # native contract: the rotation at read time uses theta = config.rope_theta (Llama-3: 5e5, Mistral: 1e6); scaled
            # RoPE variants need the caller's own tables (generation_config['rope_tables'] = (cos, sin) fp32 [>= cap, D])
            scaling = getattr(model.config, "rope_scaling", None) or (rp if rp.get("rope_type", "default") != "default" else None)
            if scaling and cfg.get("rope_tables") is None:
                raise ValueError("streaming=True on a model with scaled RoPE needs generation_config['rope_tables'] = (cos, sin)")
        self.rope_base = float(getattr(model.config, "rope_theta", None) or rp.get("rope_theta", 10000.0))

    def draw(self, n, mask_tail=0):
        """kv_policy='random': the reference's own draw — argmax of torch.rand on the global CPU generator over the row
        (easykv/easykv.py:354-356; the chunk's own columns excluded in prefill, :494-497), so a run seeded like a reference run
        evicts the same slots.  Layer-sharded: every rank draws (generators seeded alike stay in step) and rank 0's value is the
        one all ranks evict, as the reference evicts one range in all layers."""
        draw = torch.rand(n)
        if mask_tail:
            draw[-mask_tail:] = -1e9
        e = int(torch.topk(draw, k=1, dim=-1)[1][0])
        return e if self.shard is None else int(_dist().broadcast_object(e, 0))

    def new_cache(self, cap, length):
        n_layers, hq, h, d = self.dims
        hf_rope = self.cfg.get("rope_tables")
        if self.hf_stream:     # tables cover every slot index (< cap) and every true position (< length + max_new_tokens)
            from . import hf
            hf_rope = hf.rope_tables_from_model(self.model, max(cap + 8, length + self.max_new_tokens + 1) + 64, d, self.dev)
        cache = BudgetedKVCache(n_layers, hq, h, d, cap + 8, self.dev, streaming=self.streaming, record=self.record, rope=hf_rope,
                                layer_begin=self.layers[0], layer_count=self.layers[1], rope_base=self.rope_base, dtype=self.kv_dtype,
                                **(dict(long_rows=True) if self.long_rows else {}),      # (opt-in: named only when asked for)
                                **{k: v for k, v in (("logit_cap", self.logit_cap), ("sm_scale", self.sm_scale), ("sinks", self.sinks),
                                                    ("windows", self.windows)) if v is not None})
        cache.unrotate = hf_rope if self.hf_stream else None
        if self.head_decode == "deferred":      # (opt-in: set only when asked for)
            cache.head_decode = "deferred"
        return cache

    def forward(self, cache, ids, positions, plan):
        plan.streaming = self.streaming
        pos = torch.as_tensor(positions, dtype=torch.long, device=self.dev)
        with cache.active(plan, pos):
            out = self.model(input_ids=ids, past_key_values=cache, position_ids=pos.view(1, -1), use_cache=True)
        # every owned layer must have gone through attend() exactly once: a model whose attention was not routed here
        # (an un-patched HF model) would otherwise silently run stock attention over the new rows only
        if cache.n_attend != cache.layer_count:
            raise RuntimeError(f"model forward made {cache.n_attend} attend() calls for {cache.layer_count} owned layers: route "
                               "every attention layer through past_key_values.attend (easykv_amd.hf.patch_model for HF models)")
        return out

    def sample(self, logits_last):
        """Next token ``[rows, 1]`` on the device.  Sharded: only the last stage holds the logits; its draw is broadcast."""
        last_rank = self.shard.world - 1 if self.shard is not None else 0
        if self.shard is None or self.shard.rank == last_rank:
            prob, raw = logits_adapter(logits_last.float(), self.temperature, self.top_p)
            tok = torch.multinomial(prob, num_samples=1)
        else:
            tok = torch.zeros(1, 1, dtype=torch.long, device=self.dev)
        return tok if self.shard is None else _dist().broadcast(tok, last_rank)


class TokenLog:
    """Sampled tokens stay on the device.  The reference pulls every token to the host to test it for EOS
    (`.cpu()` / `.item()`, ~5 syncs per token, easykv/easykv.py:257-283); here the host polls the device-side log once per
    ``eos_poll`` tokens: ONE host sync per ``eos_poll`` tokens.  ``eos_poll=1`` (the default) is the reference's exact
    control flow: nothing runs past an EOS.  With N > 1 (opt-in) up to N-1 forwards run past an EOS before it is seen:
    the returned text and the printed budget line are still the reference's (cut at the first EOS; counts derived from
    the EOS index, not from the cache), but those forwards have evicted from the cache handed back by
    ``return_cache=True`` and have drawn from the sampler's / the 'random' policy's generators."""

    def __init__(self, max_new_tokens, eos_token_ids, eos_poll, dev):
        self.max_new_tokens, self.eos_poll = max_new_tokens, eos_poll
        self.buf = torch.empty(max(1, max_new_tokens), dtype=torch.long, device=dev)
        self.eos = torch.as_tensor([int(e) for e in eos_token_ids], dtype=torch.long, device=dev)
        self.n = self.checked = self.syncs = self.sampled = 0
        self.stopped_by_eos = False

    def push(self, tok):
        self.buf[self.n:self.n + 1].copy_(tok.view(1))
        self.n += 1
        self.sampled += 1      # every token drawn, including those past an EOS a later poll cuts off

    def poll(self):
        """True when the loop must stop: an EOS was found among the tokens not looked at yet (``n`` is cut back to it)."""
        if self.n - self.checked < self.eos_poll and self.n < self.max_new_tokens:
            return False
        hit = torch.isin(self.buf[self.checked:self.n], self.eos).cpu()     # the one host sync of this poll
        self.syncs += 1
        first = self.checked
        self.checked = self.n
        if bool(hit.any()):
            self.n = first + int(torch.nonzero(hit)[0, 0]) + 1
            self.stopped_by_eos = True
            return True
        return False

    def ids(self):
        return self.buf[:self.n].cpu().tolist()

    @property
    def fed(self):   # tokens the reference would have fed back into the model (:257-264: the EOS token itself is not)
        return self.n - 1 if self.stopped_by_eos else self.n


class GraphedForward:
    """One forward of the WHOLE model captured in a hipGraph — a decode step (one token), or, since round 6, a
    strided chunk of the prefill (`stride` tokens).  At a fixed budget every evicting forward has the same shapes, the same
    StepPlan and the same cache length before and after (the cache oscillates idx <-> idx + stride, easykv/easykv.py:426-433), so
    the host work of a forward (HF's per-layer Python, ~0.4 ms per layer: 12 ms of a 13 ms chunk forward of a 32-layer model) is
    paid once at capture and a forward costs one graph launch.  Token ids and positions live in static device tensors; sampling, the
    EOS test and the collection of logits / evicted ids stay outside the graph."""

    def __init__(self, model, cache, plan, tok, positions, streaming=False):
        n = len(positions)
        self.tok = tok.view(1, n).clone()
        self.pos = torch.as_tensor(positions, dtype=torch.long).to(tok.device)
        self.graph = torch.cuda.CUDAGraph()
        plan.streaming = streaming
        self.cache = cache
        n_recorded = len(cache.evictions)
        tk = _ACTIVE.set(cache)
        try:
            with torch.cuda.graph(self.graph):      # capture launches nothing: the first replay runs this forward
                cache.begin_forward(plan, self.pos)
                self.logits = model(input_ids=self.tok, past_key_values=cache, position_ids=self.pos.view(1, -1), use_cache=True).logits
        finally:
            _ACTIVE.reset(tk)
        if cache.n_attend != cache.layer_count:
            raise RuntimeError(f"model forward made {cache.n_attend} attend() calls for {cache.layer_count} owned layers")
        # record=True: the captured forward left its (static) id tensors in the log; every replay appends a copy instead
        self.static_ids = cache.evictions.pop() if len(cache.evictions) > n_recorded else None
        self.layout = cache.bank.layout_signature()     # the captured kernels are those of THIS score-row layout

    def __call__(self, tok, positions):
        if self.cache.bank.layout_signature() != self.layout:
            raise RuntimeError("the bank's score-row layout changed between capture and replay of the forward's graph "
                               "(an eager call on the bank in between): capture again")
        self.tok.copy_(tok.view(self.tok.shape))
        if len(positions) == 1:
            self.pos.fill_(positions[0])
        else:      # (consecutive positions, built on the device: no host-to-device copy on the replay path)
            torch.arange(positions[0], positions[0] + len(positions), dtype=torch.long, device=self.pos.device, out=self.pos)
        self.graph.replay()
        if self.static_ids is not None:
            self.cache.evictions.append([t.clone() for t in self.static_ids])
        return self.logits


class DecodePlanner:
    """The per-token decode rule of ONE sequence (easykv/easykv.py:287-362; the tail of auto mode, :708-747): whether a step evicts,
    and for recency / random which slot.  ``score_off``: first position the score rows cover (decoding: the prompt length — only
    generated slots are evicted); ``budget_d``: slots from there on the cache may hold; ``whole_cache``: auto mode, every step evicts
    over the whole cache.  Plain decode without eviction (encoding mode, :508-526) is policy "full" with ``score_off = budget_d = 0``.
    :func:`generate` drives one planner, :func:`generate_batch` one per sequence."""

    def __init__(self, policy, sink, score_off, budget_d, whole_cache, cur_pos, draw):
        self.policy, self.sink, self.score_off, self.budget_d, self.whole_cache = policy, sink, score_off, budget_d, whole_cache
        self.scored = policy in SCORED
        self.evicting = policy in KNOWN_POLICIES and policy != "full"
        self.cur_pos = cur_pos                  # true position of the token the next step feeds
        self.positions: List[int] = []          # true positions of the fed tokens still in the cache (recency / random)
        self.draw = draw                        # n -> index of the 'random' victim among n generated slots (_Run.draw)

    def step(self, t_before: int) -> StepPlan:
        """The plan of the step that feeds the token at ``cur_pos`` to a cache of ``t_before`` slots; moves on to the next position."""
        policy, score_off = self.policy, self.score_off
        evict = self.evicting and (self.whole_cache or (t_before + 1 - score_off) > self.budget_d)     # :303 / every step :708
        plan = StepPlan(policy=policy, phase="decode", accumulate=self.scored, evict=evict, score_off=score_off, budget=self.budget_d)
        self.positions.append(self.cur_pos)
        self.cur_pos += 1
        if evict and policy in ("recency", "random"):
            if self.whole_cache:                            # :741-747
                if policy == "random":
                    raise UnboundLocalError("auto mode + kv_policy='random' is broken in the reference (easykv/easykv.py:744)")
                plan.range_start = self.sink
            else:                                           # :343-362: oldest / uniformly random generated slot
                e = 0 if policy == "recency" else self.draw(len(self.positions))
                self.positions.pop(e)
                plan.range_start = score_off + e
        return plan


@dataclasses.dataclass
class Prefilled:
    """What the decode phase of one sequence starts from (:func:`_prefill`)."""
    cache: Optional[BudgetedKVCache]
    logits: torch.Tensor         # [1, V]: the logits of the prompt's last token
    planner: DecodePlanner
    mode: str                    # "decoding" | "encoding" | "encoding_decoding" ('auto' resolved)
    length: int                  # prompt length


# ------------------------------------------------------------------------------------------------
# prefill (easykv/easykv.py:228-245, :367-503, :530-669), decode, report; generate and generate_batch on top of them
# ------------------------------------------------------------------------------------------------
def _strided_prefill(run, cache, input_ids, budget_p, idx, r_idx, tova_head_mean, keep_logits=False):
    """Dense prefix + strided chunks with eviction (encoding, auto, ppl).  -> (last logits, [logits per forward], [their token ids])"""
    length, stride, policy, sink, keep_attention = input_ids.shape[-1], run.stride, run.policy, run.sink, run.keep_attention
    recent = int(budget_p * run.recent_ratio)                # :394
    cache.bank.state_init(idx + stride, 1 if keep_attention else 2, stride)       # :412-416
    cache.score_prefix = keep_attention
    # prefix [0, r_idx): dense causal; with keep_attention its probabilities seed S and Q (:396, :403-405)
    plan = StepPlan(policy="roco" if keep_attention else "full", phase="prefill", accumulate=keep_attention,
                    evict=False, stride=stride)
    # extension key `dense_growth` (default off = the reference's forward sequence): the chunks that only GROW the cache —
    # tokens [r_idx, idx): no eviction, and without keep_attention no accumulation either (easykv.py:443, :460) — attend
    # causally to everything before them, which is what the dense prefix does: they join it as ONE forward of idx tokens.
    # auto / ppl geometry takes the smallest r_idx (:551-552, :779-780), i.e. (idx - r_idx) / stride shape-changing forwards
    # that no graph can replay (256 of the 511 forwards of a 4096-token prompt at stride 8).  Same K / V rows, same state, same
    # evictions afterwards; with keep_attention the prefix' column sums are formed in one sweep instead of chunk by chunk
    # (equal up to fp32 summation order).
    r_dense = idx if run.dense_growth else r_idx
    out = run.forward(cache, input_ids[:, :r_dense], list(range(r_dense)), plan)
    cache.score_prefix = False
    logits_last = out.logits[:, -1, :]
    all_logits, all_ids = [], []
    if keep_logits and r_dense > r_idx:      # (ppl mode collects the logits of every token from r_idx on, :816-901)
        all_logits.append(out.logits[0, r_idx:r_dense])
        all_ids.append(input_ids[0, r_idx:r_dense])
    graphed, prev_sig = None, None
    for tok_i in range(r_dense, length, stride):              # :426
        t_now = cache.get_seq_length() + stride
        plan = StepPlan(policy=policy, phase="prefill", accumulate=run.scored and (t_now > idx or keep_attention),
                        evict=run.evicting and t_now > idx, budget=budget_p, recent=recent, sink=sink, stride=stride,
                        tova_head_mean=tova_head_mean)
        if plan.evict and policy == "recency":
            plan.range_start = sink                          # :491-493
        elif plan.evict and policy == "random":              # :494-499: argmax of torch.rand over the row, chunk excluded
            plan.range_start = run.draw(idx + stride, stride)
        # steady state (generation_config['hipgraph']): from the second evicting chunk on every forward has the plan, the shapes and
        # the cache length of the one before it — captured once, replayed for the rest of the prompt
        sig = (t_now, plan.accumulate, plan.evict, plan.range_start)
        chunk_ids, chunk_pos = input_ids[:, tok_i:tok_i + stride], list(range(tok_i, tok_i + stride))
        if run.use_graph and plan.evict and policy != "random" and sig == prev_sig and chunk_ids.shape[1] == stride:
            if graphed is None:
                graphed = GraphedForward(run.model, cache, plan, chunk_ids, chunk_pos, run.streaming)
            logits = graphed(chunk_ids, chunk_pos)
            if keep_logits:
                logits = logits.clone()      # (the graph's output buffer is overwritten by the next replay)
        else:
            logits = run.forward(cache, chunk_ids, chunk_pos, plan).logits
        prev_sig = sig
        logits_last = logits[:, -1, :]
        if keep_logits:
            all_logits.append(logits[0])
            all_ids.append(input_ids[0, tok_i:tok_i + stride])
    cache.bank.release_workspace(keep_bytes=64 << 20)      # (deferred chunk steps keep all layers' logits / column sums: not the decode phase's business)
    return logits_last, all_logits, all_ids


def _one_shot_prefill(run, input_ids, budget, cap_decode, tova_head_mean, grow=1):
    """One-shot prompt compression (include/easykv_hip.h, "one-shot prefill"): two forwards and a hand-over.  ``budget``: the resolved
    integer budget B < n; ``cap_decode``: the capacity the same mode's strided prefill would have given the cache; ``grow``: rows a head
    gains in the decode phase (adaptive head budgets size the decode bank by the ceiling of a head's keep).  -> (cache, last logits)"""
    n, obs, sink = input_ids.shape[-1], run.obs_window, run.sink
    if obs >= n or budget < obs + sink:
        raise ValueError(f"generation_config['prefill'] = 'one_shot': obs_window = {obs} does not fit a prompt of {n} tokens cut to {budget} "
                         f"(the {sink} sink tokens and the observation window are always kept); the largest that works is {max(0, min(n - 1, budget - sink))}")
    adaptive = None
    if run.adaptive:      # (the bounds of a head's victims; the decode bank holds the ceiling's rows, not what a sync would report)
        C, n_evict = n - obs - sink, n - budget
        K = C - n_evict
        adaptive = (max(0, C - math.ceil(run.head_ceil * K)), C - math.floor(run.head_floor * K))
        longest = n - adaptive[0]
        if longest + grow > 6144:
            raise ValueError(f"generation_config['head_budgets'] = 'adaptive': a head may keep {longest} rows (+ {grow} decoded), more than the 6144 "
                             "slots per head the decode steps over heads of different lengths take; lower head_budget_ceil or the budget")
        cap_decode = (longest + grow + 3) // 4 * 4
    # the prefill's peak memory is the whole prompt's K/V: a bank of n rows, released at the hand-over
    cache = run.new_cache(n, n)
    dense = StepPlan(policy="full", phase="prefill", accumulate=False)
    run.forward(cache, input_ids[:, :n - obs], list(range(n - obs)), dense)                      # forward A
    cache.bank.state_init(n, 2, obs)
    plan = StepPlan(policy=run.policy, phase="prefill", accumulate=True, evict=True, budget=n, recent=obs, sink=sink, stride=obs,
                    tova_head_mean=tova_head_mean and run.policy == "tova",      # (the head-averaged row is tova's alone; a pooled step refuses the flag)
                    n_evict=n - budget, pool=run.score_pool, pool_op=run.score_pool_op, **(dict(head_adaptive=adaptive) if adaptive else {}))
    logits = run.forward(cache, input_ids[:, n - obs:], list(range(n - obs, n)), plan).logits[:, -1, :]      # forward B: score, pool, select once
    # hand-over: the decode steps stream the physical rows [0, extent) of every head; without it that is the prompt's n rows for the rest
    # of the generation
    cache.bank = cache.bank.hand_over(cap_decode + 8)
    return cache, logits


def _print_budget_line(mode, length, size, n_out=0, fed=0, budget_d=None):
    """The reference's report, one function of the mode and the counts.  ``size``: live slots when the line is printed — encoding:
    right after the prefill (:503); auto: after the last step (:751).  decoding (:364-365) reports the generated slots kept, derived
    from the tokens ``fed`` (== cache length - prompt length when no forward ran past an EOS); ``budget_d`` None = nothing evicts."""
    if mode == "encoding_decoding":
        print(f"KV Cache Budget ratio {size / (length + n_out) * 100:.2f}%[{size}/({length}+{n_out})]")
    else:
        kept, of = (size, length) if mode == "encoding" else (fed if budget_d is None else min(fed, budget_d), n_out)
        print(f"KV cache budget ratio: {kept / of * 100:.2f}%({kept}/{of})")


def _prefill(run: _Run, input_ids, kv_mode) -> Prefilled:
    """Everything before the decode phase of ONE prompt: 'auto' resolved, geometry, the cache, dense prefix, strided chunks, the
    state of the decode rule.  Shared by :func:`generate` and, prompt by prompt, :func:`generate_batch`."""
    length, budget, stride = input_ids.shape[-1], run.budget, run.stride
    input_ids = input_ids.to(run.dev)
    if kv_mode == "auto":                                        # easykv/easykv.py:220-227
        kv_mode, budget = ("decoding", budget - length) if budget > length else ("encoding_decoding", budget)
    dense = StepPlan(policy="full", phase="prefill", accumulate=False)
    if kv_mode == "decoding":                                    # :228-366
        cache = run.new_cache(length + (budget + 1 if run.evicting else run.max_new_tokens + 1), length)
        logits = run.forward(cache, input_ids, list(range(length)), dense).logits[:, -1, :]
        if run.evicting and run.scored:
            cache.bank.state_init(budget + 1, 0)                 # :242-245
        rule = dict(policy=run.policy, score_off=length, budget_d=budget, whole_cache=False)
    elif kv_mode == "encoding":                                  # :367-529
        if (type(budget) == float and budget >= 1.0) or (type(budget) == int and budget >= length):
            cache = run.new_cache(length + run.max_new_tokens, length)
            logits = run.forward(cache, input_ids, list(range(length)), dense).logits[:, -1, :]
        else:
            budget_p, idx, r_idx = geometry("encoding", length, budget, stride)
            if run.one_shot:      # (the resolved integer budget: B < length here)
                cache, logits = _one_shot_prefill(run, input_ids, int(length * budget) if type(budget) == float else budget,
                                                  idx + stride + run.max_new_tokens, True, run.max_new_tokens)
            else:
                # 'full' / unknown policy strings evict nothing (the reference's cache just grows): size for the whole prompt
                cache = run.new_cache((idx + stride if run.evicting else length) + run.max_new_tokens, length)
                logits = _strided_prefill(run, cache, input_ids, budget_p, idx, r_idx, True)[0]
        _print_budget_line("encoding", length, cache.get_seq_length())
        rule = dict(policy="full", score_off=0, budget_d=0, whole_cache=False)      # :508-526 plain decode, no eviction
    elif kv_mode == "encoding_decoding":                         # :530-753
        assert type(budget) == int and budget <= length
        white_lst = ["random", "recency", "tova", "roco"]
        assert run.policy in white_lst, f"mode must be within {white_lst}, get {run.policy} instead"
        assert stride > 1, "auto mode needs stride > 1 (the reference asserts at easykv/easykv.py:666-669)"
        budget_p, idx, r_idx = geometry("auto", length, budget, stride)
        if run.one_shot and budget < length:
            cache, logits = _one_shot_prefill(run, input_ids, budget, idx + stride + 1, False)
            # the decode policy runs over the whole cache with budget B, on the score rows the observation step left
            rule = dict(policy=run.policy, score_off=0, budget_d=budget, whole_cache=True)
        else:
            cache = run.new_cache(idx + stride + 1, length)
            logits = _strided_prefill(run, cache, input_ids, budget_p, idx, r_idx, False)[0]
            # the score rows keep their first idx+1 columns (:666-669); the decode rules then run over the whole cache
            rule = dict(policy=run.policy, score_off=0, budget_d=budget_p, whole_cache=True)
    else:
        raise ValueError(f"unknown kv_mode {kv_mode!r}")
    return Prefilled(cache, logits, DecodePlanner(sink=run.sink, cur_pos=length, draw=run.draw, **rule), kv_mode, length)


def _decode(run: _Run, pre: Prefilled, report_latency=False):
    """The decode phase of one sequence (:257-366, :508-526, :670-747): sample, test for EOS, plan, forward.  -> (token ids, tokens fed)"""
    cache, planner, logits_last = pre.cache, pre.planner, pre.logits
    log = TokenLog(run.max_new_tokens, run.eos_token_ids, run.eos_poll, run.dev)
    graphed, prev_sig, n_fwd, t_first = None, None, 0, None
    while log.n < run.max_new_tokens:                           # :257 / :670
        tok = run.sample(logits_last)
        log.push(tok)
        if log.poll():
            break
        t_now, pos = cache.get_seq_length() + 1, [planner.cur_pos]
        plan = planner.step(t_now - 1)
        # steady state (same plan, same cache length as the step before, one slot evicted per step): replay the graph
        sig = (t_now, plan.evict, plan.range_start)
        if run.use_graph and plan.evict and planner.policy != "random" and sig == prev_sig:
            if graphed is None:
                graphed = GraphedForward(run.model, cache, plan, tok, pos, run.streaming)
            logits_last = graphed(tok, pos)[:, -1, :]
        else:
            logits_last = run.forward(cache, tok.view(1, 1), pos, plan).logits[:, -1, :]
        prev_sig = sig
        n_fwd += 1
        if report_latency and n_fwd == 1:                       # the reference drops the first step from the mean (:527)
            torch.cuda.synchronize(run.dev)
            t_first = time.time()
    cache.host_syncs, cache.tokens_sampled = log.syncs, log.sampled
    if report_latency and n_fwd > 1:
        torch.cuda.synchronize(run.dev)
        print(f"Per-step decoding latency: {(time.time() - t_first) / (n_fwd - 1):.3f}")
    return log.ids(), log.fed


def _perplexity(run: _Run, input_ids):
    """kv_mode='ppl' (easykv/easykv.py:754-901): the strided prefill alone, keeping every token's logits.  -> (perplexity, cache)"""
    length, budget, shard = input_ids.shape[-1], run.budget, run.shard
    input_ids = input_ids.to(run.dev)
    has_logits = shard is None or shard.rank == shard.world - 1     # sharded: the logits exist on the last stage only
    if budget >= 1.0:     # NB: like the reference, ANY int budget takes this branch (:759); pass a ratio to evict
        cache = run.new_cache(length, length)
        out = run.forward(cache, input_ids, list(range(length)), StepPlan(policy="full", phase="prefill", accumulate=False))
        all_logits, all_ids = ([out.logits[0]], [input_ids[0]]) if has_logits else ([], [])
    else:
        budget_p, idx, r_idx = geometry("ppl", length, budget, run.stride)
        cache = run.new_cache(idx + run.stride if run.evicting else length, length)
        _, all_logits, all_ids = _strided_prefill(run, cache, input_ids, budget_p, idx, r_idx, True, keep_logits=has_logits)
        _print_budget_line("encoding", length, cache.get_seq_length())
    result = None
    if has_logits:
        ids_cat, log_cat = torch.cat(all_ids), torch.cat(all_logits, dim=0)
        assert ids_cat.shape[0] == log_cat.shape[0]
        lp = torch.nn.CrossEntropyLoss(reduction="none")(log_cat[:-1].float(), ids_cat[1:]).cpu().numpy().tolist()
        result = math.exp(statistics.mean(lp))
    if shard is not None:
        result = _dist().broadcast_object(result, shard.world - 1)
    return result, cache


@torch.inference_mode()
def generate(self, input_ids, generation_config, kv_mode="encoding", stride=1, report_decoding_latency: bool = False,
             return_cache: bool = False):
    run = _Run(self, generation_config, kv_mode, stride, [input_ids])
    if kv_mode == "ppl":
        result, cache = _perplexity(run, input_ids)
    else:
        pre = _prefill(run, input_ids, kv_mode)
        cache = pre.cache
        if run.kv_quant:      # prefill -> decode boundary: the decode steps run on quantised rows
            cache.bank.quantize(run.kv_quant)
        out_ids, fed = _decode(run, pre, report_decoding_latency and pre.mode == "encoding")
        if pre.mode != "encoding":      # (encoding mode reports the cache the prefill left: printed there)
            _print_budget_line(pre.mode, pre.length, cache.get_seq_length(), len(out_ids), fed, pre.planner.budget_d if run.evicting else None)
        result = self.tokenizer.decode(out_ids, skip_special_tokens=True).strip()
    if run.shard is not None:       # stage outputs still in flight (easykv_amd.dist.PipelineStage posts them without waiting)
        _dist().drain_stages()
    return (result, cache) if return_cache else result


@torch.inference_mode()
def generate_batch(self, input_ids_list, generation_config, kv_mode="encoding", stride=1, return_cache: bool = False):
    """``generate`` for several prompts of different lengths: every prompt is prefilled ALONE through :func:`_prefill`, as
    ``generate`` does it (all modes keep the reference's geometry), its bank becomes one sequence of a :class:`KVBankBatch`, and the
    decode phase then runs ONE model forward per token for all live sequences — ``input_ids [B', 1]``, ``position_ids [B', 1]`` with
    each sequence's own position, one batched library step per layer.  Each sequence's plan comes from its own
    :class:`DecodePlanner` (it evicts when ITS length exceeds ITS budget, ``score_off`` = ITS prompt length, recency / random ranges
    per sequence) and a sequence leaves the batch when it samples an EOS or has been fed ``max_new_tokens`` tokens.  Returns the
    decoded strings, in prompt order, and prints each sequence's budget line as ``generate`` prints it.
    ``generation_config['kv_quant'] = 'fp8'``: every prompt's bank is quantised right after its own 16-bit prefill (as ``generate``
    does at the prefill -> decode boundary) and the decode phase runs one FP8 batched step per layer and token.  ``'mxfp6'``: the same
    on MXFP6 rows (head_dim 128, GQA factors up to 4); ``'fp8_mxfp4'``: the same on FP8 keys with MXFP4 values (head_dim 128);
    ``'k16_mxfp4'``: the same on 16-bit keys with MXFP4 values (head_dim 128; the evictions of the unquantised run).
    ``'mxfp4'`` is refused here.

    Sampling: ``torch.multinomial`` draws for all live sequences at once, so with ``temperature`` / ``top_p`` that leave more than
    one candidate the global generator is consumed differently from B solo runs; ``kv_policy='random'`` draws once per sequence
    and step, in batch order."""
    cfg = generation_config
    if cfg.get("streaming", False):
        raise ValueError("generate_batch: streaming=True (RoPE-on-read) has no batched decode step")
    if kv_mode == "ppl":
        raise ValueError("generate_batch: kv_mode='ppl' has no decode phase to batch")
    if cfg.get("hipgraph", False):
        raise ValueError("generate_batch: generation_config['hipgraph'] is not supported")
    if getattr(self, "layer_shard", None) is not None and self.layer_shard.world > 1:
        raise ValueError("generate_batch is not supported on a layer-sharded model (model.layer_shard)")
    if cfg.get("long_rows", False):
        raise ValueError("generate_batch: generation_config['long_rows'] has no batched decode step (the long-row scorer serves single sequences)")
    if cfg.get("kv_quant", None) == "mxfp4":
        raise ValueError("generate_batch: generation_config['kv_quant'] = 'mxfp4' has no batched decode step (use 'fp8' or None)")
    if getattr(self.config, "attn_logit_softcapping", None) is not None:
        raise ValueError("generate_batch: a model with attn_logit_softcapping has no batched decode step (soft-capped logits serve single sequences)")
    if _collect_sinks(self, cfg, *_dims(self)[:2]) is not None:
        raise ValueError("generate_batch: a model with attention sinks has no batched decode step (the sink kernels serve single sequences)")
    if cfg.get("sliding_window", None) is not None:
        raise ValueError("generate_batch: generation_config['sliding_window'] has no batched decode step (the window kernels serve single sequences)")
    prompts = [p.view(1, -1) if p.dim() == 1 else p for p in input_ids_list]
    if not 1 <= len(prompts) <= _lib.MAX_SEQS or any(p.dim() != 2 or p.shape[0] != 1 for p in prompts):
        raise ValueError(f"generate_batch takes 1..{_lib.MAX_SEQS} prompts of shape [S] or [1, S]")
    run = _Run(self, cfg, kv_mode, stride, prompts)
    eos, dev, max_new_tokens = set(int(e) for e in run.eos_token_ids), run.dev, run.max_new_tokens

    # ---- every prompt alone, through the single-sequence prefill; its bank becomes one sequence of the batch
    # (kv_quant='fp8' / 'mxfp6' / 'fp8_mxfp4' / 'k16_mxfp4': a prompt's bank is quantised right after its own prefill, so at most one 16-bit bank is alive at a time, and the
    # batch bank is created holding that format's planes only)
    seqs = []
    for p in prompts:
        seqs.append(_prefill(run, p, kv_mode))
        if run.kv_quant:
            seqs[-1].cache.bank.quantize(run.kv_quant)
    first = seqs[0].cache.bank
    rows = dict(kv_quant=run.kv_quant) if run.kv_quant else {}      # (the format's planes only: the 16-bit rows of the batch are never allocated)
    bat = KVBankBatch(len(seqs), first.n_layers, first.n_q_heads, first.n_kv_heads, first.head_dim, max(s.cache.bank.cap for s in seqs),
                      device=dev, dtype=first.dtype, **rows, **(dict(sm_scale=run.sm_scale) if run.sm_scale is not None else {}))
    cache = BudgetedKVCacheBatch(bat, record=run.record)
    for i, s in enumerate(seqs):
        bat.adopt(i, s.cache.bank)
        cache.evictions[i] = s.cache.evictions      # (the prefill's own evictions come first)
        s.cache = None
    out_ids, by_eos = [[] for _ in seqs], [False] * len(seqs)

    # ---- the decode phase: one forward per token for all live sequences
    live = list(range(len(seqs))) if max_new_tokens > 0 else []
    while live:
        tok = run.sample(torch.cat([seqs[i].logits for i in live]))       # [B', 1]
        rows, now, plans, pos = [], [], [], []
        for row, t in enumerate(tok.view(-1).tolist()):                   # (the one host sync of the step: the EOS test, easykv.py:257-263)
            i = live[row]
            out_ids[i].append(t)
            if t in eos:
                by_eos[i] = True
                continue
            rows.append(row)
            now.append(i)
            pos.append(seqs[i].planner.cur_pos)
            plans.append(seqs[i].planner.step(bat.n_slots(i)))
        if not now:
            break
        pos = torch.as_tensor(pos, dtype=torch.long, device=dev).view(-1, 1)
        with cache.active(plans, now, pos):
            out = self(input_ids=tok[torch.as_tensor(rows, device=dev)].view(-1, 1), past_key_values=cache, position_ids=pos, use_cache=True)
        if cache.n_attend != bat.n_layers:
            raise RuntimeError(f"model forward made {cache.n_attend} batched attend() calls for {bat.n_layers} layers: route every "
                               "attention layer through past_key_values.attend (easykv_amd.hf.patch_model for HF models)")
        for row, i in enumerate(now):
            seqs[i].logits = out.logits[row:row + 1, -1, :]
        live = [i for i in now if len(out_ids[i]) < max_new_tokens]

    results = []
    for i, s in enumerate(seqs):
        n_out = len(out_ids[i])
        if s.mode != "encoding":
            _print_budget_line(s.mode, s.length, bat.n_slots(i), n_out, n_out - 1 if by_eos[i] else n_out, s.planner.budget_d if run.evicting else None)
        results.append(self.tokenizer.decode(out_ids[i], skip_special_tokens=True).strip())
    return (results, cache) if return_cache else results


def enable_fixed_kv(model, tokenizer, mode, stride=1, verbose=False):
    """easykv/easykv.py:903-908."""
    model.tokenizer = tokenizer
    model.easykv_generate = functools.partial(generate, self=model, kv_mode=mode, stride=stride, report_decoding_latency=verbose)
    model.easykv_ppl = functools.partial(generate, self=model, kv_mode="ppl", stride=stride)
    model.easykv_generate_batch = functools.partial(generate_batch, self=model, kv_mode=mode, stride=stride)
    print(f"Fixed KV Cache for {mode} enabled")
