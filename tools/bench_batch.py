"""The batched decode step (ekv_batch_step_attend, KVBankBatch) against the paths a caller had before it, in one process, legs
interleaved (rep of leg a, rep of leg b, ...); writes profiles/batch_bench.json and prints it as one JSON line.

Llama2-7B head shape (Hq = H = 32, D = 128), budget 2048 (T = 2049), roco, every step evicting (steady state: lengths stay put),
scattered slot maps, warm score state, per-layer calls of a decoder stack: a "token" is one call per layer, and every leg reports
µs per per-layer call for B sequences (median over reps of per-rep means, HIP events on the launch stream) and its run-to-run spread.

Per B in {1, 2, 4, 8, 16, 32}:
  batched          one ekv_batch_step_attend per layer over the B sequences (table prebuilt: it is the same every step) — the feature
  batched_engine   the same through KVBankBatch.attend (builds the table in Python every call: what a Python caller pays today)
  solo_whole       B KVBank.attend calls of one layer each, whole-step form (attention + fold + scorer launches per call)
  solo_deferred    B attend(defer=True) calls per layer + one flush() per token (the form tools/bench_kv8.py times per layer)
  uniform_ordered  the existing multi-layer ekv_step_attend, layer_count = B, on the ORDERED score-row layout — like against like:
                   the batched instance does the same work plus a handful of scalar loads
  batched_contig   the batched call on a bank laid out as uniform_ordered's ([layer][sequence]: the B layers of a call are adjacent,
                   where KVBankBatch keeps them a whole sequence apart) — same addresses, same kernels but for the table: separates
                   what the table costs from what the [sequence][layer] layout costs
  uniform_slot     the same launch on the slot-indexed layout where the library takes it (recorded as what a follow-up that brings
                   that layout to batches would gain, not as a yardstick)
and the same B with lengths spread over [256, 2049] (fixed seed, recorded):
  ragged           one batched call per layer; against `batched` at the envelope length and against live bytes / envelope bytes
and with --kv8 (output: profiles/batch_kv8_bench.json), interleaved with the legs above on copies of the SAME rows, slot maps and
score state, quantised (KVBankBatch.quantize_fp8 / KVBank.quantize_fp8):
  batched_kv8        one ekv_kv8_batch_step_attend per layer over the B sequences (table prebuilt) — against `batched`
  solo_kv8_deferred  B FP8 attend(defer=True) calls per layer + one flush() per token — what a caller of FP8 banks had before
  ragged_kv8         the FP8 batched call at the ragged lengths — against `ragged`
and with --mxfp4 (output: profiles/batch_kv4_bench.json), interleaved in the same way with `batched`, `batched_kv8`, `ragged` and
`ragged_kv8` — the yardsticks of the same run; the other 16-bit legs are left to the two files above — on MXFP4 copies of the same
state (KVBankBatch.quantize_mxfp4 / KVBank.quantize_mxfp4):
  batched_kv4        one ekv_kv4_batch_step_attend per layer over the B sequences (table prebuilt)
  solo_kv4_deferred  B MXFP4 attend(defer=True) calls per layer + one flush() per token — what a caller of MXFP4 banks had before
  ragged_kv4         the MXFP4 batched call at the ragged lengths
plus one GQA x 4 table (Hq 32 over H 8, B = 8 and 32; key "gqa4"): `batched` and `batched_kv4` as planned, with a forced key-range split
(n_split = 8: the split kernel's GQA builds do not spill) and forced into one launch (n_split = 1: the one-launch GQA x 4 kv4 build
spills, profiles/batch_kv4_registers.txt).
Every leg also reports its algorithmic bytes per per-layer call (K+V row pair: 4 * D bytes in 16 bits, 2 * D + 8 as FP8 codes + row
scales, D + D / 16 as MXFP4 codes + block exponents, 3 D / 2 + D / 16 as MXFP6 codes + block exponents).
--mxfp6 (output: profiles/batch_kv6_bench.json) does what --mxfp4 does for MXFP6 rows — batched_kv6, solo_kv6_deferred, ragged_kv6 —
with `batched`, `batched_kv8`, `batched_kv4`, `ragged`, `ragged_kv8` and `ragged_kv4` as the yardsticks of the same interleaved run
(no GQA x 4 table).

--fp8-mxfp4 (output: profiles/batch_kv84_bench.json) does the same for FP8 keys with MXFP4 values (3 D / 2 + 4 + D / 32 bytes per row
pair) — batched_kv84, solo_kv84_deferred, ragged_kv84 — with the 16-bit, FP8, MXFP4 and MXFP6 batched / ragged legs as the yardsticks
of the same interleaved run.

--k16-mxfp4 (output: profiles/batch_kv164_bench.json) does the same for 16-bit keys with MXFP4 values (2 D + D / 2 + D / 32 bytes per row
pair) — batched_kv164, solo_kv164_deferred, ragged_kv164 — with the 16-bit, FP8 and FP8-key / MXFP4-value batched / ragged legs as the
yardsticks of the same interleaved run.

Usage: python tools/bench_batch.py [--reps 9] [--tokens 24] [--warm 20] [--batches 1,2,4,8,16,32] [--kv8 | --mxfp4 | --mxfp6 | --fp8-mxfp4 | --k16-mxfp4] [--out profiles/batch_bench.json]"""
from __future__ import annotations

import argparse
import ctypes as C
import gc
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.bench_common import HBM_PEAK_GBS, algorithmic_bytes  # noqa: E402

HQ = H = 32
D = 128
BUDGET = 2048


def _time(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(n):
        fn(i)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / n


def _interleave(fns, reps, tokens, warm):
    for f in fns.values():
        for i in range(warm):
            f(i)
    torch.cuda.synchronize()
    got = {k: [] for k in fns}
    for _ in range(reps):
        for k, f in fns.items():
            got[k].append(_time(f, tokens))
    return {k: dict(us=statistics.median(v), spread=round((max(v) - min(v)) / statistics.median(v), 4)) for k, v in got.items()}


def _fill(bank, layers, rows, g):
    """Layers of `bank` at `rows[i]` live rows each: random K/V, scattered slot map, decoding score state of width rows + 1, warm."""
    dev = bank.device
    for l, n in zip(layers, rows):
        bank.load_rows(torch.randn(1, H, n, D, generator=g, device=dev).half(), torch.randn(1, H, n, D, generator=g, device=dev).half(),
                       pos_begin=0, layer_begin=l)
        bank.slot_of_pos[l, :, :n] = torch.argsort(torch.rand(H, n, generator=g, device=dev), dim=-1).int()
        bank.state_init(n + 1, 0, layer_begin=l, layer_count=1)
        warm = torch.rand(H, n, generator=g, device=dev) * 1e-3
        bank.score_sum[l, :, :n] += warm
        bank.score_sq[l, :, :n] += warm ** 2


def _plan(budget, **kw):
    from easykv_amd import StepPlan
    return StepPlan(policy="roco", phase="decode", evict=True, score_off=0, budget=budget, **kw)


def _tokens(B, lps, g, dev, n=8):
    return tuple(torch.randn(n, lps, B, hh, 1, D, generator=g, device=dev).half() for hh in (HQ, H, H))


def _quantised_copy(src, make, rows="kv8"):
    """A bank from `make()` holding the state of `src` (rows, slot maps, score rows, lengths, extents), quantised to FP8 / MXFP4 rows."""
    dst = make()
    for name in ("k", "v", "slot_of_pos", "score_sum", "score_sq", "score_cnt"):
        getattr(dst, name).copy_(getattr(src, name))
    dst.n_slots, dst.extent = list(src.n_slots), list(src.extent)
    return dst.quantize({"kv4": "mxfp4", "kv6": "mxfp6", "kv84": "fp8_mxfp4", "kv164": "k16_mxfp4"}.get(rows, "fp8"))


def batched_quant_leg(bat, lps, plans, toks, rows="kv8", n_split=0):
    """The FP8 / MXFP4 twin of a batched leg: the same bank contents quantised, the same tables and tokens, straight through the C ABI."""
    from easykv_amd import KVBankBatch
    B = bat.n_seq
    batq = KVBankBatch(B, lps, HQ, H, D, cap=BUDGET + 1 + 63)
    _quantised_copy(bat.bank, lambda: batq.bank, rows)
    qs, ks, vs = toks
    out = torch.empty(B, HQ, 1, D, dtype=torch.float16, device=batq.device)
    ids = torch.empty(B, H, 1, dtype=torch.int32, device=batq.device)
    tables = [batq.make_table(plans, l, n_split=n_split)[:2] for l in range(lps)]
    b = batq.bank
    ws = b._workspace(max(batq.workspace_bytes(st, tb) for st, tb in tables))
    assert batq.step_info(plans, 0, n_split=n_split) == bat.step_info(plans, 0, n_split=n_split)      # planned as the 16-bit batched call of the same table
    call, desc = getattr(batq.lib, f"ekv_{rows}_batch_step_attend"), b._desc

    def rawq(i):
        j = i % qs.shape[0]
        for l, (st, tb) in enumerate(tables):
            rc = call(C.byref(b._bank), C.byref(st), b._dt, C.byref(desc), tb, B, qs[j, l].data_ptr(), ks[j, l].data_ptr(),
                      vs[j, l].data_ptr(), out.data_ptr(), ids.data_ptr(), ws.data_ptr(), ws.numel(), b._stream())
            assert rc == 0, rc
    return rawq


def batched_legs(B, lps, lens, g, quant=(), n_split=0):
    """-> (forward through the C ABI, forward through the engine, plan info, one twin per row kind in `quant`) of the batched call over B
    sequences at `lens` (rows before the token)."""
    from easykv_amd import KVBankBatch
    bat = KVBankBatch(B, lps, HQ, H, D, cap=BUDGET + 1 + 63)
    _fill(bat.bank, [s * lps + l for s in range(B) for l in range(lps)], [lens[s] for s in range(B) for _ in range(lps)], g)
    plans = [_plan(n) for n in lens]
    qs, ks, vs = _tokens(B, lps, g, bat.device)
    out = torch.empty(B, HQ, 1, D, dtype=torch.float16, device=bat.device)
    ids = torch.empty(B, H, 1, dtype=torch.int32, device=bat.device)
    tables = [bat.make_table(plans, l, n_split=n_split)[:2] for l in range(lps)]      # steady state: every entry evicts, the table never changes
    b = bat.bank
    ws = b._workspace(max(bat.lib.ekv_batch_workspace_bytes(C.byref(b._bank), C.byref(st), b._dt, tb, B) for st, tb in tables))
    info = bat.step_info(plans, 0, n_split=n_split)

    def raw(i):
        j = i % qs.shape[0]
        for l, (st, tb) in enumerate(tables):
            rc = bat.lib.ekv_batch_step_attend(C.byref(b._bank), C.byref(st), b._dt, tb, B, qs[j, l].data_ptr(), ks[j, l].data_ptr(), vs[j, l].data_ptr(),
                                               out.data_ptr(), ids.data_ptr(), ws.data_ptr(), ws.numel(), b._stream())
            assert rc == 0, rc

    def engine(i):
        j = i % qs.shape[0]
        for l in range(lps):
            bat.attend(plans, qs[j, l], ks[j, l], vs[j, l], l, out=out, evict_ids=ids)
    # (the twins are built before any leg has stepped the 16-bit bank)
    return (raw, engine, info) + tuple(batched_quant_leg(bat, lps, plans, (qs, ks, vs), rows, n_split) for rows in quant)


def solo_legs(B, lps, g, quant=(), only_quant=False):
    from easykv_amd import KVBank
    n = BUDGET
    plan = _plan(n)
    whole = None if only_quant else KVBank(B * lps, HQ, H, D, cap=n + 1 + 63)      # (only_quant: the 16-bit solo legs are not run)
    if not only_quant:
        _fill(whole, range(B * lps), [n] * (B * lps), g)
    defer = KVBank(B * lps, HQ, H, D, cap=n + 1 + 63)
    _fill(defer, range(B * lps), [n] * (B * lps), g)
    qs, ks, vs = _tokens(B, lps, g, defer.device)
    out = torch.empty(1, HQ, 1, D, dtype=torch.float16, device=defer.device)
    ids = torch.empty(1, H, 1, dtype=torch.int32, device=defer.device)

    def f_whole(i):
        j = i % qs.shape[0]
        for l in range(lps):
            for s in range(B):
                whole.attend(plan, qs[j, l, s:s + 1], ks[j, l, s:s + 1], vs[j, l, s:s + 1], layer_begin=s * lps + l, out=out, evict_ids=ids)

    def f_defer(i):
        j = i % qs.shape[0]
        for l in range(lps):
            for s in range(B):
                defer.attend(plan, qs[j, l, s:s + 1], ks[j, l, s:s + 1], vs[j, l, s:s + 1], layer_begin=s * lps + l, defer=True, out=out)
        defer.flush()
    def deferred_twin(rows):
        bank = _quantised_copy(defer, lambda: KVBank(B * lps, HQ, H, D, cap=n + 1 + 63), rows)

        def f_deferq(i):
            j = i % qs.shape[0]
            for l in range(lps):
                for s in range(B):
                    bank.attend(plan, qs[j, l, s:s + 1], ks[j, l, s:s + 1], vs[j, l, s:s + 1], layer_begin=s * lps + l, defer=True, out=out)
            bank.flush()
        return f_deferq
    return (f_whole, f_defer) + tuple(deferred_twin(rows) for rows in quant)


def uniform_legs(B, lps, g):
    """The existing multi-layer step over B contiguous layers ([layer][sequence] layout), ordered and slot-indexed score rows."""
    from easykv_amd import KVBank, _lib
    n = BUDGET
    plan = _plan(n)
    legs = {}
    for name, slot in (("uniform_ordered", False), ("uniform_slot", True)):
        bank = KVBank(B * lps, HQ, H, D, cap=n + 1 + 63)
        bank.use_slot_rows = slot
        _fill(bank, range(B * lps), [n] * (B * lps), g)
        if slot and not bank.step_plan(plan, 1, 0, B)[1]:
            continue      # (the layout is the one-launch step's: launches the planner splits stay ordered)
        qs, ks, vs = _tokens(B, lps, g, bank.device)
        out = torch.empty(B, HQ, 1, D, dtype=torch.float16, device=bank.device)
        ids = torch.empty(B, H, 1, dtype=torch.int32, device=bank.device)

        def fwd(i, bank=bank, qs=qs, ks=ks, vs=vs, out=out, ids=ids):
            j = i % qs.shape[0]
            for l in range(lps):
                bank.attend(plan, qs[j, l], ks[j, l], vs[j, l], layer_begin=l * B, out=out, evict_ids=ids)
        legs[name] = fwd
    # the batched call over the same [layer][sequence] layout (straight through the C ABI, table prebuilt)
    bank = KVBank(B * lps, HQ, H, D, cap=n + 1 + 63)
    _fill(bank, range(B * lps), [n] * (B * lps), g)
    qs, ks, vs = _tokens(B, lps, g, bank.device)
    out = torch.empty(B, HQ, 1, D, dtype=torch.float16, device=bank.device)
    ids = torch.empty(B, H, 1, dtype=torch.int32, device=bank.device)
    st = bank.make_step(plan, 1, 0, B)
    tables = []
    for l in range(lps):
        tb = (_lib.Seq * B)()
        for s, e in enumerate(tb):
            e.layer, e.n_slots, e.score_off, e.n_evict, e.phys_extent = l * B + s, st.n_slots, st.score_off, st.n_evict, st.phys_extent
            e.win_lo, e.win_tail, e.roco_k1, e.range_start = st.win_lo, st.win_tail, st.roco_k1, st.range_start
        tables.append(tb)
    ws = bank._workspace(bank.lib.ekv_batch_workspace_bytes(C.byref(bank._bank), C.byref(st), bank._dt, tables[0], B))

    def contig(i):
        j = i % qs.shape[0]
        for l, tb in enumerate(tables):
            rc = bank.lib.ekv_batch_step_attend(C.byref(bank._bank), C.byref(st), bank._dt, tb, B, qs[j, l].data_ptr(), ks[j, l].data_ptr(),
                                                vs[j, l].data_ptr(), out.data_ptr(), ids.data_ptr(), ws.data_ptr(), ws.numel(), bank._stream())
            assert rc == 0, rc
    legs["batched_contig"] = contig
    return legs


PAIR_BYTES = {"kv16": 4 * D, "kv8": 2 * D + 8, "kv4": D + D // 16, "kv6": 3 * D // 2 + D // 16,
              "kv84": 3 * D // 2 + 4 + D // 32, "kv164": 2 * D + D // 2 + D // 32}      # one K+V row pair: 16-bit / FP8 codes + two fp32 scales / MXFP4 codes + exponents


def _rows_of(leg):
    return next((r for r in ("kv164", "kv84", "kv8", "kv4", "kv6") if r in leg.split("_")), "kv16")


def bytes_per_call(lens, rows="kv16"):
    """Algorithmic bytes of one per-layer call over sequences of `lens` rows, their K/V rows held as `rows`."""
    total = 0
    for n in lens:
        b = algorithmic_bytes(H, HQ, D, n + 1, 1, 3)
        total += b["total"] - H * (n + 1) * PAIR_BYTES["kv16"] + H * (n + 1) * PAIR_BYTES[rows]
    return total


def run_batch(B, args):
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(1000 + B)
    lps = 16 if B <= 2 else 8      # layers per sequence: every leg's working set stays far above the 256 MB of the memory-side cache
    rs = torch.Generator().manual_seed(20261016 + B)
    ragged = sorted(int(x) for x in torch.randint(255, BUDGET + 1, (B,), generator=rs))
    ragged[-1] = BUDGET      # (the envelope is the uniform shape)
    mx = "kv164" if args.k16_mxfp4 else "kv84" if args.fp8_mxfp4 else "kv6" if args.mxfp6 else ("kv4" if args.mxfp4 else None)      # the MX format under test: its legs + the yardsticks of the same run
    quant = ("kv8", "kv84", "kv164") if args.k16_mxfp4 else ("kv8", "kv4", "kv6", "kv84") if args.fp8_mxfp4 else ("kv8", "kv4", "kv6") if args.mxfp6 else (("kv8", "kv4") if args.mxfp4 else (("kv8",) if args.kv8 else ()))
    raw, engine, info, *rawq = batched_legs(B, lps, [BUDGET] * B, g, quant)
    fns = {"batched": raw, "batched_engine": engine}
    solo_quant = (mx,) if mx else quant
    fns["solo_whole"], fns["solo_deferred"], *deferq = solo_legs(B, lps, g, solo_quant, only_quant=mx is not None)
    if not mx:
        fns.update(uniform_legs(B, lps, g))
    fns.update({f"batched_{rows}": f for rows, f in zip(quant, rawq)})
    fns.update({f"solo_{rows}_deferred": f for rows, f in zip(solo_quant, deferq)})
    if B > 1:
        fns["ragged"], _, rinfo, *raggedq = batched_legs(B, lps, ragged, g, quant)
        assert rinfo == info, (rinfo, info)      # a ragged table plans as its envelope
        for rows, f in zip(quant, raggedq):
            fns[f"ragged_{rows}"] = f
    if mx:      # the yardsticks of the same run and the three new legs; the other legs: profiles/batch_bench.json, batch_kv8_bench.json
        keep = ("batched", "batched_kv8", "batched_kv4", "batched_kv6", "batched_kv84", "batched_kv164", f"solo_{mx}_deferred", "ragged", "ragged_kv8", "ragged_kv4",
                "ragged_kv6", "ragged_kv84", "ragged_kv164")
        fns = {k: f for k, f in fns.items() if k in keep}
    if args.legs:      # (a kernel trace of two legs: their launches alone)
        fns = {k: f for k, f in fns.items() if k in args.legs.split(",")}
    t = _interleave(fns, args.reps, args.tokens, args.warm)
    del fns
    gc.collect()
    torch.cuda.empty_cache()
    res = {"layers_per_sequence": lps, "plan": info}
    ub = bytes_per_call([BUDGET] * B)
    for k, v in t.items():
        us = v["us"] / lps      # per per-layer call (solo legs: B calls; solo_deferred: + its share of the flush)
        nb = bytes_per_call(ragged if k.startswith("ragged") else [BUDGET] * B, _rows_of(k))
        res[k] = dict(us_per_layer_call=round(us, 2), run_to_run_spread=v["spread"], path_tokens_per_s=round(B / (us * 32 * 1e-6), 1),
                      bytes_per_layer_call=nb, gb_per_s=round(nb / (us * 1e-6) / 1e9, 1), frac_of_hbm_peak=round(nb / (us * 1e-6) / 1e9 / HBM_PEAK_GBS, 4))
    if args.legs:
        return res
    us = lambda k: res[k]["us_per_layer_call"]
    if "uniform_ordered" in res:
        res["ratio_batched_over_uniform_ordered"] = round(us("batched") / us("uniform_ordered"), 4)
        res["ratio_batched_contig_over_uniform_ordered"] = round(us("batched_contig") / us("uniform_ordered"), 4)
        res["ratio_batched_over_solo_whole"] = round(us("batched") / us("solo_whole"), 4)
        res["ratio_batched_over_solo_deferred"] = round(us("batched") / us("solo_deferred"), 4)
    if "uniform_slot" in res:
        res["ratio_uniform_slot_over_uniform_ordered"] = round(us("uniform_slot") / us("uniform_ordered"), 4)
    if "batched_kv8" in res:
        res["ratio_batched_kv8_over_batched"] = round(us("batched_kv8") / us("batched"), 4)
        if "solo_kv8_deferred" in res:
            res["ratio_batched_kv8_over_solo_kv8_deferred"] = round(us("batched_kv8") / us("solo_kv8_deferred"), 4)
        res["byte_ratio_batched_kv8_over_batched"] = round(res["batched_kv8"]["bytes_per_layer_call"] / res["batched"]["bytes_per_layer_call"], 4)
    if "batched_kv4" in res:
        res["ratio_batched_kv4_over_batched"] = round(us("batched_kv4") / us("batched"), 4)
        res["ratio_batched_kv4_over_batched_kv8"] = round(us("batched_kv4") / us("batched_kv8"), 4)
        if "solo_kv4_deferred" in res:
            res["ratio_batched_kv4_over_solo_kv4_deferred"] = round(us("batched_kv4") / us("solo_kv4_deferred"), 4)
        res["byte_ratio_batched_kv4_over_batched"] = round(res["batched_kv4"]["bytes_per_layer_call"] / res["batched"]["bytes_per_layer_call"], 4)
        res["byte_ratio_batched_kv4_over_batched_kv8"] = round(res["batched_kv4"]["bytes_per_layer_call"] / res["batched_kv8"]["bytes_per_layer_call"], 4)
    if "ragged_kv4" in res:
        res["ratio_ragged_kv4_over_ragged"] = round(us("ragged_kv4") / us("ragged"), 4)
        res["ratio_ragged_kv4_over_ragged_kv8"] = round(us("ragged_kv4") / us("ragged_kv8"), 4)
        res["ratio_ragged_kv4_over_batched_kv4_at_envelope"] = round(us("ragged_kv4") / us("batched_kv4"), 4)
    if "batched_kv6" in res:
        for other in ("batched", "batched_kv8", "batched_kv4", "solo_kv6_deferred"):
            if other in res:      # (the solo leg runs only for the format under test)
                res[f"ratio_batched_kv6_over_{other}"] = round(us("batched_kv6") / us(other), 4)
        for other in ("batched", "batched_kv8"):
            res[f"byte_ratio_batched_kv6_over_{other}"] = round(res["batched_kv6"]["bytes_per_layer_call"] / res[other]["bytes_per_layer_call"], 4)
    if "ragged_kv6" in res:
        for other in ("ragged", "ragged_kv8", "ragged_kv4"):
            res[f"ratio_ragged_kv6_over_{other}"] = round(us("ragged_kv6") / us(other), 4)
        res["ratio_ragged_kv6_over_batched_kv6_at_envelope"] = round(us("ragged_kv6") / us("batched_kv6"), 4)
    if "batched_kv164" in res:
        for other in ("batched", "batched_kv8", "batched_kv84", "solo_kv164_deferred"):
            res[f"ratio_batched_kv164_over_{other}"] = round(us("batched_kv164") / us(other), 4)
        for other in ("batched", "batched_kv8"):
            res[f"byte_ratio_batched_kv164_over_{other}"] = round(res["batched_kv164"]["bytes_per_layer_call"] / res[other]["bytes_per_layer_call"], 4)
    if "ragged_kv164" in res:
        for other in ("ragged", "ragged_kv8", "ragged_kv84"):
            res[f"ratio_ragged_kv164_over_{other}"] = round(us("ragged_kv164") / us(other), 4)
        res["ratio_ragged_kv164_over_batched_kv164_at_envelope"] = round(us("ragged_kv164") / us("batched_kv164"), 4)
    if "batched_kv84" in res:
        for other in ("batched", "batched_kv8", "batched_kv4", "batched_kv6", "solo_kv84_deferred"):
            if other in res:      # (the legs of the run: --k16-mxfp4 has no MXFP4 / MXFP6 leg and no kv84 solo leg)
                res[f"ratio_batched_kv84_over_{other}"] = round(us("batched_kv84") / us(other), 4)
        for other in ("batched", "batched_kv8"):
            res[f"byte_ratio_batched_kv84_over_{other}"] = round(res["batched_kv84"]["bytes_per_layer_call"] / res[other]["bytes_per_layer_call"], 4)
    if "ragged_kv84" in res:
        for other in (o for o in ("ragged", "ragged_kv8", "ragged_kv4", "ragged_kv6") if o in res):
            res[f"ratio_ragged_kv84_over_{other}"] = round(us("ragged_kv84") / us(other), 4)
        res["ratio_ragged_kv84_over_batched_kv84_at_envelope"] = round(us("ragged_kv84") / us("batched_kv84"), 4)
    if "ragged_kv8" in res:
        res["ratio_ragged_kv8_over_ragged"] = round(us("ragged_kv8") / us("ragged"), 4)
        res["ratio_ragged_kv8_over_batched_kv8_at_envelope"] = round(us("ragged_kv8") / us("batched_kv8"), 4)
    if "ragged" in res:
        res["ragged_lengths"] = [n + 1 for n in ragged]
        res["ratio_ragged_over_batched_at_envelope"] = round(us("ragged") / us("batched"), 4)
        res["live_bytes_over_envelope_bytes"] = round(bytes_per_call(ragged) / ub, 4)
    return res


def run_gqa4(B, args):
    """The GQA x 4 table (Hq 32 over H 8): `batched` and `batched_kv4` at the uniform length, as planned, with a forced key-range split
    and forced into one launch — the one-launch GQA x 4 kv4 build spills registers, the split kernel's does not."""
    global HQ, H
    dev = torch.device("cuda")
    keep = (HQ, H)
    HQ, H = 32, 8
    try:
        lps = 16
        fns, plans = {}, {}
        for name, n_split in (("planned", 0), ("split8", 8), ("one_launch", 1)):
            g = torch.Generator(device=dev).manual_seed(3000 + B)      # (the same rows, maps and tokens under every plan)
            raw, _, info, raw4 = batched_legs(B, lps, [BUDGET] * B, g, ("kv4",), n_split)
            fns[f"batched_{name}"], fns[f"batched_kv4_{name}"], plans[name] = raw, raw4, info
        t = _interleave(fns, args.reps, args.tokens, args.warm)
        del fns
        gc.collect()
        torch.cuda.empty_cache()
        res = {"layers_per_sequence": lps, "plans": plans}
        for k, v in t.items():
            us = v["us"] / lps
            nb = bytes_per_call([BUDGET] * B, _rows_of(k))
            res[k] = dict(us_per_layer_call=round(us, 2), run_to_run_spread=v["spread"], bytes_per_layer_call=nb, gb_per_s=round(nb / (us * 1e-6) / 1e9, 1))
        for name in plans:
            res[f"ratio_batched_kv4_over_batched_{name}"] = round(res[f"batched_kv4_{name}"]["us_per_layer_call"] / res[f"batched_{name}"]["us_per_layer_call"], 4)
        res["byte_ratio_batched_kv4_over_batched"] = round(res["batched_kv4_planned"]["bytes_per_layer_call"] / res["batched_planned"]["bytes_per_layer_call"], 4)
        return res
    finally:
        HQ, H = keep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--tokens", type=int, default=24)
    ap.add_argument("--warm", type=int, default=20)
    ap.add_argument("--batches", default="1,2,4,8,16,32")
    ap.add_argument("--legs", default=None, help="comma-separated legs to run alone, e.g. batched,uniform_ordered (no ratios; for a kernel trace)")
    ap.add_argument("--kv8", action="store_true", help="add the FP8 legs batched_kv8, solo_kv8_deferred, ragged_kv8 (default --out: profiles/batch_kv8_bench.json)")
    ap.add_argument("--mxfp4", action="store_true", help="the MXFP4 legs batched_kv4, solo_kv4_deferred, ragged_kv4 next to batched, batched_kv8, ragged, "
                    "ragged_kv8, and the GQA x 4 table (default --out: profiles/batch_kv4_bench.json)")
    ap.add_argument("--mxfp6", action="store_true", help="the MXFP6 legs batched_kv6, solo_kv6_deferred, ragged_kv6 next to the 16-bit, FP8 and MXFP4 "
                    "batched / ragged legs of the same run (default --out: profiles/batch_kv6_bench.json)")
    ap.add_argument("--fp8-mxfp4", action="store_true", help="the FP8-key / MXFP4-value legs batched_kv84, solo_kv84_deferred, ragged_kv84 next to the 16-bit, "
                    "FP8, MXFP4 and MXFP6 batched / ragged legs of the same run (default --out: profiles/batch_kv84_bench.json)")
    ap.add_argument("--k16-mxfp4", action="store_true", help="the 16-bit-key / MXFP4-value legs batched_kv164, solo_kv164_deferred, ragged_kv164 next to the "
                    "16-bit, FP8 and FP8-key / MXFP4-value batched / ragged legs of the same run (default --out: profiles/batch_kv164_bench.json)")
    ap.add_argument("--gqa4-batches", default="8,32", help="--mxfp4: batch sizes of the GQA x 4 table ('' = none)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    args.out = args.out or os.path.join(ROOT, "profiles", "batch_kv164_bench.json" if args.k16_mxfp4 else "batch_kv84_bench.json" if args.fp8_mxfp4 else "batch_kv6_bench.json" if args.mxfp6 else "batch_kv4_bench.json" if args.mxfp4 else ("batch_kv8_bench.json" if args.kv8 else "batch_bench.json"))
    torch.cuda.set_device(0)
    res = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "tokens_per_rep": args.tokens, "warm_tokens": args.warm,
           "hbm_peak_gb_per_s": HBM_PEAK_GBS,
           "shape": "Hq = H = 32, D = 128, budget 2048 (T = 2049), roco, every step evicting, scattered slot maps, warm score state; "
                    "per-layer calls; path tokens/s = B / (32 layers x us per per-layer call)"}
    for B in (int(x) for x in args.batches.split(",")):
        res[f"B{B}"] = run_batch(B, args)
        print(f"B{B}", json.dumps(res[f"B{B}"]), flush=True)
    if args.mxfp4 and not args.legs and args.gqa4_batches:
        res["gqa4"] = {"shape": "Hq = 32 over H = 8 (GQA x 4), D = 128, otherwise as above; planned / split8 (n_split = 8) / one_launch (n_split = 1)"}
        for B in (int(x) for x in args.gqa4_batches.split(",")):
            res["gqa4"][f"B{B}"] = run_gqa4(B, args)
            print(f"gqa4 B{B}", json.dumps(res["gqa4"][f"B{B}"]), flush=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
