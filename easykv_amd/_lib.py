"""ctypes binding of the C ABI in include/easykv_hip.h.

The product path has NO CPU fallback: if the shared library is missing or a symbol is not
exported this module raises, loudly, at import of the engine.
"""
from __future__ import annotations

import ctypes as C
import os

import torch

from ._build import LIB

# policy codes (include/easykv_hip.h)
POLICY_NONE, POLICY_H2O_HEAD, POLICY_ROCO, POLICY_TOVA, POLICY_RANGE = 0, 1, 2, 3, 4
PHASE_SLOT_TAIL_OK = 32
PHASE_SLOT_ROWS = 16      # ekv_step.phases bit: the layers' score rows are in the slot-indexed layout (include/easykv_hip.h)
POLICY_CODES = {"full": POLICY_NONE, "h2o_head": POLICY_H2O_HEAD, "roco": POLICY_ROCO, "tova": POLICY_TOVA,
                "recency": POLICY_RANGE, "random": POLICY_RANGE}

# element type of a step's 16-bit tensors (the bank's k / v, q, k_new, v_new, out): the *_typed calls
DTYPE_F16, DTYPE_BF16 = 0, 1
DTYPE_CODES = {torch.float16: DTYPE_F16, torch.bfloat16: DTYPE_BF16}

MAX_SEQS = 64      # EKV_MAX_SEQS: entries of one batched decode step
DTYPE_F32 = 2      # ekv_kv8_dequantize's / ekv_kv4_dequantize's out_dtype only
STEP_CALLS = ("step_check", "step_info", "workspace_bytes", "step_attend")


def step_call_name(rows, batch, what):
    """Name of the call `what` (one of STEP_CALLS) of the step family for a bank's row format — None (16-bit rows: the _typed calls),
    "kv8", "kv4", "kv6", "kv84" or "kv164" — and a uniform step or a batched one (include/easykv_hip.h)."""
    if rows is None and not batch:
        return "ekv_" + what + "_typed"
    return "ekv_" + (rows + "_" if rows else "") + ("batch_" if batch else "") + what


# every function of include/easykv_hip.h (tests/test_host_cpu.py holds the tuple to the header's declarations)
EXPORTS = ("ekv_abi_version", "ekv_strerror", "ekv_workspace_bytes", "ekv_step_plan", "ekv_bank_reset", "ekv_state_init",
           "ekv_step_attend", "ekv_gather_ordered", "ekv_scatter_rows", "ekv_compact_inplace", "ekv_step_check", "ekv_step_info",
           "ekv_rows_to_slots", "ekv_rows_to_order", "ekv_kv8_quantize", "ekv_kv8_dequantize", "ekv_kv4_quantize", "ekv_kv4_dequantize",
           "ekv_kv6_quantize", "ekv_kv6_dequantize", "ekv_set_resident_bytes", "ekv_step_resident_rows", "ekv_kv84_quantize", "ekv_kv84_dequantize",
           "ekv_kv164_quantize", "ekv_kv164_dequantize") + tuple(
               step_call_name(rows, batch, what) for rows in (None, "kv8", "kv4", "kv6", "kv84", "kv164") for batch in (False, True) for what in STEP_CALLS)
# the long-row family (include/easykv_hip.h, "long score rows"): the signatures of the _typed calls; 16-bit rows, one sequence
LONG_CALLS = {what: "ekv_long_" + what for what in STEP_CALLS}
EXPORTS += tuple(LONG_CALLS[what] for what in STEP_CALLS)
LONG_INFO_N = 12      # EKV_LONG_INFO_N: [10] the step ends in the long-row scorer, [11] column tiles per head of its sweep
# the soft-capped family (include/easykv_hip.h, "soft-capped logits"): the _typed calls with a float cap behind the dtype; 16-bit rows, one sequence
CAP_CALLS = {what: "ekv_cap_" + what for what in STEP_CALLS}
EXPORTS += tuple(CAP_CALLS[what] for what in STEP_CALLS) + ("ekv_softcap_eval",)
# the sink family (include/easykv_hip.h, "attention sinks"): the _typed calls with the device pointer of the sinks behind the dtype; 16-bit rows, one sequence
SINK_CALLS = {what: "ekv_sink_" + what for what in STEP_CALLS}
EXPORTS += tuple(SINK_CALLS[what] for what in STEP_CALLS)
# the window family (include/easykv_hip.h, "sliding windows"): the _typed calls with an ekv_win struct behind the dtype; 16-bit rows, one sequence
WIN_CALLS = {what: "ekv_win_" + what for what in STEP_CALLS}
EXPORTS += tuple(WIN_CALLS[what] for what in STEP_CALLS)
# the pooled family (include/easykv_hip.h, "pooled selection"): the _typed calls with an ekv_pool struct behind the dtype; 16-bit rows, one sequence
POOL_CALLS = {what: "ekv_pool_" + what for what in STEP_CALLS}
EXPORTS += tuple(POOL_CALLS[what] for what in STEP_CALLS)
POOL_OPS = {"max": 0, "avg": 1}      # EKV_POOL_MAX, EKV_POOL_AVG
# the adaptive family (include/easykv_hip.h, "adaptive head budgets"): the _typed calls with an ekv_ada struct behind the dtype; 16-bit rows, one sequence
ADA_CALLS = {what: "ekv_ada_" + what for what in STEP_CALLS}
EXPORTS += tuple(ADA_CALLS[what] for what in STEP_CALLS)
# the heads family (include/easykv_hip.h, "heads"): the _typed calls with an ekv_heads struct behind the dtype and no rope tables; 16-bit rows
HEADS_CALLS = {what: "ekv_heads_" + what for what in STEP_CALLS}
EXPORTS += tuple(HEADS_CALLS[what] for what in STEP_CALLS)


class Bank(C.Structure):
    _fields_ = [("k", C.c_void_p), ("v", C.c_void_p), ("slot_of_pos", C.c_void_p),
                ("score_sum", C.c_void_p), ("score_sq", C.c_void_p), ("score_cnt", C.c_void_p),
                ("n_layers", C.c_int32), ("n_q_heads", C.c_int32), ("n_kv_heads", C.c_int32),
                ("head_dim", C.c_int32), ("cap", C.c_int32), ("arrive", C.c_void_p), ("birth", C.c_void_p), ("slot_state", C.c_void_p)]


class Kv8(C.Structure):
    """ekv_kv8: the FP8 code planes and fp32 row scales that stand for a bank's K/V rows (include/easykv_hip.h, "kv8")."""
    _fields_ = [("k_codes", C.c_void_p), ("v_codes", C.c_void_p), ("k_scale", C.c_void_p), ("v_scale", C.c_void_p)]


class Kv4(C.Structure):
    """ekv_kv4: the MXFP4 code planes and E8M0 block exponents that stand for a bank's K/V rows (include/easykv_hip.h, "kv4")."""
    _fields_ = [("k_codes", C.c_void_p), ("v_codes", C.c_void_p), ("k_exp", C.c_void_p), ("v_exp", C.c_void_p)]


class Kv6(C.Structure):
    """ekv_kv6: the MXFP6 code planes and E8M0 block exponents that stand for a bank's K/V rows (include/easykv_hip.h, "kv6")."""
    _fields_ = [("k_codes", C.c_void_p), ("v_codes", C.c_void_p), ("k_exp", C.c_void_p), ("v_exp", C.c_void_p)]


class Kv84(C.Structure):
    """ekv_kv84: FP8 key codes with fp32 row scales and MXFP4 value codes with E8M0 block exponents (include/easykv_hip.h, "kv84")."""
    _fields_ = [("k_codes", C.c_void_p), ("v_codes", C.c_void_p), ("k_scale", C.c_void_p), ("v_exp", C.c_void_p)]


class Kv164(C.Structure):
    """ekv_kv164: MXFP4 value codes with E8M0 block exponents; the keys are the bank's 16-bit rows (include/easykv_hip.h, "kv164")."""
    _fields_ = [("v_codes", C.c_void_p), ("v_exp", C.c_void_p)]


class Win(C.Structure):
    """ekv_win: token positions of the physical rows, the layers' windows (device, and a host copy the library can check), the sinks or
    NULL, and the token position of the step's query (include/easykv_hip.h, "sliding windows")."""
    _fields_ = [("tok_pos", C.c_void_p), ("windows", C.c_void_p), ("windows_host", C.POINTER(C.c_int32)), ("s_aux", C.c_void_p), ("q_pos0", C.c_int32)]


class Pool(C.Structure):
    """ekv_pool: radius (kernel size 2 * radius + 1) and op (POOL_OPS) of a pooled selection (include/easykv_hip.h, "pooled selection")."""
    _fields_ = [("radius", C.c_int32), ("op", C.c_int32)]


class Ada(C.Structure):
    """ekv_ada: pooling (radius >= 0, op) and the bounds of a head's victims of an adaptive step; n_evict_out: device int32 [layer_count][H]
    (include/easykv_hip.h, "adaptive head budgets")."""
    _fields_ = [("radius", C.c_int32), ("op", C.c_int32), ("evict_min", C.c_int32), ("evict_max", C.c_int32), ("n_evict_out", C.c_void_p)]


class Heads(C.Structure):
    """ekv_heads: the row counts of a decode step over KV heads of different lengths — rows: device int32 [n_layers][H], rows_host: a host
    copy of the same (every check and plan reads this one), grow: rows every head has gained since (include/easykv_hip.h, "heads")."""
    _fields_ = [("rows", C.c_void_p), ("rows_host", C.c_void_p), ("grow", C.c_int32)]


class Step(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "layer_begin", "layer_count", "q_len", "n_slots", "score_off", "policy", "accumulate", "n_evict",
        "win_lo", "win_tail", "roco_k1", "roco_tail", "range_start", "tova_head_mean", "causal", "rope_on_read",
        "n_split", "phases")] + [(n, C.c_float) for n in ("count_add", "count_tail_step", "sm_div")] + [(n, C.c_int32) for n in (
        "two_pass", "phys_extent", "defer_layers", "defer_index",
        "q_token_stride", "q_head_stride", "kv_token_stride", "kv_head_stride", "out_token_stride", "out_head_stride")]


class Seq(C.Structure):
    """ekv_seq: one sequence of a batched decode step (include/easykv_hip.h)."""
    _fields_ = [(n, C.c_int32) for n in ("layer", "n_slots", "score_off", "n_evict", "win_lo", "win_tail", "roco_k1", "range_start",
                                         "phys_extent")]


class EkvError(RuntimeError):
    pass


_lib = None


def load():
    """Load (once) and type the shared library.  Raises if it was not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB):
        raise EkvError(f"{LIB} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                       "(hipcc --offload-arch=gfx950).  There is no CPU fallback for the product path.")
    lib = C.CDLL(LIB)
    for name in EXPORTS:
        if not hasattr(lib, name):
            raise EkvError(f"{LIB} does not export {name}")
    vp, i32 = C.c_void_p, C.c_int32
    lib.ekv_abi_version.restype = C.c_int
    lib.ekv_strerror.restype = C.c_char_p
    lib.ekv_strerror.argtypes = [C.c_int]
    lib.ekv_workspace_bytes.restype = C.c_size_t
    lib.ekv_workspace_bytes.argtypes = [C.POINTER(Bank), C.POINTER(Step)]
    lib.ekv_step_plan.argtypes = [C.POINTER(Bank), C.POINTER(Step), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    lib.ekv_bank_reset.argtypes = [C.POINTER(Bank), vp]
    lib.ekv_state_init.argtypes = [C.POINTER(Bank), i32, i32, i32, i32, i32, vp]
    lib.ekv_step_attend.argtypes = [C.POINTER(Bank), C.POINTER(Step), vp, vp, vp, vp, vp, vp, vp, vp, C.c_size_t, vp]
    lib.ekv_gather_ordered.argtypes = [C.POINTER(Bank), i32, i32, i32, vp, vp, vp]
    lib.ekv_scatter_rows.argtypes = [C.POINTER(Bank), i32, i32, i32, i32, vp, vp, vp]
    lib.ekv_compact_inplace.argtypes = [C.POINTER(Bank), i32, i32, i32, i32, vp, vp]
    lib.ekv_step_check.argtypes = [C.POINTER(Bank), C.POINTER(Step)]
    lib.ekv_step_info.argtypes = [C.POINTER(Bank), C.POINTER(Step), C.POINTER(C.c_int32), C.c_int32]
    lib.ekv_rows_to_slots.argtypes = [C.POINTER(Bank), i32, i32, i32, vp]
    lib.ekv_rows_to_order.argtypes = [C.POINTER(Bank), i32, i32, i32, vp]
    lib.ekv_set_resident_bytes.argtypes = [C.c_int64]
    lib.ekv_step_resident_rows.argtypes = [C.POINTER(Bank), C.POINTER(Step), i32]
    # the step family: (bank, step, dtype[, descriptor][, table, entries]) + what the call itself takes
    tails = {"step_check": [], "workspace_bytes": [], "step_info": [C.POINTER(C.c_int32), C.c_int32]}
    for rows, desc in ((None, None), ("kv8", Kv8), ("kv4", Kv4), ("kv6", Kv6), ("kv84", Kv84), ("kv164", Kv164)):
        for batch in (False, True):
            head = [C.POINTER(Bank), C.POINTER(Step), i32] + ([C.POINTER(desc)] if desc else []) + ([C.POINTER(Seq), i32] if batch else [])
            tails["step_attend"] = [vp] * (6 if batch else 8) + [C.c_size_t, vp]      # (a batch has no rope tables)
            for what in STEP_CALLS:
                getattr(lib, step_call_name(rows, batch, what)).argtypes = head + tails[what]
        if rows is None:      # (the long family: the uniform 16-bit signatures)
            tails["step_attend"] = [vp] * 8 + [C.c_size_t, vp]
            for what in STEP_CALLS:
                getattr(lib, LONG_CALLS[what]).argtypes = [C.POINTER(Bank), C.POINTER(Step), i32] + tails[what]
                getattr(lib, CAP_CALLS[what]).argtypes = [C.POINTER(Bank), C.POINTER(Step), i32, C.c_float] + tails[what]
                getattr(lib, SINK_CALLS[what]).argtypes = [C.POINTER(Bank), C.POINTER(Step), i32, vp] + tails[what]
                getattr(lib, WIN_CALLS[what]).argtypes = [C.POINTER(Bank), C.POINTER(Step), i32, C.POINTER(Win)] + tails[what]
                getattr(lib, POOL_CALLS[what]).argtypes = [C.POINTER(Bank), C.POINTER(Step), i32, C.POINTER(Pool)] + tails[what]
                getattr(lib, ADA_CALLS[what]).argtypes = [C.POINTER(Bank), C.POINTER(Step), i32, C.POINTER(Ada)] + tails[what]
            tails["step_attend"] = [vp] * 6 + [C.c_size_t, vp]      # (the heads family: no rope tables)
            for what in STEP_CALLS:
                getattr(lib, HEADS_CALLS[what]).argtypes = [C.POINTER(Bank), C.POINTER(Step), i32, C.POINTER(Heads)] + tails[what]
        if desc:
            getattr(lib, f"ekv_{rows}_quantize").argtypes = [C.POINTER(Bank), C.POINTER(desc), i32, i32, i32, i32, vp]
            getattr(lib, f"ekv_{rows}_dequantize").argtypes = [C.POINTER(Bank), C.POINTER(desc), i32, i32, i32, i32, vp, vp, vp]
    lib.ekv_softcap_eval.argtypes = [vp, C.c_int64, C.c_float, C.c_float, vp, vp]
    lib.ekv_kv164_dequantize.argtypes = [C.POINTER(Bank), C.POINTER(Kv164), i32, i32, i32, i32, vp, vp]      # (V only: one output)
    for name in EXPORTS:
        if name != "ekv_strerror":
            getattr(lib, name).restype = C.c_size_t if "workspace_bytes" in name else C.c_int
    if lib.ekv_abi_version() != 8:
        raise EkvError("ABI version mismatch")
    _lib = lib
    return lib


def set_resident_bytes(nbytes):
    """Byte budget of the resident rows of one-launch decode steps (include/easykv_hip.h, "resident rows") for this process; None or
    a negative value: the library's default (EKV_RESIDENT_MB in the environment, else the compile-time value).  Always handed to the
    library (the value is a process global there: whoever calls the C setter directly is overruled by the next step of a bank)."""
    load().ekv_set_resident_bytes(-1 if nbytes is None or nbytes < 0 else int(nbytes))


def check(code: int, what: str):
    if code != 0:
        msg = load().ekv_strerror(code).decode()
        if code == -1:
            raise ValueError(f"{what}: {msg}")
        raise EkvError(f"{what}: {msg} ({code})")
