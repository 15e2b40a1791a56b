/*
 * easykv_hip.h — C ABI of the MI355X-native budgeted-KV-cache attention path.
 *
 * Drop-in boundary for the ONE hot path of DRSY/EasyKV (reference paths relative to
 * /root/reference):  per layer and per model forward the reference does, in Python,
 *
 *   patched attention forward      easykv/llama_patch.py:198-222, :310-327   (mistral_patch.py:144-169, :225-241)
 *   GQA fold of the probabilities  easykv/easykv.py:188-196
 *   score accumulation             easykv/easykv.py:287-300, :443-457, :693-707
 *   victim selection               easykv/easykv.py:310-347, :462-493, :711-742
 *   K/V compaction                 easykv/easykv.py:56-82, :105-112
 *   score-state compaction         easykv/easykv.py:315-333, :465-490
 *
 * The reference has no FFI of its own (it is 100 % Python); the entry points below are what a
 * ctypes binding for this path binds (see INTEGRATION.md for the reference-side stub).  Plain
 * pointers and sizes only, no torch types.  Every launch is asynchronous on the `stream`
 * argument (a hipStream_t passed as void*), re-entrant per stream, and keeps no global state.
 * Return value: 0 on success, a negative EKV_E_* code otherwise (ekv_strerror() describes it).
 *
 * Memory model ("bank" = the layers resident on this GPU, all device memory, caller-owned):
 *
 *   k, v          16-bit [n_layers][n_kv_heads][cap][head_dim]  physical rows ("slots"): fp16, or bf16 through the _typed calls
 *   slot_of_pos   int32 [n_layers][n_kv_heads][cap]             permutation: logical position -> row.
 *                       positions [0, n_slots) are live, in the reference's birth order;
 *                       positions [n_slots, cap) hold the free rows.
 *   score_sum     fp32  [n_layers][n_kv_heads][cap]             S  (sum p),      index j <-> position score_off + j
 *   score_sq      fp32  [n_layers][n_kv_heads][cap]             Q  (sum p^2)     (roco only)
 *   score_cnt     fp32  [n_layers][n_kv_heads][cap]             C  (#queries)    (roco only)
 *   arrive        u32   [n_layers][n_kv_heads]                  optional arrival counters (see ekv_bank)
 *
 * Eviction never moves K/V rows: the victim's row is recycled for the next token and only the
 * 4-byte slot map is compacted (order-preserving, exactly the reference's list semantics).
 * ekv_gather_ordered() materialises the ordered [T][D] view the HF legacy-tuple boundary needs;
 * ekv_compact_inplace() is the reference-shaped physical compaction for banks kept in identity
 * layout.
 */
#ifndef EASYKV_HIP_H
#define EASYKV_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EKV_ABI_VERSION 8

/* kv_policy strings of the reference -> codes (easykv/easykv.py:288-300, :310-362) */
enum {
  EKV_POLICY_NONE = 0,     /* 'full' or any unknown string: attention only                    */
  EKV_POLICY_H2O_HEAD = 1, /* 'h2o_head'                                                      */
  EKV_POLICY_ROCO = 2,     /* 'roco'                                                          */
  EKV_POLICY_TOVA = 3,     /* 'tova'                                                          */
  EKV_POLICY_RANGE = 4     /* 'recency' / 'random': host-chosen contiguous range, all heads   */
};

enum {
  EKV_OK = 0,
  EKV_E_ARG = -1,          /* inconsistent sizes / null pointer          */
  EKV_E_UNSUPPORTED = -2,  /* head_dim / group size / width not built    */
  /* head_dim: 32 / 64 / 96 / 128 / 256.  head_dim 256 (16-bit rows, fp16 or bf16): every step with plain keys — decode steps of any GQA
   * factor, single and batched, chunk steps of GQA factors up to 32, the long family; rope_on_read and every quantised row format
   * (ekv_kv8_* ... ekv_kv164_*) answer EKV_E_UNSUPPORTED at that head_dim, before anything is launched. */
  EKV_E_WORKSPACE = -3,    /* workspace too small                        */
  EKV_E_LAUNCH = -4        /* hipLaunch failure (hipGetLastError)        */
};

/* Element type of the 16-bit tensors of a step: the bank's k / v, q, k_new, v_new and out alike (ABI 8, additive).  The untyped
 * calls are the EKV_DTYPE_F16 calls of the same code; any other value returns EKV_E_ARG.  A bf16 step is planned exactly as the
 * fp16 step (tiling, launches, workspace) and runs the bf16 builds of the same kernels: logits, softmax statistics, scores and
 * selection stay fp32, P is rounded to bf16 where it feeds a matrix-core product, and the output is rounded once from fp32.  Steps
 * with rope_on_read have no bf16 build (EKV_E_UNSUPPORTED, no launches).  The row moves (ekv_gather_ordered, ekv_scatter_rows,
 * ekv_compact_inplace) and the slot-map / score-row calls (ekv_rows_to_slots, ekv_rows_to_order, ekv_bank_reset, ekv_state_init)
 * never read an element's value and serve bf16 banks as they are. */
enum { EKV_DTYPE_F16 = 0, EKV_DTYPE_BF16 = 1 };

typedef struct ekv_bank {
  void *k, *v;
  int32_t *slot_of_pos;
  float *score_sum, *score_sq, *score_cnt;
  int32_t n_layers, n_q_heads, n_kv_heads, head_dim, cap;
  uint32_t *arrive; /* optional (ABI 3), uint32 [n_layers][n_kv_heads], zeroed by ekv_bank_reset and left zero by every call:
                       arrival counters of the split decode path.  With it the key-range partials of a head are folded inside the
                       attention kernel by the last split to arrive (no fold launch); NULL = separate fold kernel.            */
  int32_t *birth;   /* optional (ABI 6), int32 [2][n_layers][n_kv_heads][cap] (order keys; the parked tail of the count rows) + */
  float *slot_state;/* float [n_layers][n_kv_heads][4]: the slot-indexed layout of the score rows (EKV_PHASE_SLOT_ROWS); NULL = the
                       bank only ever holds the ordered layout                                                                */
} ekv_bank;

/* One model forward over `layer_count` layers starting at `layer_begin` (all layers share the
 * geometry, as in the reference where every layer's cache has the same length). */
typedef struct ekv_step {
  int32_t layer_begin, layer_count;
  int32_t q_len;        /* 1 = decode, stride = prefill chunk                                            */
  int32_t n_slots;      /* T: live positions INCLUDING the q_len new ones                                */
  int32_t score_off;    /* P: first position covered by the score rows (decoding mode: prompt length)    */
  int32_t policy;       /* EKV_POLICY_*                                                                   */
  int32_t accumulate;   /* 1: add this forward's probabilities to the score rows                         */
  int32_t n_evict;      /* victims per (layer, head) after the attention; 0 = none                       */
  int32_t win_lo;       /* h2o/tova: first candidate index; roco: leading indices forced to 1e9 (sink)   */
  int32_t win_tail;     /* h2o/tova: trailing indices excluded (recent window)                           */
  int32_t roco_k1;      /* roco stage 1: size of the smallest-std feasible set                           */
  int32_t roco_tail;    /* roco: trailing indices forced to 1e9 (10 in the reference)                    */
  int32_t range_start;  /* EKV_POLICY_RANGE: evict positions [range_start, range_start + n_evict)        */
  int32_t tova_head_mean; /* encoding/ppl 'tova': one head-averaged last-query row for all heads (:456)  */
  int32_t causal;       /* 1: the last q_len positions are the chunk itself, causal inside it            */
  int32_t rope_on_read; /* 1: streaming variant, rotate keys by position index at read time             */
  int32_t n_split;      /* key-range splits per head (0 = choose)                                        */
  int32_t phases;       /* 0 = whole step; else bit mask: 1 attention kernel, 2 scorer (fold+score), 4 fold only, 8 scorer
                           without the fold (1|4 then 8 lets the caller run the scorer on a side stream)          */
  float count_add;      /* added to C before selection (1 decode, stride prefill); 0 = leave             */
  float count_tail_step;/* C tail after compaction: tail[i] = i * count_tail_step (0 decode, -1 prefill) */
  float sm_div;         /* logits are divided by this (sqrt(head_dim))                                   */
  int32_t two_pass;     /* scored chunk steps: 0 = library decides (two passes from 40 GQA-folded query rows, one pass below,
                           for tova and head_dim 32 with rope_on_read; 9..64 rows against <= 1280 plain keys — <= 32 rows: 2560 — at head_dim 128: the
                           one-launch logits-resident kernel), 1 = two passes — on the wide-block kernel one pass over K and V (output +
                           row statistics) and a K-only column-sum pass; on the 16x16 kernel a statistics pass + an exact pass —
                           whenever the shape allows it, -1 = always one pass with exported logits                      */
  int32_t phys_extent;  /* E: every live row of these layers has a physical index < E (n_slots <= E <= cap), and rows
                           [0, E) hold initialised memory.  0 = unknown (cap is used).  The one-launch decode step streams
                           the rows [0, E) in PHYSICAL order (sequential HBM reads however fragmented the slot map is) and
                           masks the dead ones, so a tight E saves reading free rows.  With the free list kept as this
                           library keeps it (freed rows first, then never-used rows ascending) E is simply the high-water
                           mark of n_slots.                                                                          */
  int32_t defer_layers; /* > 0: DEFERRED SCORER for a model that issues one layer per call (a real decoder stack: layer l + 1's
                           query depends on layer l's output, easykv/easykv.py:264-269).  The attention output of a layer is
                           needed at once, its scoring / eviction only before the NEXT forward: the per-layer call (decode steps,
                           and since ABI 5 chunk steps of any q_len; phases = 1|4: attention + fold — for two-pass steps of the
                           wide-block kernel the column-sum pass is deferred as well and runs in the phases = 8 call) leaves its logits and partials in slice `defer_index` of a workspace laid
                           out for `defer_layers` layers, and ONE call with phases = 8 over all those layers
                           (layer_count = defer_layers, defer_index = 0) scores and evicts for the whole token.  Both calls must
                           pass the same explicit n_split and the same workspace.  0 = off.                               */
  int32_t defer_index;  /* slice of this call's first layer in the deferred workspace                                      */
  /* Row strides of the call's tensors, in ELEMENTS (ABI 8; SURVEY.md §8b "raw device pointers + explicit strides").  A row is the
   * head_dim contiguous halfs of one (head, token); inside a layer's block it sits at  head * head_stride + token * token_stride,
   * and the layers of a multi-layer call follow each other n_heads * q_len * head_dim elements apart.  Both zero = the dense layout
   * [heads][q_len][head_dim] (token_stride = head_dim, head_stride = q_len * head_dim).  The patched attention modules of HF
   * transformers hand over [1, heads, q_len, head_dim] VIEWS of the projections' [1, q_len, heads * head_dim] output
   * (llama_patch.py:176-182 does the same transpose): token_stride = heads * head_dim, head_stride = head_dim — read in place, no
   * copy kernels in front of the step, and `out` written straight in the [q_len][heads * head_dim] layout o_proj wants
   * (llama_patch.py:230-232 transposes back).  Strides must be multiples of 8 (16-byte row loads); for q_len = 1 only
   * head_stride = head_dim is accepted (token_stride is irrelevant).                                                      */
  int32_t q_token_stride, q_head_stride;      /* q                                                                          */
  int32_t kv_token_stride, kv_head_stride;    /* k_new and v_new                                                            */
  int32_t out_token_stride, out_head_stride;  /* out                                                                        */
} ekv_step;

int ekv_abi_version(void);
const char *ekv_strerror(int code);

/* bytes of scratch ekv_step_attend needs for (bank, step) */
size_t ekv_workspace_bytes(const ekv_bank *bank, const ekv_step *step);
size_t ekv_workspace_bytes_typed(const ekv_bank *bank, const ekv_step *step, int32_t dtype);

/* How ekv_step_attend will run (bank, step): *n_split = key-range splits per head, *fused = 1 when the whole
 * step is ONE launch (the fused decode kernel, the logits-in-LDS chunk kernel, or a chunk step whose scorer runs as the tail
 * of its attention kernel), 0 when it is an attention launch (two for the two-pass chunk scheme) + fold / scorer launches. */
int ekv_step_plan(const ekv_bank *bank, const ekv_step *step, int32_t *n_split, int32_t *fused);

/* The dispatch decisions behind ekv_step_plan, for host code that must shape its calls after them instead of mirroring the rules
 * (ABI 5): info[0 .. n_info) <- { n_split, fused, two_pass (1 = statistics + column-sum scheme, no logits in HBM), wide (1 = the
 * 32x32x16 wide-block kernel, which walks all query blocks of a head inside one launch), n_qblocks, qb_rows, n_col_parts,
 * fold_in_kernel, n_launches (ABI 7: kernel launches this call issues — a two-pass wide step is 2 since the scorer became the tail
 * of its column-sum pass, 3 before; 0 = the dispatch refuses the step), fused_order (phase order of the one-launch decode step's
 * workgroups: 0 = all stream K+V and then run the scorer tail, 1 = mixed per CU with workgroups that run the tail between the K and
 * the V rows, 2 = all of those; same results either way; EKV_FUSED_ORDER=0|1|2 in the environment forces it) }; entries beyond EKV_STEP_INFO_N are zeroed.  The reference has no counterpart (its keep_attention prefix
 * materialises the r x r map, easykv/easykv.py:396-405); easykv_amd.api uses it to decide whether a scored prefix goes down as
 * one step or in query blocks. */
#define EKV_STEP_INFO_N 10
int ekv_step_info(const ekv_bank *bank, const ekv_step *step, int32_t *info, int32_t n_info);
int ekv_step_info_typed(const ekv_bank *bank, const ekv_step *step, int32_t dtype, int32_t *info, int32_t n_info);

/* Resident rows of the one-launch decode step.  Step i + 1 reads the K/V rows of step i except one per head, so a fixed share of the
 * bank can stay in the 256 MiB Infinity Cache between two steps: the physical rows [0, R) of every head of a launch are read with
 * default-policy loads, the rest non-temporally as before (results are bit-identical for every R).  R is planned per launch from a
 * byte budget: the largest multiple of 32 rows whose K + V bytes, plus the score rows, slot map and birth rows the step re-reads
 * anyway, fit it; at most the physical extent rounded up to 32, so a launch that fits entirely is read with plain loads.  R is 0
 * for RoPE-on-read, quantised rows, batched and split steps, and for shapes other than head_dim 128 with one query head per KV head
 * on the slot-indexed score rows.  The budget: EKV_RESIDENT_MB in the environment (MiB, read once per process; 0 = every K/V load
 * non-temporal) over the library's default, until ekv_set_resident_bytes sets a value for the process (negative: back to the
 * former).  A caller whose process streams more than the cache holds between two decode steps of a layer (a model's weights) should
 * set 0: plain loads that miss are slower than non-temporal ones.  ekv_step_resident_rows is the dry run: R of (bank, step), or a
 * negative error code.  EKV_RESIDENT_ROWS in the environment forces R (capped at the rounded extent) under any budget but 0, for A/B
 * runs and tests: a caller that set the budget to 0 keeps every load non-temporal. */
int ekv_set_resident_bytes(int64_t bytes);
int ekv_step_resident_rows(const ekv_bank *bank, const ekv_step *step, int32_t dtype);

/* slot_of_pos <- identity for the whole bank */
int ekv_bank_reset(const ekv_bank *bank, void *stream);

/* Score-row initialisation for `layer_count` layers from `layer_begin` over width W:
 *   S = Q = 0;  C[j] = c0 - j for j < ramp_from ... see easykv/easykv.py:242-245, :412-416.
 * mode 0 (decoding, :245):            C[j] = (W-1) - j
 * mode 1 (prefill, keep_attention):   C[j] = (W - j) - stride
 * mode 2 (prefill, no keep):          C[j] = 0 for j < W-stride, else -(j-(W-stride))            */
int ekv_state_init(const ekv_bank *bank, int32_t layer_begin, int32_t layer_count, int32_t width, int32_t mode,
                   int32_t stride, void *stream);

/* The fused step: append q_len new K/V rows, attention of the q_len queries over the n_slots live
 * positions, GQA fold, score accumulation, victim selection, slot-map + score-row compaction.
 *   q      16-bit [layer_count][n_q_heads][q_len][head_dim]    (dense, or rows at ekv_step.q_*_stride)
 *   k_new  16-bit [layer_count][n_kv_heads][q_len][head_dim]   (already rotated unless rope_on_read; ekv_step.kv_*_stride)
 *   v_new  16-bit [layer_count][n_kv_heads][q_len][head_dim]   (same strides as k_new)
 *   out    16-bit [layer_count][n_q_heads][q_len][head_dim]    (ekv_step.out_*_stride)
 *          (16-bit: fp16, or bf16 through the _typed calls — the bank's k / v in the same type)
 *   evict_ids int32 [layer_count][n_kv_heads][n_evict] or NULL: evicted logical positions, ascending
 *   rope_cos/rope_sin fp32 [>= n_slots][head_dim] or NULL; layout cat(freqs, freqs) as in the reference (llama_patch.py:74-98):
 *                    the kernels read the first half of a row for both halves of the head.  The tables must be what RoPE tables are —
 *                    a rotation LINEAR in the position, row j = (cos(j * theta_f), sin(j * theta_f)) for per-frequency angles
 *                    theta_f of any scaling (linear / NTK / llama3 / yarn frequencies) — : the decode stream reads only the first
 *                    row of every run of consecutive positions from the table and advances (cos, sin) to the following rows by the
 *                    angle-addition recurrence with row 1 as the step (easykv_amd.KVBank.set_rope verifies the property)
 * After the call the bank holds n_slots - n_evict live positions (the caller tracks that number). */
int ekv_step_attend(const ekv_bank *bank, const ekv_step *step, const void *q, const void *k_new, const void *v_new,
                    void *out, int32_t *evict_ids, const float *rope_cos, const float *rope_sin, void *workspace,
                    size_t workspace_bytes, void *stream);
int ekv_step_attend_typed(const ekv_bank *bank, const ekv_step *step, int32_t dtype, const void *q, const void *k_new,
                          const void *v_new, void *out, int32_t *evict_ids, const float *rope_cos, const float *rope_sin,
                          void *workspace, size_t workspace_bytes, void *stream);

/* Dry run of ekv_step_attend (ABI 4): every argument / shape / capability test of the real call for (bank, step), in the same
 * order, and nothing launched — no data pointer, workspace or stream is needed.  Returns what ekv_step_attend would return
 * before its first launch (EKV_OK, EKV_E_ARG, EKV_E_UNSUPPORTED).  For callers that split a step over several calls (the
 * deferred scorer: per-layer phases = 1|4 calls append rows long before the phases = 8 call that scores them), so that a shape
 * the LAST call would refuse is refused before the FIRST one touches the bank. */
int ekv_step_check(const ekv_bank *bank, const ekv_step *step);
int ekv_step_check_typed(const ekv_bank *bank, const ekv_step *step, int32_t dtype);

/* Slot-indexed score rows (ABI 6).  In the ordered layout an eviction shifts every entry of S / Q / C and of the slot map behind
 * the victim: a decode step rewrites all of them (28 KB per head at 2 k slots), and written bytes cost about twice what read
 * bytes do in the middle of the K/V stream.  ekv_rows_to_slots re-indexes the score rows of `layer_count` layers (n_slots live
 * entries each) by PHYSICAL row — S[row], Q[row], a count base C0[row] in score_cnt (count = C0 + the head's running sum of
 * count_add, slot_state[head][0]) and an order key birth[row] (the rank of `birth` among the live rows is the entry's order index;
 * the next birth is slot_state[head][1] as int32; [2] = the last decode step's roco threshold key, a hint for the next select; [3] = the same for the logits-in-LDS chunk kernel,
 * which uses it on the ordered layout too) — after which a step with EKV_PHASE_SLOT_ROWS set in `phases` moves nothing on an
 * eviction: the victim's row goes to the front of the free list (slot_of_pos[n_slots - 1]), S / Q of the live rows are rewritten,
 * C0 / birth only for the appended row.  Decisions (victims, ties to the older entry) and reported ids (order indices) are those
 * of the ordered layout.  While a layer is in this layout slot_of_pos[0, n_slots) is undefined and only steps with the flag may
 * run on it; ekv_rows_to_order converts back (slot map, score rows and zero tails exactly as the ordered steps would have left
 * them, counts included while all count_add were integers).  ekv_step_check / ekv_step_attend return EKV_E_UNSUPPORTED for a
 * flagged step the layout does not cover: anything but a one-launch decode step (q_len = 1, phases otherwise 0) with plain keys, a
 * scored policy with accumulate, score_off = 0, win_lo = 0, n_evict <= 1, GQA factor <= 4, phys_extent <= 6144, cap <= 9600, and a bank
 * that carries score_sq and score_cnt (the count base of every policy's appended row lives in score_cnt). */
#define EKV_PHASE_SLOT_ROWS 16
/* with EKV_PHASE_SLOT_ROWS: the caller guarantees that this step's protected tail (roco: 10 entries; h2o_head: win_tail) is not
 * longer than that of any earlier evicting step since ekv_rows_to_slots — the newest entries then have consecutive births and the
 * kernel skips the counting check (one block reduction) that otherwise proves it, with an exact bisection when it fails */
#define EKV_PHASE_SLOT_TAIL_OK 32
int ekv_rows_to_slots(const ekv_bank *bank, int32_t layer_begin, int32_t layer_count, int32_t n_slots, void *stream);
int ekv_rows_to_order(const ekv_bank *bank, int32_t layer_begin, int32_t layer_count, int32_t n_slots, void *stream);

/* Ordered view: k_out/v_out 16-bit (the bank's type) [layer_count][n_kv_heads][n_slots][head_dim] <- rows in position order */
int ekv_gather_ordered(const ekv_bank *bank, int32_t layer_begin, int32_t layer_count, int32_t n_slots, void *k_out,
                       void *v_out, void *stream);

/* Load ordered rows into the bank at positions [pos_begin, pos_begin+n) (prefix prefill / cache import):
 *   k_in/v_in 16-bit (the bank's type) [layer_count][n_kv_heads][n][head_dim] */
int ekv_scatter_rows(const ekv_bank *bank, int32_t layer_begin, int32_t layer_count, int32_t pos_begin, int32_t n,
                     const void *k_in, const void *v_in, void *stream);

/* Reference-shaped physical compaction (easykv/easykv.py:56-82) for a bank in identity layout:
 * removes `n_evict` ascending positions per (layer, head) from the first n_slots rows in place,
 * order-preserving.  evict_ids int32 [layer_count][n_kv_heads][n_evict]. */
int ekv_compact_inplace(const ekv_bank *bank, int32_t layer_begin, int32_t layer_count, int32_t n_slots,
                        int32_t n_evict, const int32_t *evict_ids, void *stream);

/* FP8 K/V storage with per-row scales ("kv8"; ABI 8, additive).  A bank's K/V rows may be held as
 *
 *   k_codes, v_codes   uint8 [n_layers][n_kv_heads][cap][head_dim]   OCP e4m3fn codes (not fnuz), one byte per element
 *   k_scale, v_scale   fp32  [n_layers][n_kv_heads][cap]             one scale per (layer, KV head, PHYSICAL row);  value = code * scale
 *
 * — 2 * head_dim + 8 bytes per K+V row pair instead of 4 * head_dim (264 instead of 512 at head_dim 128).  Rows never move, so a
 * row's scale lives at the row's physical index for the row's whole life, and the slot map, the free list and the score rows (either
 * layout) are those of the 16-bit bank: selection reads logits, never a K/V element.
 *
 * Quantisation rule of a row x (normative):  amax = max |x| over the row, in fp32;  s = amax / 448  (s = 1 when amax == 0);
 * code = round-to-nearest-even(x / s), x / s being the correctly rounded fp32 quotient.  Nothing saturates by construction.  Rows are
 * assumed finite.  What is stored is what is attended: the row a decode step appends takes part in that step's attention AS
 * QUANTISED, so the bank's contents alone determine the step.
 *
 * The descriptor carries the four planes; every other field of `bank` is used as it is, and bank->k / bank->v are NOT read by the
 * kv8 step calls (they may be NULL once the 16-bit rows have been released). */
typedef struct ekv_kv8 {
  void *k_codes, *v_codes;
  float *k_scale, *v_scale;
} ekv_kv8;

/* Bank conversion, one pass: rows [0, extent) of `layer_count` layers of the 16-bit bank (dtype: EKV_DTYPE_F16 / _BF16 = the type of
 * bank->k / bank->v) -> codes and scales at the SAME physical indices.  Rows >= extent and the 16-bit rows are left untouched. */
int ekv_kv8_quantize(const ekv_bank *bank, const ekv_kv8 *kv8, int32_t dtype, int32_t layer_begin, int32_t layer_count,
                     int32_t extent, void *stream);
/* The inverse, for tests and tooling: k_out / v_out [layer_count][n_kv_heads][extent][head_dim] <- code * scale of the physical rows
 * [0, extent), as out_dtype: EKV_DTYPE_F16, EKV_DTYPE_BF16 (rounded to nearest even) or EKV_DTYPE_F32 (exact). */
#define EKV_DTYPE_F32 2 /* ekv_kv8_dequantize's out_dtype only: no step takes fp32 tensors */
int ekv_kv8_dequantize(const ekv_bank *bank, const ekv_kv8 *kv8, int32_t out_dtype, int32_t layer_begin, int32_t layer_count,
                       int32_t extent, void *k_out, void *v_out, void *stream);

/* Decode steps on a kv8 bank: the _typed calls with the descriptor; `dtype` is the type of q, k_new, v_new and out (EKV_DTYPE_F16 /
 * _BF16, anything else EKV_E_ARG).  Accepted: q_len == 1 with plain keys at head_dim 64 / 128 — every policy, every GQA factor and
 * every phase combination the 16-bit decode step takes (whole step incl. the one-launch kernel on either score-row layout, the split
 * path, the deferred per-layer form), planned exactly as the 16-bit step of that shape (same splits, launches and workspace) and run
 * on the kv8 builds of the decode attention kernels: codes are widened in registers, logit = (q . codes) * k_scale[row] / sm_div,
 * v_scale[row] is folded into p, and the appended row is quantised by the kernel (codes + scale written to the recycled row).
 * Everything else is EKV_E_UNSUPPORTED from the dry run, before anything is launched: q_len > 1 (chunk steps), rope_on_read,
 * head_dim 32 / 96.  The row moves (ekv_gather_ordered, ekv_scatter_rows, ekv_compact_inplace) do not serve kv8 banks. */
int ekv_kv8_step_check(const ekv_bank *bank, const ekv_step *step, int32_t dtype, const ekv_kv8 *kv8);
int ekv_kv8_step_info(const ekv_bank *bank, const ekv_step *step, int32_t dtype, const ekv_kv8 *kv8, int32_t *info, int32_t n_info);
size_t ekv_kv8_workspace_bytes(const ekv_bank *bank, const ekv_step *step, int32_t dtype, const ekv_kv8 *kv8);
int ekv_kv8_step_attend(const ekv_bank *bank, const ekv_step *step, int32_t dtype, const ekv_kv8 *kv8, const void *q,
                        const void *k_new, const void *v_new, void *out, int32_t *evict_ids, const float *rope_cos,
                        const float *rope_sin, void *workspace, size_t workspace_bytes, void *stream);

/* MXFP4 K/V storage with block scales ("kv4"; ABI 8, additive; head_dim 128).  A bank's K/V rows may be held as
 *
 *   k_codes, v_codes   uint8 [n_layers][n_kv_heads][cap][head_dim / 2]    two e2m1 codes per byte: element 2i in the low nibble
 *                                                                         (bits 3:0), element 2i + 1 in the high nibble (bits 7:4) —
 *                                                                         the order the gfx950 pack conversions read and write
 *   k_exp,   v_exp     uint8 [n_layers][n_kv_heads][cap][head_dim / 32]   E8M0: one biased exponent per 32-element block of the
 *                                                                         PHYSICAL row;  value = code * 2^(byte - 127)
 *
 * — head_dim + head_dim / 16 bytes per K+V row pair: 136 at head_dim 128, against 264 (kv8) and 512 (16-bit rows).  A code is sign
 * (bit 3) and magnitude index into {0, 0.5, 1, 1.5, 2, 3, 4, 6}.  As for kv8, rows never move: a row's exponents live at its physical
 * index, and the slot map, the free list and the score rows (either layout) are those of the 16-bit bank.
 *
 * Quantisation rule of a block x[0..32) (normative), in fp32:  amax = max |x|;  e = the smallest integer with amax <= 6 * 2^e, clamped
 * to [-126, 127], and e = 0 for an all-zero block;  the stored byte is e + 127 (255 never occurs);  code = round-to-nearest(x / 2^e)
 * onto the eight magnitudes with the sign of x, ties to the even code (1.25 -> 1, 2.5 -> 2, 5 -> 4).  The quotient is exact, |x / 2^e|
 * <= 6, so nothing saturates by construction and the rule has no rounding of its own: an implementation is bit-identical to another
 * up to the sign of zero — codes 0 and 8 (+0 / -0) are equivalent.  Rows are assumed finite.  What is stored is what is attended:
 * the row a decode step appends is quantised by the kernel and takes part in that step AS QUANTISED.
 *
 * The descriptor carries the four planes; every other field of `bank` is used as it is, and bank->k / bank->v are NOT read by the
 * kv4 step calls. */
typedef struct ekv_kv4 {
  void *k_codes, *v_codes;
  uint8_t *k_exp, *v_exp;
} ekv_kv4;

/* Bank conversion and its inverse: the arguments and contracts of ekv_kv8_quantize / ekv_kv8_dequantize (rows [0, extent) at the same
 * physical indices, rows >= extent and the 16-bit rows untouched; out_dtype EKV_DTYPE_F32 is exact: code * 2^e).  head_dim != 128 is
 * EKV_E_UNSUPPORTED. */
int ekv_kv4_quantize(const ekv_bank *bank, const ekv_kv4 *kv4, int32_t dtype, int32_t layer_begin, int32_t layer_count,
                     int32_t extent, void *stream);
int ekv_kv4_dequantize(const ekv_bank *bank, const ekv_kv4 *kv4, int32_t out_dtype, int32_t layer_begin, int32_t layer_count,
                       int32_t extent, void *k_out, void *v_out, void *stream);

/* Decode steps on a kv4 bank: the ekv_kv8_step_* signatures with the kv4 descriptor.  Accepted: q_len == 1 with plain keys at
 * head_dim 128 and a GQA factor <= 4 (factor 3 on the padded build), fp16 / bf16 q, k_new, v_new and out — every policy and every
 * phase combination the 16-bit decode step takes (the whole step incl. the one-launch kernel on either score-row layout, the split
 * path, the deferred per-layer form), planned exactly as the 16-bit step of that shape: same splits, launches, workspace and info
 * fields, fused_order 0.  The kv4 builds of the decode attention kernels read a row as a 4-lane group, one block per lane: the lane's
 * partial q . codes is multiplied by its block's 2^e before the group sum, V codes are converted to fp32 with the block's scale, and
 * the appended row is quantised by its lane group (codes + exponents written to the recycled row).  Everything behind the logits is
 * the 16-bit step's.  EKV_E_UNSUPPORTED from the dry run, before anything is launched: q_len > 1, rope_on_read, head_dim != 128, a
 * GQA factor > 4.  A missing plane is EKV_E_ARG.  The row moves do not serve kv4 banks; the batch form is ekv_kv4_batch_* below. */
int ekv_kv4_step_check(const ekv_bank *bank, const ekv_step *step, int32_t dtype, const ekv_kv4 *kv4);
int ekv_kv4_step_info(const ekv_bank *bank, const ekv_step *step, int32_t dtype, const ekv_kv4 *kv4, int32_t *info, int32_t n_info);
size_t ekv_kv4_workspace_bytes(const ekv_bank *bank, const ekv_step *step, int32_t dtype, const ekv_kv4 *kv4);
int ekv_kv4_step_attend(const ekv_bank *bank, const ekv_step *step, int32_t dtype, const ekv_kv4 *kv4, const void *q,
                        const void *k_new, const void *v_new, void *out, int32_t *evict_ids, const float *rope_cos,
                        const float *rope_sin, void *workspace, size_t workspace_bytes, void *stream);

/* MXFP6 K/V storage with block scales ("kv6"; ABI 8, additive; head_dim 128).  A bank's K/V rows may be held as
 *
 *   k_codes, v_codes   uint8 [n_layers][n_kv_heads][cap][3 * head_dim / 4]   32 six-bit e2m3 codes per 24-byte block, 4 blocks per row
 *                                                                            (head_dim 128: 96 bytes)
 *   k_exp,   v_exp     uint8 [n_layers][n_kv_heads][cap][head_dim / 32]      E8M0, exactly kv4's plane: value = code * 2^(byte - 127)
 *
 * — 3 * head_dim / 2 + head_dim / 16 bytes per K+V row pair: 200 at head_dim 128, against 136 (kv4), 264 (kv8) and 512 (16-bit rows).
 * A code is sign (bit 5) and a magnitude index i (bits 4:0): the value is i / 8 for i < 8 and (1 + (i & 7) / 8) * 2^((i >> 3) - 1)
 * otherwise — the grid 0 .. 0.875 and 1 .. 1.875 in steps of 0.125, 2 .. 3.75 in steps of 0.25, 4 .. 7.5 in steps of 0.5.
 * Packing: element j of a block sits at bits [6j, 6j + 6) of the block's 24 bytes read as one little-endian 192-bit integer — the
 * order v_cvt_scalef32_pk32_{f32,f16,bf16}_fp6 read (measured on MI355X).  v_cvt_scalef32_2xpk16_fp6_f32 writes that order with its
 * operands INTERLEAVED: element i of the first operand lands at position 2i, of the second at 2i + 1 (measured likewise), so a block
 * is packed from its even and its odd elements.  Rows never move, as for kv8 / kv4.
 *
 * Quantisation rule of a block x[0..32) (normative), in fp32:  amax = max |x|;  e = the smallest integer with amax <= 7.5 * 2^e, clamped
 * to [-126, 127], and e = 0 for an all-zero block;  the stored byte is e + 127 (255 never occurs);  code = round-to-nearest(x / 2^e)
 * onto the 32 magnitudes with the sign of x, ties to the even code (1.9375 -> 2, 3.875 -> 4, 0.0625 -> 0).  The quotient is exact,
 * |x / 2^e| <= 7.5, so nothing saturates by construction and the rule has no rounding of its own: an implementation is bit-identical
 * to another up to the sign of zero — codes 0 and 32 (+0 / -0) are equivalent.  Rows are assumed finite.  What is stored is what is
 * attended: the row a decode step appends is quantised by the kernel and takes part in that step AS QUANTISED.
 *
 * The descriptor carries the four planes; bank->k / bank->v are NOT read by the kv6 step calls. */
typedef struct ekv_kv6 {
  void *k_codes, *v_codes;
  uint8_t *k_exp, *v_exp;
} ekv_kv6;

/* Bank conversion and its inverse: the arguments and contracts of ekv_kv4_quantize / ekv_kv4_dequantize (out_dtype EKV_DTYPE_F32 is
 * exact: code * 2^e).  head_dim != 128 is EKV_E_UNSUPPORTED. */
int ekv_kv6_quantize(const ekv_bank *bank, const ekv_kv6 *kv6, int32_t dtype, int32_t layer_begin, int32_t layer_count,
                     int32_t extent, void *stream);
int ekv_kv6_dequantize(const ekv_bank *bank, const ekv_kv6 *kv6, int32_t out_dtype, int32_t layer_begin, int32_t layer_count,
                       int32_t extent, void *k_out, void *v_out, void *stream);

/* Decode steps on a kv6 bank: the ekv_kv4_step_* signatures with the kv6 descriptor, and exactly what a kv4 step accepts — q_len == 1
 * with plain keys at head_dim 128 and a GQA factor <= 4 (factor 3 on the padded build), fp16 / bf16 q, k_new, v_new and out, every
 * policy and phase combination of the 16-bit decode step — planned exactly as the 16-bit step of that shape, fused_order 0.  The kv6
 * builds read a row as a 4-lane group, one 24-byte block per lane: the lane's partial q . codes is multiplied by its block's 2^e
 * before the group sum, V codes are converted to fp32 with the block's scale, and the appended row is quantised by its lane group.
 * EKV_E_UNSUPPORTED from the dry run, before anything is launched: q_len > 1, rope_on_read, head_dim != 128, a GQA factor > 4.  A
 * missing plane is EKV_E_ARG.  The row moves do not serve kv6 banks; the batch form is ekv_kv6_batch_* below. */
int ekv_kv6_step_check(const ekv_bank *bank, const ekv_step *step, int32_t dtype, const ekv_kv6 *kv6);
int ekv_kv6_step_info(const ekv_bank *bank, const ekv_step *step, int32_t dtype, const ekv_kv6 *kv6, int32_t *info, int32_t n_info);
size_t ekv_kv6_workspace_bytes(const ekv_bank *bank, const ekv_step *step, int32_t dtype, const ekv_kv6 *kv6);
int ekv_kv6_step_attend(const ekv_bank *bank, const ekv_step *step, int32_t dtype, const ekv_kv6 *kv6, const void *q,
                        const void *k_new, const void *v_new, void *out, int32_t *evict_ids, const float *rope_cos,
                        const float *rope_sin, void *workspace, size_t workspace_bytes, void *stream);

/* FP8 keys with MXFP4 values ("kv84"; ABI 8, additive; head_dim 128).  A bank's K/V rows may be held as
 *
 *   k_codes   uint8 [n_layers][n_kv_heads][cap][head_dim]        and   k_scale   fp32  [n_layers][n_kv_heads][cap]
 *   v_codes   uint8 [n_layers][n_kv_heads][cap][head_dim / 2]    and   v_exp     uint8 [n_layers][n_kv_heads][cap][head_dim / 32]
 *
 * — head_dim + 4 bytes of K and head_dim / 2 + head_dim / 32 bytes of V per row: 200 per K+V row pair at head_dim 128, what kv6 takes,
 * against 264 (kv8) and 136 (kv4).  The K planes follow the quantisation rule of kv8 ("FP8 K/V storage" above: layout, rule and scale
 * of ekv_kv8's k_codes / k_scale), the V planes the rule of kv4 ("MXFP4 K/V storage": layout, packing, rule and exponent of ekv_kv4's
 * v_codes / v_exp); neither is restated here.  The eviction scores of a step are computed from its logits alone, so a kv84 bank takes
 * the eviction decisions of the kv8 bank with the same K planes, exactly; the V format touches the output only.  What is stored is
 * what is attended, for both planes.  Rows never move, as for kv8 / kv4.
 *
 * The descriptor carries the four planes; bank->k / bank->v are NOT read by the kv84 step calls (they may be NULL). */
typedef struct ekv_kv84 {
  void *k_codes, *v_codes;
  float *k_scale;
  uint8_t *v_exp;
} ekv_kv84;

/* Bank conversion and its inverse: the arguments and contracts of ekv_kv8_quantize / ekv_kv8_dequantize and of the kv4 pair
 * (out_dtype EKV_DTYPE_F32 is exact: code * scale for K, code * 2^e for V).  head_dim != 128 is EKV_E_UNSUPPORTED. */
int ekv_kv84_quantize(const ekv_bank *bank, const ekv_kv84 *kv84, int32_t dtype, int32_t layer_begin, int32_t layer_count,
                      int32_t extent, void *stream);
int ekv_kv84_dequantize(const ekv_bank *bank, const ekv_kv84 *kv84, int32_t out_dtype, int32_t layer_begin, int32_t layer_count,
                        int32_t extent, void *k_out, void *v_out, void *stream);

/* Decode steps on a kv84 bank: the ekv_kv8_step_* signatures with the kv84 descriptor — q_len == 1 with plain keys at head_dim 128,
 * the GQA factors a kv8 step takes, fp16 / bf16 q, k_new, v_new and out, every policy and phase combination of the 16-bit decode
 * step — planned exactly as the 16-bit step of that shape, fused_order 0.  The kv84 builds run on the geometry of the kv8 builds (a row
 * is an 8-lane group, 16 elements per lane) and their K side is the kv8 builds' arithmetic: logits, softmax partials, scores and
 * victims are bit for bit those of a kv8 step on the same K planes.  A lane's V piece is half a block (16 codes) under the block's
 * exponent; the appended row's K is quantised by the kv8 rule, its V by the kv4 rule (block maximum over the lane pair).
 * EKV_E_UNSUPPORTED from the dry run, before anything is launched: q_len > 1, rope_on_read, head_dim != 128.  A missing plane is
 * EKV_E_ARG.  The row moves do not serve kv84 banks; the batch form is ekv_kv84_batch_* below. */
int ekv_kv84_step_check(const ekv_bank *bank, const ekv_step *step, int32_t dtype, const ekv_kv84 *kv84);
int ekv_kv84_step_info(const ekv_bank *bank, const ekv_step *step, int32_t dtype, const ekv_kv84 *kv84, int32_t *info, int32_t n_info);
size_t ekv_kv84_workspace_bytes(const ekv_bank *bank, const ekv_step *step, int32_t dtype, const ekv_kv84 *kv84);
int ekv_kv84_step_attend(const ekv_bank *bank, const ekv_step *step, int32_t dtype, const ekv_kv84 *kv84, const void *q,
                         const void *k_new, const void *v_new, void *out, int32_t *evict_ids, const float *rope_cos,
                         const float *rope_sin, void *workspace, size_t workspace_bytes, void *stream);

/* 16-bit keys with MXFP4 values ("kv164"; ABI 8, additive; head_dim 128).  A bank may keep its K rows as they are — bank->k, the
 * 16-bit rows [n_layers][n_kv_heads][cap][head_dim], untouched — and hold only its V rows as
 *
 *   v_codes   uint8 [n_layers][n_kv_heads][cap][head_dim / 2]    and   v_exp     uint8 [n_layers][n_kv_heads][cap][head_dim / 32]
 *
 * at the rows' physical indices: 2 * head_dim bytes of K and head_dim / 2 + head_dim / 32 bytes of V per row, 324 per K+V row pair at
 * head_dim 128 against 512 for 16-bit rows.  The V planes follow the rule of kv4 ("MXFP4 K/V storage" above: layout, packing, rule and
 * exponent of ekv_kv4's v_codes / v_exp), which is not restated here; they are exactly the V planes ekv_kv4_quantize and
 * ekv_kv84_quantize write for the same rows.  The eviction scores of a step are computed from its logits alone and the keys are not
 * quantised, so a kv164 bank takes the eviction decisions of the 16-bit bank with the same rows, exactly, on every path; the V format
 * touches the output only.  What is stored is what is attended.  Rows never move, as for kv8 / kv4.
 *
 * The descriptor carries the two V planes; K is bank->k, which the kv164 step calls READ and append to (NULL is EKV_E_ARG).  bank->v is
 * not read by them (it may be NULL). */
typedef struct ekv_kv164 {
  void *v_codes;
  uint8_t *v_exp;
} ekv_kv164;

/* Bank conversion and its inverse, V only.  ekv_kv164_quantize writes the two planes from bank->v (fp16 / bf16 by `dtype`) for the
 * physical rows [0, extent) of the layers [layer_begin, layer_begin + layer_count); it reads and writes nothing of K (bank->k may be
 * NULL here).  ekv_kv164_dequantize writes those rows of V densely, [layer_count][n_kv_heads][extent][head_dim], to v_out (out_dtype
 * EKV_DTYPE_F32 is exact: code * 2^e).  The argument checks and contracts are those of the kv4 pair; head_dim != 128 is
 * EKV_E_UNSUPPORTED; every check precedes any device access. */
int ekv_kv164_quantize(const ekv_bank *bank, const ekv_kv164 *kv164, int32_t dtype, int32_t layer_begin, int32_t layer_count,
                       int32_t extent, void *stream);
int ekv_kv164_dequantize(const ekv_bank *bank, const ekv_kv164 *kv164, int32_t out_dtype, int32_t layer_begin, int32_t layer_count,
                         int32_t extent, void *v_out, void *stream);

/* Decode steps on a kv164 bank: the ekv_kv8_step_* signatures with the kv164 descriptor — q_len == 1 with plain keys at head_dim 128,
 * every GQA factor the 16-bit decode step takes, fp16 / bf16 banks, q, k_new, v_new and out, every policy and phase combination of
 * the 16-bit decode step — planned exactly as the 16-bit step of that shape, fused_order 0 (no resident rows, no phase order K).  The
 * kv164 builds run on the geometry of the 16-bit builds (a row is a 16-lane group, 8 elements per lane) and their K side is the
 * 16-bit builds' code: logits, softmax partials, scores and victims are bit for bit those of a 16-bit step on the same K rows.  A
 * lane's V piece is a quarter of a block (8 codes, its own 8 output elements) under the block's exponent; the appended row's K is
 * stored as it comes, its V is quantised by the kv4 rule (block maximum over the lane quad) and attended as quantised.
 * EKV_E_UNSUPPORTED from the dry run, before anything is launched: q_len > 1, rope_on_read, head_dim != 128.  A missing plane or a
 * NULL bank->k is EKV_E_ARG.  The row moves do not serve kv164 banks; the batch form is ekv_kv164_batch_* below. */
int ekv_kv164_step_check(const ekv_bank *bank, const ekv_step *step, int32_t dtype, const ekv_kv164 *kv164);
int ekv_kv164_step_info(const ekv_bank *bank, const ekv_step *step, int32_t dtype, const ekv_kv164 *kv164, int32_t *info, int32_t n_info);
size_t ekv_kv164_workspace_bytes(const ekv_bank *bank, const ekv_step *step, int32_t dtype, const ekv_kv164 *kv164);
int ekv_kv164_step_attend(const ekv_bank *bank, const ekv_step *step, int32_t dtype, const ekv_kv164 *kv164, const void *q,
                          const void *k_new, const void *v_new, void *out, int32_t *evict_ids, const float *rope_cos,
                          const float *rope_sin, void *workspace, size_t workspace_bytes, void *stream);

/* Long score rows (ABI 8, additive): the *_typed calls of a 16-bit bank with a scorer whose row width is bounded by memory, not by one
 * CU's LDS.  The plain calls refuse a scored step with EKV_E_UNSUPPORTED once a head's score row has more than about 38 400 columns (the
 * generic scorer keeps its selection keys in LDS); the attention kernels have no such bound.  A long call plans exactly as the plain call
 * of the same (bank, step, dtype) — same tiling, same attention launches, same return codes for argument errors and for what an attention
 * kernel refuses — except where that plan would end in the generic scorer launch (whole steps, phases & 2, phases & 8, the deferred
 * flush over all layers).  There the long scorer runs instead, in two launches: a sweep over (column tile, head, layer) that builds the
 * working copies of the score rows and the selection keys in workspace scratch, and one 1024-thread workgroup per (head, layer) that
 * selects and compacts with its keys in that scratch.  Where the generic scorer would have folded the key-range partials into `out`
 * itself, a fold launch of the long family precedes the sweep.  The width refusal does not apply: n_slots is bounded by cap and the
 * workspace alone.  The arithmetic, its order and the selection rule (the k smallest (key, index) pairs, ties to the lowest index, NaN
 * largest) are the generic scorer's: wherever both families run, out, evict_ids, the slot map and the score rows are equal bit for bit.
 * Steps that end in another scorer (the one-launch kernels, the fast decode scorer, a kernel tail, the range compaction) plan and run
 * field for field as the plain call.  16-bit rows and single sequences only: the quantised and the batched calls have no long form.
 * ekv_long_step_info fills the EKV_STEP_INFO_N fields of the plain info call, then [10] = 1 when the step ends in the long scorer (0
 * otherwise, and for a step the call refuses) and [11] = the column tiles per head of its sweep (0 likewise); entries beyond
 * EKV_LONG_INFO_N are zeroed. */
#define EKV_LONG_INFO_N 12
int ekv_long_step_check(const ekv_bank *bank, const ekv_step *step, int32_t dtype);
int ekv_long_step_info(const ekv_bank *bank, const ekv_step *step, int32_t dtype, int32_t *info, int32_t n_info);
size_t ekv_long_workspace_bytes(const ekv_bank *bank, const ekv_step *step, int32_t dtype);
int ekv_long_step_attend(const ekv_bank *bank, const ekv_step *step, int32_t dtype, const void *q, const void *k_new,
                         const void *v_new, void *out, int32_t *evict_ids, const float *rope_cos, const float *rope_sin,
                         void *workspace, size_t workspace_bytes, void *stream);

/* Soft-capped logits (ABI 8, additive): the *_typed calls of a 16-bit bank with attention-logit soft-capping (Gemma 2:
 * attn_logit_softcapping).  NORMATIVE.  For a real (not masked, not dead) key the logit of a capped call is
 *
 *     s = cap * tanh((q.k / sm_div) / cap)          in fp32, cap finite and > 0
 *
 * Masked and dead entries become -inf AFTER the cap (the mask is added to the capped logit); NaN propagates; +-inf gives +-cap.
 * Everything downstream sees s and nothing else: the online and the exact softmax, the exported logits rows, the (m, l, o) partials and
 * their fold, the row statistics and column sums of the two-pass chunk scheme, the decode tails and every scorer (eviction scores are
 * sums of the probabilities of s).  The uncapped calls compute the same with s = q.k / sm_div.  One device function evaluates s for
 * every capped kernel (ekv_softcap, csrc/ekv_common.h: a form without the cancellation of 1 - 2 / (1 + e^2y) near 0; within 0.75 ulp of
 * the float64 value for a power-of-two cap, within 2 ulp otherwise), and ekv_softcap_eval below applies it to a vector for tests and tools.
 * ekv_step.sm_div is free in every call family, capped or not: the logits are q.k / sm_div whatever head_dim is.
 *
 * A capped DECODE step plans field for field as the uncapped call of the same (bank, step, dtype): same n_split, launches, workspace,
 * phase order and resident rows (info [9] and ekv_step_resident_rows of the plain call say which).  A capped CHUNK step or dense prefix
 * runs on the 16x16x32 kernel alone, in blocks of at most 32 GQA-folded rows at head_dim 128 as at head_dim 256, one pass or statistics +
 * exact pass by the rules of the plain call; it never resolves to the wide, the logits-in-LDS or the logits-resident kernel, so info [3]
 * (wide) is always 0.  Refused before any launch, with ekv_cap_workspace_bytes = 0: rope_on_read, head_dim 32 / 64 / 96, chunk steps
 * whose GQA factor exceeds 32 (EKV_E_UNSUPPORTED); a cap that is <= 0, NaN or infinite (EKV_E_ARG, behind the element type and before
 * anything else is read).  16-bit rows and single sequences only: there is no capped quantised, batched or long call. */
int ekv_cap_step_check(const ekv_bank *bank, const ekv_step *step, int32_t dtype, float softcap);
int ekv_cap_step_info(const ekv_bank *bank, const ekv_step *step, int32_t dtype, float softcap, int32_t *info, int32_t n_info);
size_t ekv_cap_workspace_bytes(const ekv_bank *bank, const ekv_step *step, int32_t dtype, float softcap);
int ekv_cap_step_attend(const ekv_bank *bank, const ekv_step *step, int32_t dtype, float softcap, const void *q, const void *k_new,
                        const void *v_new, void *out, int32_t *evict_ids, const float *rope_cos, const float *rope_sin,
                        void *workspace, size_t workspace_bytes, void *stream);
/* out[i] = cap * tanh((x[i] / sm_div) / cap) by the kernels' own function; x and out are DEVICE pointers to n floats (n = 0: nothing
 * runs).  EKV_E_ARG: n < 0, a NULL pointer with n > 0, sm_div <= 0 or NaN, a cap that is <= 0, NaN or infinite. */
int ekv_softcap_eval(const float *x, int64_t n, float sm_div, float cap, float *out, void *stream);

/* Attention sinks (ABI 8, additive): the *_typed calls of a 16-bit bank whose model adds one learned logit per query head to every
 * softmax (gpt-oss: `sinks`, handed to the attention function as s_aux).  NORMATIVE.  Take a query row of query head hq in bank layer l.
 * Its real-key logits are s_j = q.k_j / sm_div, formed exactly as the plain call forms them, with the mask and the dead rows already
 * applied as -inf.  The sink is a = sinks[l][hq], fp32 and finite.  Then
 *
 *     M   = max(max_j s_j, a)
 *     p_j = exp(s_j - M) / (sum_i exp(s_i - M) + exp(a - M))
 *     out = sum_j p_j v_j
 *
 * The sink is a virtual key with value 0.  It has no score column and no slot, and it is never a victim.  Everything downstream sees
 * p_j and nothing else: the outputs, the column sums, sum p / sum p^2 / counts, the tova row, the GQA mean over the group and every
 * select.  Selection rules, windows and tie rules are untouched.  Where M already includes a, the extra term is <= 1.  A sink far below
 * every logit (exp(a - M) rounds to 0) gives the plain call's results bit for bit.
 *
 * sinks: DEVICE pointer, fp32 [bank->n_layers][n_q_heads], indexed by BANK layer (step->layer_begin + the launch's layer); the dry-run
 * calls (check, info, workspace_bytes) only test it for NULL, and it must stay valid until the step has run (a captured graph keeps
 * the pointer).  No public struct changes.
 *
 * A sink DECODE step plans as the plain call of the same (bank, step, dtype): same n_split, launches and workspace.  The sink instances
 * are built without the mixed phase orders and without resident rows (as the kv164 ones): info [9] is 0, every workgroup runs order F.
 * A sink CHUNK step or dense prefix runs on the 16x16x32 kernel alone, by the rules of the capped call: blocks of at most 32 GQA-folded
 * rows; one pass, with the scorer as the kernel's tail where the step is one unsplit block, else statistics pass + exact pass + generic
 * scorer; never the wide, the logits-in-LDS or the logits-resident kernel, so info [3] (wide) is always 0.  Refused before any launch,
 * with ekv_sink_workspace_bytes = 0: rope_on_read, a head_dim other than 64 / 128, chunk steps whose GQA factor exceeds 32
 * (EKV_E_UNSUPPORTED); NULL sinks (EKV_E_ARG, behind the element type and before anything else is read).  The head-averaged TOVA row
 * (tova_head_mean) is rebuilt from the exported logits by a sink build of its kernel: M and the sum include the sink.  16-bit rows and single sequences only: there is no sink
 * batched, quantised, long or capped call. */
int ekv_sink_step_check(const ekv_bank *bank, const ekv_step *step, int32_t dtype, const float *sinks);
int ekv_sink_step_info(const ekv_bank *bank, const ekv_step *step, int32_t dtype, const float *sinks, int32_t *info, int32_t n_info);
size_t ekv_sink_workspace_bytes(const ekv_bank *bank, const ekv_step *step, int32_t dtype, const float *sinks);
int ekv_sink_step_attend(const ekv_bank *bank, const ekv_step *step, int32_t dtype, const float *sinks, const void *q, const void *k_new,
                         const void *v_new, void *out, int32_t *evict_ids, const float *rope_cos, const float *rope_sin,
                         void *workspace, size_t workspace_bytes, void *stream);

/* Sliding windows (ABI 8, additive): the *_typed calls of a 16-bit bank whose model masks, per layer, the keys that lie a window or
 * more behind the query (gpt-oss: sliding_window = 128 on every other layer).  NORMATIVE.  Every physical K/V row carries the TOKEN
 * POSITION at which it was appended: the count of tokens the sequence had seen before it, 0, 1, 2, ...  This is not the row's logical
 * position in the slot map: eviction is per head, so the same token can be retained in one head and gone in another, and the first
 * attended logical position differs per head.  That is why the position lives with the row and not in a per-launch scalar.
 *
 * A layer has a window W_l >= 0; 0 means no window.  For a query at token position p_q and a live key at token position p_k <= p_q:
 *
 *     the key is attended  iff  W_l == 0  or  p_q - p_k < W_l
 *
 * (transformers' sliding_window_overlay, kv_idx > q_idx - sliding_window).  A masked key's logit is -inf before the maximum, exactly
 * like a causally masked one.  Everything downstream sees p_j and nothing else: the outputs, the column sums, sum p / sum p^2 /
 * counts, the tova row, the GQA mean and every select.  A masked key is still LIVE: it keeps its slot and its score column, receives
 * p = 0 and a count, and may be a victim.  Selection rules, protected windows and tie rules are untouched.  With sinks, the virtual
 * key is never masked.  A query always attends itself (W_l >= 1 keeps p_k = p_q), so no row is empty.
 *
 * tok_pos: DEVICE pointer, int32 [bank->n_layers][n_kv_heads][cap], indexed by PHYSICAL row as a row scale of a kv8 bank is: rows never
 * move, so it is written once, when the row is appended, and no eviction or compaction touches it.  The step writes q_pos0 for the row
 * it appends, at the kernel's own append site (the lane that stores the new K/V row stores its position: no launch of its own, so the
 * plan is the sink call's launch for launch); rows put into the bank by other means must be stamped by the caller.
 * windows: DEVICE pointer, int32 [bank->n_layers], indexed by bank layer.  windows_host: optional HOST copy of the same entries, the
 * only one the library can check: a negative entry is an argument error.  s_aux: the sinks of the sink calls, or NULL for a model without
 * them.  q_pos0: token position of the step's query row, >= 0.  The dry-run calls dereference no device pointer.
 *
 * A window DECODE step plans as the SINK call of the same (bank, step, dtype), with or
 * without sinks: order F, no resident rows (info [9] = 0), the same n_split, launches and workspace.  With every window 0, or every
 * window wider than the sequence, its results are those of the plain call (s_aux == NULL; forced to order F without resident rows) or
 * the sink call, bit for bit.  A window CHUNK step or dense prefix plans as the sink call's (the 16x16x32 kernel alone, blocks of at most
 * 32 GQA-folded rows, info [3] = 0); row i of the step is at token position q_pos0 + i, and the chunk's own keys are subject to the window
 * too (i - i' >= W_l is masked).  The head-averaged TOVA row (tova_head_mean) is rebuilt from the exported logits, whose masked columns
 * are -inf, by the plain or the sink build of its kernel.  Refused before any launch, with ekv_win_workspace_bytes = 0
 * (EKV_E_UNSUPPORTED): rope_on_read, what the sink call refuses, a head_dim other than 128
 * (s_aux == NULL) or 64 (with sinks).  EKV_E_ARG, behind the element type and before anything else is read: a NULL struct, NULL
 * tok_pos / windows, q_pos0 < 0, a negative entry of windows_host.  16-bit rows and single sequences only: there is no window batched,
 * quantised, long or capped call. */
typedef struct ekv_win {
  int32_t *tok_pos;
  const int32_t *windows;
  const int32_t *windows_host;
  const float *s_aux;
  int32_t q_pos0;
} ekv_win;
int ekv_win_step_check(const ekv_bank *bank, const ekv_step *step, int32_t dtype, const ekv_win *win);
int ekv_win_step_info(const ekv_bank *bank, const ekv_step *step, int32_t dtype, const ekv_win *win, int32_t *info, int32_t n_info);
size_t ekv_win_workspace_bytes(const ekv_bank *bank, const ekv_step *step, int32_t dtype, const ekv_win *win);
int ekv_win_step_attend(const ekv_bank *bank, const ekv_step *step, int32_t dtype, const ekv_win *win, const void *q, const void *k_new,
                        const void *v_new, void *out, int32_t *evict_ids, const float *rope_cos, const float *rope_sin,
                        void *workspace, size_t workspace_bytes, void *stream);

/* Pooled selection (ABI 8, additive): the _typed calls with an ekv_pool struct behind the element type.  The one-shot prompt
 * compression of the driver (SnapKV-style: prefill the prompt densely, score the keys with the last few queries, smooth, select once) is a
 * chunk step of q_len = obs queries over n_slots = n keys with n_evict = n - budget whose scorer is pooled.
 *
 * Pooled selection applies to the single-stage policies EKV_POLICY_H2O_HEAD and EKV_POLICY_TOVA, for any n_evict >= 1.
 *   s    the per-KV-head score row the unpooled scorer would rank: after accumulation, after the GQA mean, W = n_slots - score_off columns.
 *   R    the candidate range [win_lo, W - win_tail).
 *   r    the radius, >= 1; the kernel size is 2r + 1.
 * The ranking value of j in R is what torch computes on the slice s[R], and nothing else:
 *   EKV_POOL_MAX   torch.nn.functional.max_pool1d(s[R], 2r+1, stride=1, padding=r).  The padding is -inf, so an edge window simply has
 *                  fewer members.
 *   EKV_POOL_AVG   torch.nn.functional.avg_pool1d(s[R], 2r+1, stride=1, padding=r) with torch's default count_include_pad=True: edge
 *                  windows add zeros and still divide by 2r+1.  The sum is taken in ascending index order, the division is one IEEE
 *                  division by 2r+1.
 * Columns outside R are never pooled into a window and are never victims.  The victims are the n_evict smallest pooled values; ties go
 * to the lowest logical index (the rule of every other select of the library).  A window that holds a NaN pools to NaN and ranks
 * largest.  Everything after the marking is the unpooled scorer's: the compaction of the score rows and of the slot map, evict_ids, the
 * count tails.  The pooled values are used for ranking only: score_sum / score_sq / score_cnt keep the unpooled numbers.
 * EKV_POLICY_ROCO with pooling is refused: its two-stage rule has no single row to pool.
 *
 * One-shot prefill (what the driver issues with generation_config['prefill'] = 'one_shot').  The prompt has n tokens, the resolved
 * integer budget is B < n (B >= n: the key changes nothing), the observation window is obs.
 *   1. Forward A: the tokens [0, n - obs) under the dense unscored plan (policy NONE).  The cache grows to n - obs rows in a bank whose
 *      cap holds the whole prompt.
 *   2. ekv_state_init(n, mode 2), as the strided prefill without keep_attention does.
 *   3. Forward B: the last obs tokens as ONE ordinary chunk step: q_len = obs, causal inside the chunk, accumulate = 1, n_evict = n - B,
 *      win_lo = sink, win_tail = obs (the observation tokens are always kept), count_add = obs, the run's own policy; the scorer is
 *      pooled where score_pool > 1 (these calls), the plain call otherwise.
 *   4. Hand-over: before the first decode step the B retained rows of every head live in a bank sized as the same mode's strided prefill
 *      would have sized it, in logical order in the physical rows [0, B), extent == B; slot map, score rows and (a window bank) tok_pos
 *      carried over; the prompt-sized bank is released.
 *   5. Decode by the mode's existing rule (encoding: plain decode; auto: the decode policy over the whole cache with budget B, on the
 *      score rows forward B left).
 *
 * A pooled step plans as the plain call of the same (bank, step, dtype) with every in-kernel scorer tail switched off, so that it ends in
 * the generic scorer (whose EKV_POOL build it runs): two passes or one pass with exported logits by the plain call's rules, never the
 * one-launch decode step, the split path's fast scorer, the logits-in-LDS kernel, the chunk kernel's tail, the wide column-sum pass's tail
 * or the logits-resident kernel.  Deferred steps (defer_layers) work as for the plain call.  The widest pooled row is the unpooled generic
 * scorer's: the stencil reads the score row where it sits (LDS up to ~10 000 columns, global scratch up to ~38 400) and writes the
 * selection keys, which are in LDS either way; beyond it the step is refused like the plain one.
 * EKV_E_ARG, behind the element type and before anything else is read: a NULL struct, radius < 1, an unknown op.  EKV_E_UNSUPPORTED with
 * zero launches and ekv_pool_workspace_bytes = 0: any policy but H2O_HEAD / TOVA (ROCO, RANGE, NONE), rope_on_read, tova_head_mean,
 * EKV_PHASE_SLOT_ROWS, a row beyond the pooled width.  16-bit rows and single sequences only: there is no pooled batched, quantised,
 * long, capped, sink or window call. */
#define EKV_POOL_MAX 0
#define EKV_POOL_AVG 1
typedef struct ekv_pool {
  int32_t radius;
  int32_t op;
} ekv_pool;
int ekv_pool_step_check(const ekv_bank *bank, const ekv_step *step, int32_t dtype, const ekv_pool *pool);
int ekv_pool_step_info(const ekv_bank *bank, const ekv_step *step, int32_t dtype, const ekv_pool *pool, int32_t *info, int32_t n_info);
size_t ekv_pool_workspace_bytes(const ekv_bank *bank, const ekv_step *step, int32_t dtype, const ekv_pool *pool);
int ekv_pool_step_attend(const ekv_bank *bank, const ekv_step *step, int32_t dtype, const ekv_pool *pool, const void *q, const void *k_new,
                         const void *v_new, void *out, int32_t *evict_ids, const float *rope_cos, const float *rope_sin,
                         void *workspace, size_t workspace_bytes, void *stream);

/* Adaptive head budgets (ABI 8, additive): the _typed calls with an ekv_ada struct behind the element type.  Where a pooled step evicts
 * n_evict rows of every KV head, an adaptive step evicts H * n_evict rows of a LAYER and lets the pooled ranking values decide how many of
 * them each head gives (Ada-KV on SnapKV-style selection): a head with peaked attention keeps few rows, a head with flat attention many.
 *
 * Take one layer.  W = n_slots - score_off, the candidate range is R = [win_lo, W - win_tail), C = |R|.
 *   r_h[j]   the ranking value of candidate j of head h: exactly the pooled selection's (above) for EKV_POLICY_H2O_HEAD / EKV_POLICY_TOVA,
 *            max or avg, radius r, the stencil clipped to R.  New here: radius = 0 means the unpooled score row.
 *   order    the elements of a head are ordered by (key(r_h[j]), j), key = the library's order-preserving float key; NaN ranks largest.
 * Two bounds, in victims per head: 0 <= evict_min <= n_evict <= evict_max <= C.
 *   FORCED      the evict_min smallest elements of every head.
 *   PROTECTED   the C - evict_max largest elements of every head.
 *   FREE        everything else.
 * The layer evicts H * n_evict elements in total: all forced ones, and the H * (n_evict - evict_min) smallest free elements of all heads
 * together, ordered by (key, head, j).  k_h is head h's share of that total, and the victims of head h are exactly its own k_h smallest
 * elements (forced is a subset of them, none is protected, by construction).  Everything behind the marking is the pooled step's:
 * destinations, the compaction of the score rows and of the slot map, the count tails.  Only k is per head: after the step head h has
 * n_slots - k_h rows, and the k_h of a layer sum to H * n_evict.  With evict_min = evict_max = n_evict the step equals the pooled call of
 * the same step bit for bit; with radius = 0 it equals the plain call's generic scorer (n_evict > 1).
 *
 * n_evict_out: device int32 [layer_count][H], row i = layer layer_begin + i of the call; the step writes k_h there (a deferred step: the
 * flush, for all its layers).  evict_ids is [layer_count][H][evict_max]; head h's first k_h entries are written in ascending order of
 * position, the rest is left as it was.  The caller reads n_evict_out (one device-to-host copy) to learn each head's length.
 *
 * An adaptive step plans as the pooled call of the same (bank, step, dtype): every in-kernel scorer tail off, the same tiling, scheme and
 * launches in front — and where the pooled call ends in its scorer launch, three launches: rank (the EKV_ADA build of the generic scorer:
 * accumulates, writes the score rows back, pools, exports a head's W keys and the class of each), allot (one workgroup per layer: a radix
 * select over the free keys of all heads finds the (key, head, j) threshold and writes k_h), select (the same build, entered at the
 * selection with k = k_h).  n_evict never goes through the host in between.  ekv_ada_step_info reports the pooled call's fields with
 * n_launches two higher; ekv_ada_workspace_bytes is the pooled call's plus 5 bytes per (layer, head, padded column).
 * EKV_E_ARG, behind the element type and before anything else is read: a NULL struct, NULL n_evict_out, radius < 0, an unknown op, bounds
 * out of order (evict_min < 0, evict_min > n_evict, n_evict < 1, n_evict > evict_max, evict_max > C).  EKV_E_UNSUPPORTED with zero
 * launches and ekv_ada_workspace_bytes = 0: everything the pooled call refuses (any policy but H2O_HEAD / TOVA, rope_on_read,
 * tova_head_mean, EKV_PHASE_SLOT_ROWS, a row beyond the generic scorer's width) and more than 64 KV heads.  16-bit rows and single
 * sequences only. */
typedef struct ekv_ada {
  int32_t radius;
  int32_t op;
  int32_t evict_min;
  int32_t evict_max;
  int32_t *n_evict_out;
} ekv_ada;
int ekv_ada_step_check(const ekv_bank *bank, const ekv_step *step, int32_t dtype, const ekv_ada *ada);
int ekv_ada_step_info(const ekv_bank *bank, const ekv_step *step, int32_t dtype, const ekv_ada *ada, int32_t *info, int32_t n_info);
size_t ekv_ada_workspace_bytes(const ekv_bank *bank, const ekv_step *step, int32_t dtype, const ekv_ada *ada);
int ekv_ada_step_attend(const ekv_bank *bank, const ekv_step *step, int32_t dtype, const ekv_ada *ada, const void *q, const void *k_new,
                        const void *v_new, void *out, int32_t *evict_ids, const float *rope_cos, const float *rope_sin,
                        void *workspace, size_t workspace_bytes, void *stream);

/* Decode steps over KV heads of different lengths ("heads"; ABI 8, additive): the _typed calls with an ekv_heads struct behind the
 * element type.  A decode step of a multi-layer bank in which every (layer, KV head) holds its own number of rows, as a bank does after
 * adaptive steps.  The counts are read by the kernels from a DEVICE-resident table, so the call has no limit on the number of heads and
 * takes every form the uniform _typed decode call takes: the whole step, the per-layer call phases = 1 | 4 with defer_layers, and the
 * flush phases = 8 over all deferred layers — a ragged bank steps like a uniform one, attention + fold per layer and ONE scorer launch
 * over all heads per token.
 *
 *   rows       DEVICE int32 [bank->n_layers][n_kv_heads], indexed by bank layer: the rows head (l, h) held when the table was written.
 *   rows_host  HOST copy of the same, required.  Every check and every plan reads this copy; ekv_heads_step_check, ekv_heads_step_info
 *              and ekv_heads_workspace_bytes dereference no device pointer.  Read during the call only.
 *   grow       rows every head of the call's layers has gained since the table was written (>= 0).
 *
 * Head (l, h) of the call's layers steps with T = rows[l][h] + grow + 1; the + 1 is the step's own token.  step->n_slots is IGNORED.
 * Every other field of ekv_step keeps its meaning and is shared by the heads (score_off, the selection windows, phys_extent: an extent
 * every head's live rows lie below, or 0 for cap).  n_evict is 0 (every head grows by one row) or 1 (every T stays put).  The call never
 * writes the table: the caller advances `grow`, or rewrites the table when the lengths change in any other way.
 *
 * The launch is the uniform kernels' own (KV head, layer) grid.  Workgroup (h, ll) reads its count with one scalar load, overwrites
 * n_slots in its copy of the argument structs, and is the uniform kernel from there on: per head the arithmetic, and therefore every
 * output bit and every eviction decision, is that of the uniform step of its length under the same n_split and pitches.  A key-range
 * split wholly past a short head's end contributes (m, l, o) = (-inf, 0, 0) to the fold.
 *
 * Planning.  The ENVELOPE is the largest T of the host table over the call's layers, or, for a deferred call, over all defer_layers
 * layers (bank layers layer_begin - defer_index .. + defer_layers), so that the layer calls and the flush agree on every pitch.  A phased
 * or deferred call plans as ekv_step_*_typed of the same step with n_slots = the envelope: same n_split, launch list and workspace.  The
 * whole-step form (phases == 0) plans as that step with phases = 1 | 2 — the split kernel, then the scorer (which folds), or the fold
 * alone where nothing is scored: there is no one-launch build of this family.
 *
 * Accepted: q_len == 1 with plain keys, 16-bit rows, fp16 and bf16, every head_dim of the decode kernels, GQA factors <= 8, the ordered
 * score-row layout, any number of KV heads; scored policies within the split path's fast scorer (at most 6144 slots, cap % 4 == 0).
 * EKV_E_UNSUPPORTED with no launch and ekv_heads_workspace_bytes = 0: q_len > 1, rope_on_read, EKV_PHASE_SLOT_ROWS, tova_head_mean,
 * n_evict > 1, a GQA factor > 8, EKV_POLICY_RANGE with a victim, and scored shapes only the generic scorer serves.  EKV_E_ARG: a NULL
 * struct or pointer, grow < 0, a host count < 1, a resulting T > cap, deferred layers outside the bank, and whatever the uniform step of
 * a head's geometry refuses as EKV_E_ARG. */
typedef struct ekv_heads {
  const int32_t *rows;
  const int32_t *rows_host;
  int32_t grow;
} ekv_heads;
int ekv_heads_step_check(const ekv_bank *bank, const ekv_step *step, int32_t dtype, const ekv_heads *heads);
int ekv_heads_step_info(const ekv_bank *bank, const ekv_step *step, int32_t dtype, const ekv_heads *heads, int32_t *info, int32_t n_info);
size_t ekv_heads_workspace_bytes(const ekv_bank *bank, const ekv_step *step, int32_t dtype, const ekv_heads *heads);
int ekv_heads_step_attend(const ekv_bank *bank, const ekv_step *step, int32_t dtype, const ekv_heads *heads, const void *q,
                          const void *k_new, const void *v_new, void *out, int32_t *evict_ids, void *workspace, size_t workspace_bytes,
                          void *stream);

/* Batched decode steps (ABI 8, additive): ONE call, and one launch per kernel kind, serves n_seq sequences whose caches have
 * different lengths and different eviction geometry.  Each entry of the table names the bank layer it attends and carries what
 * ekv_step holds per step; entry i owns row i of the call's tensors.  The layers of a table need not be contiguous or ordered, so
 * one bank of B * L layers laid out [sequence][layer] gives every sequence an ordinary contiguous L-layer bank for its prefill (the
 * single-sequence calls above) and lets the batched call for model layer l address the layers { s * L + l }.
 *
 *   step   what the batch shares: q_len (must be 1), policy, accumulate, roco_tail, count_add, count_tail_step, sm_div, n_split
 *          (0 = choose) and the row strides.  Its layer_begin, layer_count, n_slots, score_off, n_evict, win_lo, win_tail, roco_k1,
 *          range_start and phys_extent are IGNORED in favour of the table.
 *   seqs   HOST memory, 1 <= n_seq <= EKV_MAX_SEQS entries, read during the call only.  The table travels to the kernels BY VALUE in
 *          their arguments (36 bytes per entry): nothing is staged in device memory, no copy is enqueued and the call never
 *          synchronises with the device.
 *   q, out            16-bit [n_seq][n_q_heads][1][head_dim]
 *   k_new, v_new      16-bit [n_seq][n_kv_heads][1][head_dim]
 *   evict_ids         int32  [n_seq][n_kv_heads][max n_evict of the table] or NULL; rows of entries that evict nothing are not written
 *
 * The step is planned as the uniform step of the table's ENVELOPE (the largest n_slots, the largest phys_extent, layer_count =
 * n_seq): same key-range splits, launches and workspace, so ekv_batch_step_info of a table whose entries are all alike equals
 * ekv_step_info_typed of the multi-layer step it spells out, and ekv_batch_workspace_bytes equals ekv_workspace_bytes_typed of it.
 * Inside those pitches every entry keeps its own bounds: a workgroup serves one (head, entry) as it serves one (head, layer) of a
 * uniform step, with the entry's n_slots, score_off, extent and selection windows — per entry the arithmetic, and therefore every
 * output bit and every eviction decision, is that of the single-sequence step of its geometry under the same n_split.  A key-range
 * split that is empty for a short entry contributes (m, l, o) = (-inf, 0, 0) to the fold.
 *
 * Accepted: q_len == 1 with plain keys, fp16 and bf16, every head_dim, in the whole-step form (phases == 0, defer_layers == 0) on the
 * ordered score-row layout; GQA factors <= 8, at most one victim per entry and step (entries with n_evict 0 and 1 mix freely), at
 * most 6144 slots and cap % 4 == 0 for scored policies — the shapes the one-launch kernel and the split path's fast scorer take.
 * EKV_E_UNSUPPORTED from the dry run, nothing launched: q_len > 1, rope_on_read, any `phases` bit (EKV_PHASE_SLOT_ROWS included),
 * defer_layers, tova_head_mean, and scored shapes only the generic scorer serves.  EKV_E_ARG: n_seq out of range, a `layer` outside
 * the bank or named twice, n_slots outside [1, cap], or entry values the single-sequence step of that geometry refuses as EKV_E_ARG. */
#define EKV_MAX_SEQS 64
typedef struct ekv_seq {      /* one sequence of a batched decode step */
  int32_t layer;        /* bank layer this entry attends                                        */
  int32_t n_slots;      /* T of this sequence, including the new token                          */
  int32_t score_off, n_evict, win_lo, win_tail, roco_k1, range_start, phys_extent;   /* as in ekv_step, per sequence */
} ekv_seq;
int ekv_batch_step_check(const ekv_bank *bank, const ekv_step *step, int32_t dtype, const ekv_seq *seqs, int32_t n_seq);
int ekv_batch_step_info(const ekv_bank *bank, const ekv_step *step, int32_t dtype, const ekv_seq *seqs, int32_t n_seq, int32_t *info,
                        int32_t n_info);
size_t ekv_batch_workspace_bytes(const ekv_bank *bank, const ekv_step *step, int32_t dtype, const ekv_seq *seqs, int32_t n_seq);
int ekv_batch_step_attend(const ekv_bank *bank, const ekv_step *step, int32_t dtype, const ekv_seq *seqs, int32_t n_seq, const void *q,
                          const void *k_new, const void *v_new, void *out, int32_t *evict_ids, void *workspace, size_t workspace_bytes,
                          void *stream);

/* Batched decode steps on a kv8 bank ("kv8 batches"; ABI 8, additive): the ekv_batch_* calls with the descriptor after `dtype`.  The
 * table, the shared step and the call's tensors are those of ekv_batch_step_attend; the bank's rows are the code and scale planes of
 * `kv8` (bank->k / bank->v are not read), and `dtype` is the type of q, k_new, v_new and out.
 *
 * Accepted: the intersection of what a kv8 step and a batched step accept — q_len == 1 with plain keys at head_dim 64 / 128, fp16 and
 * bf16, in the whole-step form (phases == 0, defer_layers == 0) on the ordered score-row layout; GQA factors <= 8, at most one victim
 * per entry and step, at most 6144 slots and cap % 4 == 0 for scored policies.  Planned exactly as ekv_batch_step_attend of the same
 * table (same key-range splits, launches, workspace and info fields) and run on the kv8 builds of the batch instances: per entry the
 * arithmetic is that of ekv_kv8_step_attend of the entry's geometry under the same n_split, the row an entry appends is quantised by
 * the kernel into the row its free list names (codes + scale), and it takes part in the step as quantised.
 * The refusals of both families apply unchanged.  EKV_E_UNSUPPORTED from the dry run, nothing launched and 0 workspace bytes: head_dim
 * 32 / 96, q_len > 1, rope_on_read, any `phases` bit, defer_layers, tova_head_mean, scored shapes only the generic scorer serves.
 * EKV_E_ARG: a NULL descriptor or plane, a dtype other than EKV_DTYPE_F16 / _BF16, and everything ekv_batch_step_check calls a bad table. */
int ekv_kv8_batch_step_check(const ekv_bank *bank, const ekv_step *step, int32_t dtype, const ekv_kv8 *kv8, const ekv_seq *seqs,
                             int32_t n_seq);
int ekv_kv8_batch_step_info(const ekv_bank *bank, const ekv_step *step, int32_t dtype, const ekv_kv8 *kv8, const ekv_seq *seqs,
                            int32_t n_seq, int32_t *info, int32_t n_info);
size_t ekv_kv8_batch_workspace_bytes(const ekv_bank *bank, const ekv_step *step, int32_t dtype, const ekv_kv8 *kv8, const ekv_seq *seqs,
                                     int32_t n_seq);
int ekv_kv8_batch_step_attend(const ekv_bank *bank, const ekv_step *step, int32_t dtype, const ekv_kv8 *kv8, const ekv_seq *seqs,
                              int32_t n_seq, const void *q, const void *k_new, const void *v_new, void *out, int32_t *evict_ids,
                              void *workspace, size_t workspace_bytes, void *stream);

/* Batched decode steps on a kv4 bank ("kv4 batches"; ABI 8, additive): the ekv_kv8_batch_* signatures with the kv4 descriptor.  The
 * table, the shared step and the call's tensors are those of ekv_batch_step_attend; the bank's rows are the code and exponent planes
 * of `kv4` (bank->k / bank->v are not read), and `dtype` is the type of q, k_new, v_new and out.
 *
 * Accepted: the intersection of what a kv4 step and a batched step accept — q_len == 1 with plain keys at head_dim 128, a GQA factor
 * <= 4 (factor 3 on the padded build), fp16 and bf16, in the whole-step form (phases == 0, defer_layers == 0) on the ordered score-row
 * layout; at most EKV_MAX_SEQS entries, at most one victim per entry and step, at most 6144 slots and cap % 4 == 0 for scored
 * policies.  Planned exactly as ekv_batch_step_attend of the same table (same key-range splits, launches, workspace and info fields,
 * fused_order 0) and run on the kv4 builds of the batch instances: per entry the arithmetic is that of ekv_kv4_step_attend of the
 * entry's geometry under the same n_split, the row an entry appends is quantised by its lane group into the row the entry's free list
 * names (codes + block exponents), and it is attended as quantised.  The scorer, the fold and the range compaction behind the
 * attention kernels are the 16-bit batch's: they read logits and partials, never a row.
 * The refusals of both families apply unchanged.  EKV_E_UNSUPPORTED from the dry run, nothing launched and 0 workspace bytes: head_dim
 * != 128, a GQA factor > 4, q_len > 1, rope_on_read, any `phases` bit, defer_layers, tova_head_mean, scored shapes only the generic
 * scorer serves.  EKV_E_ARG: a NULL descriptor or plane, a dtype other than EKV_DTYPE_F16 / _BF16, and everything
 * ekv_batch_step_check calls a bad table. */
int ekv_kv4_batch_step_check(const ekv_bank *bank, const ekv_step *step, int32_t dtype, const ekv_kv4 *kv4, const ekv_seq *seqs,
                             int32_t n_seq);
int ekv_kv4_batch_step_info(const ekv_bank *bank, const ekv_step *step, int32_t dtype, const ekv_kv4 *kv4, const ekv_seq *seqs,
                            int32_t n_seq, int32_t *info, int32_t n_info);
size_t ekv_kv4_batch_workspace_bytes(const ekv_bank *bank, const ekv_step *step, int32_t dtype, const ekv_kv4 *kv4, const ekv_seq *seqs,
                                     int32_t n_seq);
int ekv_kv4_batch_step_attend(const ekv_bank *bank, const ekv_step *step, int32_t dtype, const ekv_kv4 *kv4, const ekv_seq *seqs,
                              int32_t n_seq, const void *q, const void *k_new, const void *v_new, void *out, int32_t *evict_ids,
                              void *workspace, size_t workspace_bytes, void *stream);

/* Batched decode steps on a kv6 bank ("kv6 batches"; ABI 8, additive): the ekv_kv4_batch_* signatures with the kv6 descriptor, with
 * the acceptance, the planning (the 16-bit batched call of the same table, fused_order 0) and the refusals of the kv4 batch calls:
 * EKV_E_UNSUPPORTED from the dry run with nothing launched and 0 workspace bytes, EKV_E_ARG for a NULL descriptor or plane, a dtype
 * other than EKV_DTYPE_F16 / _BF16 and a bad table.  Per entry the arithmetic is that of ekv_kv6_step_attend of the entry's geometry
 * under the same n_split. */
int ekv_kv6_batch_step_check(const ekv_bank *bank, const ekv_step *step, int32_t dtype, const ekv_kv6 *kv6, const ekv_seq *seqs,
                             int32_t n_seq);
int ekv_kv6_batch_step_info(const ekv_bank *bank, const ekv_step *step, int32_t dtype, const ekv_kv6 *kv6, const ekv_seq *seqs,
                            int32_t n_seq, int32_t *info, int32_t n_info);
size_t ekv_kv6_batch_workspace_bytes(const ekv_bank *bank, const ekv_step *step, int32_t dtype, const ekv_kv6 *kv6, const ekv_seq *seqs,
                                     int32_t n_seq);
int ekv_kv6_batch_step_attend(const ekv_bank *bank, const ekv_step *step, int32_t dtype, const ekv_kv6 *kv6, const ekv_seq *seqs,
                              int32_t n_seq, const void *q, const void *k_new, const void *v_new, void *out, int32_t *evict_ids,
                              void *workspace, size_t workspace_bytes, void *stream);

/* Batched decode steps on a kv84 bank ("kv84 batches"; ABI 8, additive): the ekv_kv8_batch_* signatures with the kv84 descriptor, with
 * the acceptance (head_dim 128 only), the planning (the 16-bit batched call of the same table, fused_order 0) and the refusals of the
 * kv8 batch calls: EKV_E_UNSUPPORTED from the dry run with nothing launched and 0 workspace bytes, EKV_E_ARG for a NULL descriptor or
 * plane, a dtype other than EKV_DTYPE_F16 / _BF16 and a bad table.  Per entry the arithmetic is that of ekv_kv84_step_attend of the
 * entry's geometry under the same n_split. */
int ekv_kv84_batch_step_check(const ekv_bank *bank, const ekv_step *step, int32_t dtype, const ekv_kv84 *kv84, const ekv_seq *seqs,
                              int32_t n_seq);
int ekv_kv84_batch_step_info(const ekv_bank *bank, const ekv_step *step, int32_t dtype, const ekv_kv84 *kv84, const ekv_seq *seqs,
                             int32_t n_seq, int32_t *info, int32_t n_info);
size_t ekv_kv84_batch_workspace_bytes(const ekv_bank *bank, const ekv_step *step, int32_t dtype, const ekv_kv84 *kv84,
                                      const ekv_seq *seqs, int32_t n_seq);
int ekv_kv84_batch_step_attend(const ekv_bank *bank, const ekv_step *step, int32_t dtype, const ekv_kv84 *kv84, const ekv_seq *seqs,
                               int32_t n_seq, const void *q, const void *k_new, const void *v_new, void *out, int32_t *evict_ids,
                               void *workspace, size_t workspace_bytes, void *stream);

/* Batched decode steps on a kv164 bank ("kv164 batches"; ABI 8, additive): the ekv_kv8_batch_* signatures with the kv164 descriptor,
 * with the acceptance (head_dim 128 only, every GQA factor of the 16-bit batched call), the planning (the 16-bit batched call of the
 * same table, fused_order 0) and the refusals of the kv84 batch calls: EKV_E_UNSUPPORTED from the dry run with nothing launched and 0
 * workspace bytes, EKV_E_ARG for a NULL descriptor or plane, a NULL bank->k, a dtype other than EKV_DTYPE_F16 / _BF16 and a bad table.
 * Per entry the arithmetic is that of ekv_kv164_step_attend of the entry's geometry under the same n_split. */
int ekv_kv164_batch_step_check(const ekv_bank *bank, const ekv_step *step, int32_t dtype, const ekv_kv164 *kv164, const ekv_seq *seqs,
                               int32_t n_seq);
int ekv_kv164_batch_step_info(const ekv_bank *bank, const ekv_step *step, int32_t dtype, const ekv_kv164 *kv164, const ekv_seq *seqs,
                              int32_t n_seq, int32_t *info, int32_t n_info);
size_t ekv_kv164_batch_workspace_bytes(const ekv_bank *bank, const ekv_step *step, int32_t dtype, const ekv_kv164 *kv164,
                                       const ekv_seq *seqs, int32_t n_seq);
int ekv_kv164_batch_step_attend(const ekv_bank *bank, const ekv_step *step, int32_t dtype, const ekv_kv164 *kv164, const ekv_seq *seqs,
                                int32_t n_seq, const void *q, const void *k_new, const void *v_new, void *out, int32_t *evict_ids,
                                void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* EASYKV_HIP_H */
