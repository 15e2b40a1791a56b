// K1 (+K3+K4 fused): single-token decode over the retained slots.
//
// Replaces easykv/llama_patch.py:198-222 (mistral_patch.py:144-169) for q_len == 1, the K/V append of
// HF DynamicCache.update (call site llama_patch.py:193-196) and, with rope_on_read, the streaming
// rotation of llama_patch.py:310-327.  Two kernels share the streaming loop (ekv_decode_stream.h):
//
//  * ekv_attn_decode_kernel   — one workgroup per (key-range split, KV head, layer); exports logits and
//    (m, l, o) partials to the workspace; ekv_score_select_kernel finishes the step.  Used when a head
//    must be split to fill the chip (layers launched one at a time).
//  * ekv_decode_fused_kernel  — one workgroup per (KV head, layer) does the WHOLE step in one pass:
//    append, QK^T, softmax, PV, GQA fold, score accumulation (easykv/easykv.py:287-300), victim selection
//    (:310-347) and the compaction of the score rows and the slot map (:56-68, :315-333).  Logits and score rows never
//    leave LDS; with plain keys the rows are streamed in physical (address) order and the dead ones masked by a bit per
//    row.  HBM traffic = the algorithmic bytes: K and V once, the score rows once in and once out.
#ifdef EKV_TAIL_PROFILE
#define EKV_STAMP(i) do { if (threadIdx.x == 0) stamps[i] = __builtin_readcyclecounter(); } while (0)
#endif
// Compiled once per EKV_DECODE line of ekv_instances.def (EKV_D, EKV_ROPE, EKV_BF16, EKV_KV8, EKV_BATCH) so the objects build in parallel.
#include "ekv_decode_stream.h"
#include "ekv_decode_tail.h"
// EKV_KV8 = 1 (the kv8 instances): the bank's rows are FP8 codes + fp32 row scales (ekv_decode_stream.h, "FP8 rows"); q, k_new,
// v_new and out keep the 16-bit type of the build.  Only the stream and the per-lane width of the output accumulators differ.
#ifndef EKV_KV8
#define EKV_KV8 0
#endif
// EKV_BATCH = 1 (the batch instances): batched decode steps (include/easykv_hip.h, ekv_seq).  The kernels take the table of the
// batch behind their argument structs; workgroup (head, entry) copies the structs and overwrites the per-step fields with its entry's
// (scalar loads from the kernel arguments), and from there on IS the uniform kernel: pitches (t_pad, l_pad, n_split, rows_per_split,
// LDS sizes, ITEMS) stay the envelope's, bounds (T, extent, score_off, windows) become the entry's, the bank is addressed by the
// entry's layer and the workspace / q / k_new / v_new / out / evict_ids by the entry's index.  Plain keys, ordered score rows.
#ifndef EKV_BATCH
#define EKV_BATCH 0
#endif
// EKV_KV4 = 1 (the kv4 instances, the manifest's kv4 lines): the bank's rows are MXFP4 codes + E8M0 block exponents (ekv_decode_stream.h,
// "MXFP4 rows"); head_dim 128, plain keys, GQA factors up to 4 (a lane's output slice is 32 floats per query head: no REP = 8 build).
#ifndef EKV_KV4
#define EKV_KV4 0
#endif
// EKV_KV6 = 1 (the kv6 instances): MXFP6 codes + E8M0 block exponents (ekv_decode_stream.h, "MXFP6 rows").  The geometry, the rows in
// flight, the occupancy bounds and the GQA limit are the MXFP4 builds' (EKV_MX below); only the stream's piece differs, by its format tag.
#ifndef EKV_KV6
#define EKV_KV6 0
#endif
#if EKV_KV4 || EKV_KV6
#define EKV_MX 1      // one 32-element block per lane
#else
#define EKV_MX 0
#endif
// EKV_KV84 = 1 (the kv84 instances): FP8 keys with MXFP4 values (ekv_decode_stream.h, "FP8-key / MXFP4-value rows").  Geometry, rows in
// flight, occupancy bounds and GQA builds are the FP8 builds' (EKV_G8 below); the stream's V side differs, by its format tag.
#ifndef EKV_KV84
#define EKV_KV84 0
#endif
#if EKV_KV8 || EKV_KV84
#define EKV_G8 1      // the FP8 geometry: 16 elements per lane
#else
#define EKV_G8 0
#endif
// EKV_KV164 = 1 (the kv164 instances): 16-bit keys with MXFP4 values (ekv_decode_stream.h, "16-bit-key / MXFP4-value rows").  Geometry, rows
// in flight, occupancy bounds and GQA builds are the 16-bit builds'; the stream's V side differs, by its format tag, and the resident rows
// and the phase order K of the 16-bit flagship instances are compiled out (kResident, kOrders below).  One exception to "the 16-bit
// builds' rows in flight": the GQA x 1 one-launch builds run 4 rows per lane group, not 8 (EKV_KV164_FUSED_KU1).  With 8 the slot-indexed
// 4-wave build spills 2 VGPRs under its four-workgroup bound and the 8-wave build needs 133 (3 waves per SIMD, the 16-bit build: 128 / 4
// — the exponent words, their scales and the widened codes of 8 rows are live next to the 16-byte K pieces); with 4: 70 .. 103 VGPRs, no
// spill, 4 .. 7 waves per SIMD (profiles/kv164_registers.txt).  The tail takes only the maxima from the stream's partials and the split
// kernel keeps 8 rows, so logits, scores and victims stay the 16-bit step's bit for bit.
#ifndef EKV_KV164
#define EKV_KV164 0
#endif
#ifndef EKV_KV164_FUSED_KU1
#define EKV_KV164_FUSED_KU1 4
#endif
// EKV_SOFTCAP = 1 (the EKV_DECODE_CAP lines of the manifest: 16-bit rows, plain keys, one sequence): every logit is the soft-capped one
// (ekv_softcap, ekv_common.h; EKV_LOGIT at every site that forms q.k / sm_div — the stream, its appended row and the K phase of order K).
// One capped logit per (row, query head) against a 256- or 512-byte row; geometry, rows in flight, phase orders and resident rows are
// the 16-bit builds'.
#if EKV_SOFTCAP && (EKV_ROPE || EKV_KV8 || EKV_KV4 || EKV_KV6 || EKV_KV84 || EKV_KV164 || EKV_BATCH)
#error "soft-capped decode instances: 16-bit rows, plain keys, one sequence"
#endif
// EKV_SINK = 1 (the EKV_DECODE_SINK lines of the manifest: 16-bit rows, plain keys, one sequence, head_dim 64 / 128): attention sinks
// (ekv_common.h).  Both kernels take the sinks as their last argument.  The stream folds the virtual key of every query head into the
// online (m, l, o) of the lane group that scores the appended row, so the partials of the split kernel, both of its folds, the output of
// the one-launch kernel and the maxima its tail takes from the wave partials have it; the tail adds exp(a - M) to the sum it rebuilds from
// the logits (ekv_decode_tail.h).  The phase order K and the resident rows of the 16-bit flagship instances are compiled out, as for
// kv164 (kResident, kOrders below: order K would replay the softmax from the logits in LDS, where the virtual key has no column).
#if EKV_SINK && (EKV_ROPE || EKV_KV8 || EKV_KV4 || EKV_KV6 || EKV_KV84 || EKV_KV164 || EKV_BATCH || EKV_SOFTCAP)
#error "sink decode instances: 16-bit rows, plain keys, one sequence, uncapped logits"
#endif
// EKV_WINDOW = 1 (the EKV_DECODE_WIN lines of the manifest: head_dim 128; with EKV_SINK, the EKV_DECODE_SINK_WIN lines: head_dim 64):
// sliding-window masking (ekv_common.h).  Both kernels take EkvWinArgs as their last argument, behind the sinks, and hand it to the
// stream, which masks a row where it forms its logit and stamps the appended row's token position (ekv_decode_stream.h).  Nothing else
// changes: the tails read -inf logits of live rows, and the folds take partials of (-inf, 0) from a key range that is wholly masked.
// The phase order K and the resident rows are compiled out, as in the sink instances (order K's K phase forms its logits outside the
// stream), so a window instance with every window 0 is the plain (or the sink) instance in order F, bit for bit.
#if EKV_WINDOW && (EKV_ROPE || EKV_KV8 || EKV_KV4 || EKV_KV6 || EKV_KV84 || EKV_KV164 || EKV_BATCH || EKV_SOFTCAP)
#error "window decode instances: 16-bit rows, plain keys, one sequence, uncapped logits"
#endif
#if EKV_WINDOW && !EKV_SINK
#define EKV_WIN_ALONE(...) __VA_ARGS__      // (what a call site spells for the window where the sink build spells it for the sinks)
#else
#define EKV_WIN_ALONE(...)
#endif
// Both switches at once (the batch kv8 instances) are independent: DESIGN.md §3.9, "Batches".
// EKV_HEADS = 1 (the EKV_DECODE_HEADS lines of the manifest: 16-bit rows, plain keys): decode steps over KV heads of different lengths
// (ekv_kernels.h, the third spelling of the shadow macros).  The split kernel alone, with its in-kernel fold: workgroup (split, head, layer)
// takes its head's row count from the device table and is the uniform kernel from there on — a key range wholly past a short head's end
// streams nothing and still stores (-inf, 0, 0) and arrives at the fold, as in the batch builds.  There is no one-launch heads build: the
// objects export no launcher of the fused kernel, so none of its templates is instantiated.
#ifndef EKV_HEADS
#define EKV_HEADS 0
#endif
#if EKV_HEADS && (EKV_ROPE || EKV_KV8 || EKV_KV4 || EKV_KV6 || EKV_KV84 || EKV_KV164 || EKV_BATCH || EKV_SOFTCAP || EKV_SINK || EKV_WINDOW)
#error "heads decode instances: 16-bit rows, plain keys, no batch table, no sinks, no window, uncapped logits"
#endif
#define EKV_HEAD_IDX blockIdx.y
#define ekv_attn_decode_kernel EKV_KERNEL_NAME(ekv_attn_decode_kernel)
#define ekv_decode_fused_kernel EKV_KERNEL_NAME(ekv_decode_fused_kernel)
// FP8 rows: 4 rows in flight per lane group.  A lane's output slice is 16 floats per query head instead of 8, the query fragment
// doubles and a row's widened codes are live next to its bytes: with 8 rows the one-launch build of GQA factor 1 needs 149..214 spilled
// registers under its four-workgroups-per-CU bound, with 4 rows 102..111 VGPRs and none (tools/kernel_regs.py).
// MXFP4 rows: 4 rows in flight as well.  A lane's output slice is 32 floats per query head and its query fragment 16 registers; the
// GQA x 1 one-launch build needs 204..213 VGPRs, which the 8-wave build has (two waves per SIMD) and the 4-wave build gets by running
// two workgroups per CU instead of four (under the four-workgroup bound: 77..235 spilled registers; scheduling barriers between the
// rows' conversions made it 85..277).  GQA x 2 / x 4 spill (profiles/kv4_registers.txt).
#ifndef EKV_SPLIT_KU
#define EKV_SPLIT_KU (EKV_G8 || EKV_MX ? 4 : 8)
#endif
#ifndef EKV_FUSED_KU
#define EKV_FUSED_KU (EKV_G8 || EKV_MX ? 4 : 8)
#endif
#ifndef EKV_ROPE_KU
#define EKV_ROPE_KU(rep) ((rep) == 4 ? 8 : 4)      // rows in flight per lane group of the RoPE-on-read builds (the largest count without spilled VGPRs; rep 8: 8 spilled at 4)
#endif

namespace {

constexpr int kEPL = EKV_MX ? 32 : (EKV_G8 ? 16 : 8);      // elements of a lane's piece of a K/V row (16 bytes; MXFP6: 24)
constexpr int kFMT = EKV_KV6 ? 6 : (EKV_KV84 ? 84 : (EKV_KV164 ? 164 : 0));      // the stream's format tag: what EPL alone does not tell

// SLOT_LDS = false: slot-map entries are fetched per iteration (needs 16-byte aligned map rows, cap % 4 == 0); saves the
// staging pass and its barrier, which matters when a workgroup only streams one or two iterations.
template <int D, int REP, bool ROPE, bool SLOT_LDS>
__global__ void __launch_bounds__(256) ekv_attn_decode_kernel(const EkvAttnArgs EKV_ARG_A EKV_TB_PARAM EKV_SINK_ONLY(, const float* const sinks) EKV_WIN_ONLY(, const EkvWinArgs win) EKV_HEADS_ONLY(, const EkvHeadsArgs heads)) {
  EKV_SHADOW_A(blockIdx.z)
  using Gm = EkvDecodeGeom<D>;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  int32_t* s_slot = reinterpret_cast<int32_t*>(smem);
  float* s_part = reinterpret_cast<float*>(smem + (SLOT_LDS ? ekv_align((size_t)a.rows_per_split * 4, 16) : 0));

  // blockIdx.x = (group of <= REP query heads of the KV head) x (key-range split).  GQA factors up to 8 are ONE group (REP = the
  // factor rounded up to 1 / 2 / 4 / 8, the padding heads repeat the last real one); wider factors run ceil(rep / 8) groups per
  // KV head, each streaming the head's K / V for its own 8 query heads (repeat_kv accepts any factor, llama_patch.py:19-29)
  const int split = blockIdx.x % a.n_split, qgrp = blockIdx.x / a.n_split, h = blockIdx.y, ll = blockIdx.z;
  const int rep_all = a.n_q_heads / a.n_kv_heads;
  const int hq0 = h * rep_all + qgrp * REP;
  const int nrep = (REP == 1 || REP == 2) ? REP : min(REP, rep_all - qgrp * REP);
  const int tid = threadIdx.x;
  const int t0 = split * a.rows_per_split;
  const int t1 = min(a.n_slots, t0 + a.rows_per_split);
  const size_t head_row = ((size_t)(a.layer_begin + ll) * a.n_kv_heads + h) * a.cap;
  if (SLOT_LDS) {
    for (int i = tid; i < t1 - t0; i += 256) s_slot[i] = a.slot_of_pos[head_row + t0 + i];
    __syncthreads();
  }

  float m[REP], l[REP], o[REP][kEPL];
  float* logits = a.logits ? a.logits + ((size_t)ll * a.n_q_heads + hq0) * a.t_pad : nullptr;
  // EKV_SPLIT_KU = 16 would make a 256-row key range (one layer of a decoder stack, split to fill the chip) ONE batch of
  // loads per wave instead of two dependent ones (191 VGPRs, one workgroup per CU anyway).  Measured on the Llama2-7B decode
  // stack, one layer per launch: 14.0 us per layer against 13.7 with 8 — the second round trip is not what bounds the launch
  // (docs/TUNING.md §8, round 3) — so 8 stays.
  constexpr int KU = (!ROPE && !SLOT_LDS && REP <= 2) ? EKV_SPLIT_KU : (EKV_G8 || EKV_MX ? 4 : 8);
  ekv_decode_stream<D, REP, ROPE, SLOT_LDS, 4, false, KU, EkvNoop, kEPL, kFMT>(a, SLOT_LDS ? s_slot : a.slot_of_pos + head_row, logits, a.t_pad,
                                                                               t0, t1, ll, h, head_row, m, l, o, nullptr, EkvNoop(), nrep, hq0
                                                                               EKV_SINK_ONLY(, 0, sinks + (size_t)(a.layer_begin + ll) * a.n_q_heads) EKV_WIN_ALONE(, 0) EKV_WIN_ONLY(, win));

  ekv_decode_wave_combine<D, REP>(m, l, o);
  ekv_decode_stash<D, REP>(s_part, m, l, o);
  __syncthreads();
  const bool fold_here = a.arrive != nullptr;
  for (int idx = tid; idx < REP * D; idx += 256) {
    const int r = idx / D, d = idx % D;
    if (r >= nrep) continue;      // (padding head)
    float mm, ls, os;
    ekv_decode_reduce<D, REP>(s_part, r, d, mm, ls, os);
    float* dst = a.partials + (((size_t)ll * a.n_q_heads + hq0 + r) * a.n_split + split) * Gm::PS;
    if (fold_here) {      // partials another workgroup of this launch will read: write-through stores
      if (d == 0) {
        ekv_store_sc1(dst, mm);
        ekv_store_sc1(dst + 1, ls);
      }
      ekv_store_sc1(dst + 2 + d, os);
    } else {
      if (d == 0) {
        dst[0] = mm;
        dst[1] = ls;
      }
      dst[2 + d] = os;
    }
  }
  if (!fold_here) return;
  // ---- in-kernel fold: the LAST split of the head to arrive folds the partials of all splits into the fp16 output (what
  // ekv_fold_kernel does in a launch of its own: 1.5-2 us of kernel boundary + a 4 us latency-bound kernel on the critical path
  // of every layer of a decoder stack).  Protocol (MI355X_MICROARCH.md "inter-workgroup visibility"): sc1 partial stores,
  // every wave drains its stores, barrier, ONE agent-scope atomicAdd on the head's arrival counter (bank->arrive, zeroed by
  // ekv_bank_reset; the last arriver leaves it at zero again); the last arriver reads the partials with sc1 loads.
  // (First version: a CAS loop on an epoch-tagged word in the workspace, so that nothing had to be zero-initialised: 17 splits
  // arriving together retried for 25 us.)
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  uint32_t* s_last = reinterpret_cast<uint32_t*>(s_part);      // (the wave partials have been consumed)
  if (tid == 0) {
    uint32_t* word = a.arrive + (size_t)EKV_ARRIVE_ROW(ll) * a.n_kv_heads + h;
    // This is the guide's write-through hand-off in its counter form (cdna_hip_programming.md §5 "in-launch split-K reduction":
    // sc1 slab stores -> EVERY wave asm vmcnt(0) -> __syncthreads -> lane 0 relaxed agent fetch_add; the reducer reads the slabs
    // with sc1 loads): the sc1 stores have left the XCD's L2 before the counter moves, and sc1 loads bypass the reader's L1, so
    // no release / acquire fence is needed (a fence pair would cost ~3.4 us on a 12 us launch).  A launch that dies mid-way can
    // leave the counter non-zero: ekv_bank_reset and KVBank.abort_step() zero it.
    const uint32_t old = __hip_atomic_fetch_add(word, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const bool last = (int)(old + 1u) == a.n_split;
    if (last) __hip_atomic_store(word, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    *s_last = last ? 1u : 0u;
  }
  __syncthreads();
  if (*s_last == 0u) return;
  // descriptor over this layer's partials (wave-uniform base), per-lane element offsets
  const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(
      a.partials + (size_t)ll * a.n_q_heads * a.n_split * Gm::PS, 0, (int)((size_t)a.n_q_heads * a.n_split * Gm::PS * 4), 0x00020000);
  for (int idx = tid; idx < nrep * D; idx += 256) {      // (the in-kernel fold is only used with ONE query-head group per KV head)
    const int r = idx / D, d = idx % D;
    const size_t row = (size_t)ll * a.n_q_heads + hq0 + r;
    a.out_direct[row * D + d] = ekv_to_e(ekv_fold_partials_buf_auto(rsrc, (unsigned)((hq0 + r) * a.n_split * Gm::PS), a.n_split, Gm::PS, d));
  }
}

// ------------------------------------------------------------------------------------------------------
// fused kernel
// ------------------------------------------------------------------------------------------------------
// The 8-wave 5-column flagship build (16-bit rows, head_dim 128, GQA x 1, slot-indexed rows: the one with both phase orders that a
// launch of more than 512 heads runs in two rounds) must fit TWO workgroups on a CU: four waves per SIMD, 128 VGPRs.  The second
// launch bound counts waves per SIMD; every other 8-wave build of GQA factor 1 keeps 2 (the soft-capped one too: under 128 VGPRs it
// spills six, so it keeps order F alone and its code).
#define EKV_FUSED_TWO_PER_CU(D, ROPE, ITEMS, SLOT) \
  ((D) == 128 && !(ROPE) && (SLOT) && (ITEMS) <= 5 && !EKV_G8 && !EKV_MX && !EKV_KV164 && !EKV_BATCH && !EKV_SINK && !EKV_WINDOW && !EKV_SOFTCAP)
template <int D, int REP, bool ROPE, int ITEMS, int NW, bool SLOT>
__global__ void __launch_bounds__(64 * NW, (NW >= 8 ? (REP == 1 ? (EKV_FUSED_TWO_PER_CU(D, ROPE, ITEMS, SLOT) ? 4 : 2) : 1) : (SLOT && ITEMS > 12 ? 2 : (REP == 1 ? (EKV_MX ? 2 : 4) : (REP == 2 ? 3 : 2))))) ekv_decode_fused_kernel(const EkvAttnArgs EKV_ARG_A, const EkvScoreArgs EKV_ARG_SC EKV_TB_PARAM EKV_SINK_ONLY(, const float* const sinks) EKV_WIN_ONLY(, const EkvWinArgs win) EKV_HEADS_ONLY(, const EkvHeadsArgs heads)) {
  EKV_SHADOW_A(blockIdx.z)
  EKV_SHADOW_SC(blockIdx.z)
  using Gm = EkvDecodeGeom<D, NW>;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int h = blockIdx.y, ll = blockIdx.z, tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int T = a.n_slots;
  // REP = the GQA factor rounded up to 1 / 2 / 4 / 8; nrep = the factor itself (3, 5, 6, 7: the padding heads repeat the last real
  // one in the stream and stay out of the GQA mean and of the output)
  const int nrep = (REP == 1 || REP == 2) ? REP : a.n_q_heads / a.n_kv_heads;
  const bool roco = sc.policy == EKV_POLICY_ROCO;
  const bool scored = roco || sc.policy == EKV_POLICY_H2O_HEAD || sc.policy == EKV_POLICY_TOVA;
  const int off = scored ? sc.score_off : 0;
  // SLOT: the score rows are indexed by physical row [0, E) like the logits (ekv_decode_tail.h, "slot-indexed score rows")
  const int W = SLOT ? a.phys_extent : T - off;
  const int w_pad = (int)ekv_align((size_t)W, 256);
  // Plain keys: stream the rows in PHYSICAL order (ekv_decode_stream.h); RoPE-on-read needs the position index of a row.
#ifdef EKV_NO_PHYS
  constexpr bool PHYS = false;   // A/B build: position-ordered gather through the slot map
#else
  constexpr bool PHYS = !ROPE;
#endif
  const int l_pad = a.l_pad;   // pitch of a logits row: physical rows [0, E) (PHYS) or positions [0, T)
  // Resident rows (ekv_decode_stream.h, "load policy"): the 16-bit instances of the flagship geometry — head_dim 128, one query head
  // per KV head, slot-indexed score rows, both phase orders, 4 and 8 waves, every column count.  Every other instance keeps its code.
  constexpr bool kResident = D == 128 && REP == 1 && PHYS && SLOT && !EKV_G8 && !EKV_MX && !EKV_KV164 && !EKV_BATCH && !EKV_SINK && !EKV_WINDOW;
  const int res_rows = kResident ? EKV_RESIDENT_ROWS(a.fused_order) : 0;
  // LDS: logits [REP][l_pad] | wave partials [4][REP][PS] | score rows S (Q C) [w_pad] | reduction scratch | dead-row bits
  float* s_logit = reinterpret_cast<float*>(smem);
  float* s_part = s_logit + (size_t)REP * l_pad;
  float* sS = s_part + (size_t)Gm::NP * REP * Gm::PS + ((Gm::NP * REP * Gm::PS) & 3 ? 4 - ((Gm::NP * REP * Gm::PS) & 3) : 0);
  float* sQ = sS + w_pad;
  float* sC = sQ + w_pad;
  RedN<NW> red;
  red.buf = reinterpret_cast<unsigned long long*>(sS + (size_t)(roco ? (SLOT ? 2 : 3) : 1) * w_pad);
  red.phase = 0;
  red.lane = lane;
  red.wave = wave;
  const size_t head_row = ((size_t)(a.layer_begin + ll) * a.n_kv_heads + h) * a.cap;
#ifdef EKV_TAIL_PROFILE
  unsigned long long* stamps = reinterpret_cast<unsigned long long*>(sc.tova_row) + ((size_t)ll * a.n_kv_heads + h) * 8;
#endif
  EKV_STAMP(0);
  // ---- phase order of this workgroup (kOrders instances; a.fused_order: ekv_kernels.h).  Order F, what every other instance does:
  // stream K+V, then the tail.  Order K: stream K, run the tail on the logits, stream V and replay the online softmax from the logits
  // in LDS.  The tail is a latency-bound chain of block barriers that leaves HBM idle; when the workgroups of a CU are in different
  // orders, each order's tail falls under the other's stream.  Both orders produce the same bits (below), so WHICH workgroups take
  // order K may depend on where the hardware placed them.
  // 8-wave workgroups (not the soft-capped builds) have both orders too: the plane loop, the KEEP tail and the V replay are written
  // over NW, and a launch of more than two of them per CU runs in dispatch rounds (rule source 3 below).  ITEMS 5: extents up to 2304
  // rows.  Extents up to 6144 rows: the 12-column build keeps order F alone and its code — with both orders in it, its order F ran 4 %
  // slower (118.9 -> 124.0 us at 512 heads x 2561 rows: 78 scalar registers spilled, 36 bytes of scratch) — and a launch that asks
  // for order K there runs a build of its own, ITEMS 13 (launch_fused_nw).
  constexpr bool kOrders = D == 128 && REP == 1 && !ROPE && ((NW == 4 && ITEMS <= 12) || (NW == 8 && !EKV_SOFTCAP && (ITEMS <= 5 || ITEMS == 13))) && SLOT && !EKV_G8 && !EKV_MX && !EKV_KV164 && !EKV_BATCH && !EKV_SINK && !EKV_WINDOW;
  bool order_k = false;
  if constexpr (kOrders) {
    const int om = a.fused_order & 3;
    if (om == 2) {
      order_k = scored;
    } else if (om == 1 && scored) {
      // one number per workgroup, from wave 0 (uniform by construction: the other waves read it from LDS, not from their own registers)
      uint32_t* s_flag = reinterpret_cast<uint32_t*>(red.buf);
      if (tid == 0) {
        const uint32_t hw = __builtin_amdgcn_s_getreg(63492);   // HW_REG_HW_ID: WAVE_ID [3:0], TG_ID [19:16]
        const int src = (a.fused_order >> 4) & 3;
        const uint32_t x = src == 0 ? (hw >> 16) & 15u : (src == 1 ? hw & 15u : (uint32_t)(ll * a.n_kv_heads + h));
        bool below = (x & ((a.fused_order >> 8) & 15u)) < ((a.fused_order >> 12) & 15u);
        // Source 3 (the 8-wave instances; the 4-wave ones keep their code and read it as source 2), the rule by dispatch round:
        // workgroups are dispatched in grid order, so on a launch that runs in rounds the position in the grid, not the hardware
        // slot, says who ends last.  The two nibbles are one threshold, (mask << 4 | bound) * EKV_ORDER_ROUND_UNIT workgroups.
        if constexpr (NW == 8)
          if (src == 3) below = x < (uint32_t)EKV_ORDER_ROUND_THRESHOLD(a.fused_order);
        *s_flag = below != (((a.fused_order >> 6) & 1) != 0) ? 1u : 0u;
      }
      __syncthreads();
      order_k = __builtin_amdgcn_readfirstlane((int)*s_flag) != 0;
    }
  }
  const int32_t* slot_row = a.slot_of_pos + head_row;
  uint32_t* s_deadw = reinterpret_cast<uint32_t*>(red.buf + 2 * NW * 8);
  // ---- score rows -> LDS by asynchronous LDS-DMA, hidden inside the K/V stream (the ragged end follows after the stream) ----
  if (scored) ekv_tail_prefetch_rows<NW, false>(sc, head_row, W, w_pad, roco, sS, sQ, sC, !SLOT);
  float g_old = 0.f, c_new = 0.f;
  int nb = 0;
  // The 8-wave instances with both orders have 128 VGPRs for two workgroups per CU and none to carry the three numbers across the
  // stream: they are requested behind it, with the count bases and births (the tail reads all of them after its softmax passes).
  // Every other instance keeps the statements where they were (and its device code).
  constexpr bool kLateHeadState = kOrders && NW == 8;
  // (the appended entry starts from the count the ordered row holds behind its live entries — 0 after decode steps — minus the
  //  running offset: count = base + g)
#define EKV_HEAD_STATE()                                                                  \
  do {                                                                                    \
    const size_t head = (size_t)(a.layer_begin + ll) * a.n_kv_heads + h;                  \
    g_old = sc.slot_state[4 * head];                                                      \
    nb = reinterpret_cast<const int32_t*>(sc.slot_state)[4 * head + 1];                   \
    c_new = sc.cnt_tail[head_row + T - 1] - g_old;                                        \
  } while (0)
  if (SLOT && !kLateHeadState) {
    const size_t head = (size_t)(a.layer_begin + ll) * a.n_kv_heads + h;
    g_old = sc.slot_state[4 * head];
    nb = reinterpret_cast<const int32_t*>(sc.slot_state)[4 * head + 1];
    c_new = sc.cnt_tail[head_row + T - 1] - g_old;
  }
  // Dead-row bits of the physical rows [0, align(E, 128)): the padding past the extent, the free rows (slot-map entries
  // [T, cap)) and the row the new token is being written to (entry T-1; ekv_decode_stream scores it from k_new / v_new).
  // The free-list entry of this thread is loaded NOW and applied inside the stream, after the first K/V loads are in flight.
  const int E = a.phys_extent;
  const int fl_idx = T - 1 + tid;
  int fl = 0;
  if (PHYS) {
    fl = slot_row[min(fl_idx, a.cap - 1)];
    const int n_words = (int)ekv_align((size_t)E, 128) / 32;
    for (int i = tid; i < n_words; i += 64 * NW)
      s_deadw[i] = i * 32 >= E ? ~0u : (i * 32 + 32 > E ? ~0u << (E & 31) : 0u);
  }
  auto mask_ready = [&]() {
    ekv_lds_barrier();     // (LDS-only barriers: the K/V loads of the first iteration stay in flight across them)
    if (fl_idx < a.cap && fl < E) atomicOr(&s_deadw[fl >> 5], 1u << (fl & 31));
    for (int i = fl_idx + 64 * NW; i < a.cap; i += 64 * NW) {   // free lists longer than the workgroup: rare
      const int row = slot_row[i];
      if (row < E) atomicOr(&s_deadw[row >> 5], 1u << (row & 31));
    }
    ekv_lds_barrier();
  };

  if constexpr (kOrders) {
    if (order_k) {
      constexpr int LPR = Gm::LPR;
      const int sub = lane % LPR, grp = lane / LPR;
      const int new_row = slot_row[T - 1];
      const uint8_t* s_dead = reinterpret_cast<const uint8_t*>(s_deadw);
      // ---- K phase: raw logits of the live rows -> LDS at the physical row index (a logit depends on its row alone), running maximum
      const uint4 qv = reinterpret_cast<const uint4*>(a.q + ((size_t)ll * a.n_q_heads + h) * D)[sub];
      float mk = EKV_NEG_INF;
      ekv_decode_plane_loop<D, NW, kResident>(a.k, head_row, E, mask_ready, [&](uint4 (&kr)[8], const int j0) {
        const unsigned dead8 = (unsigned)s_dead[j0 >> 3];
        float s[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const float acc = ekv_group_sum<LPR>(ekv_dot8(qv, kr[u], 0.f));
          s[u] = !((dead8 >> u) & 1u) ? EKV_LOGIT(acc, a) : EKV_NEG_INF;
        }
        float mine = s[0];
#pragma unroll
        for (int u = 1; u < 8; ++u) mine = (sub == u) ? s[u] : mine;
        if (sub < 8 && !((dead8 >> sub) & 1u)) s_logit[j0 + sub] = mine;
#pragma unroll
        for (int u = 0; u < 8; ++u) mk = fmaxf(mk, s[u]);
      }, res_rows);
      // the appended row: written to the bank (K and V) and scored from k_new, as in ekv_decode_stream
      const __half* v_new_row = a.v_new + ((size_t)ll * a.n_kv_heads + h) * D;
      if (wave == 0 && grp == 0) {
        const uint4 kn = reinterpret_cast<const uint4*>(a.k_new + ((size_t)ll * a.n_kv_heads + h) * D)[sub];
        const uint4 vn = reinterpret_cast<const uint4*>(v_new_row)[sub];
        const size_t off_new = (head_row + new_row) * D;
        reinterpret_cast<uint4*>(a.k_w + off_new)[sub] = kn;
        reinterpret_cast<uint4*>(a.v_w + off_new)[sub] = vn;
        const float acc = EKV_LOGIT(ekv_group_sum<LPR>(ekv_dot8(qv, kn, 0.f)), a);
        if (sub == 0) s_logit[new_row] = acc;
        mk = fmaxf(mk, acc);
      }
      ekv_tail_prefetch_ragged<NW>(sc, head_row, W, roco, sS, sQ, sC, false);
      if constexpr (kLateHeadState) EKV_HEAD_STATE();
      float cC[ITEMS];
      int32_t cB[ITEMS];
#pragma unroll
      for (int it = 0; it < ITEMS; ++it) {
        const int j = min(tid + it * 64 * NW, a.cap - 1);
        cC[it] = roco ? sc.score_cnt[head_row + j] : 0.f;
        cB[it] = sc.birth[head_row + j];
      }
      EKV_STAMP(1);
      // the wave maxima where the tail looks for them (the maximum is exact in any order); the rest of s_part is the tail's candidate list
      mk = ekv_wave_max(mk);
      if (lane == 0) s_part[(size_t)wave * Gm::PS] = mk;
      __syncthreads();  // publishes the maxima, s_logit and (vmcnt(0) before the barrier) the DMA'd score rows
      uint32_t* s_hist = s_deadw + ekv_align(ekv_align((size_t)l_pad, 128) / 32, 4);
      ekv_decode_tail_slot<REP, ITEMS, NW, true>(sc, ll, h, head_row, T, E, s_logit, l_pad, sS, sQ, cC, cB, red, s_hist,
                                                 reinterpret_cast<unsigned long long*>(s_part), Gm::NP * REP * Gm::PS / 2, s_part, Gm::NP,
                                                 Gm::PS, s_deadw, new_row, g_old, c_new, nb, nrep);
      EKV_STAMP(2);
      // ---- V phase: the fused loop's rows, in its order, with its online softmax — s[u] read back instead of computed, so (m, l, o)
      // go through the same floating-point operations as in order F and the output is bit-identical
      float m[1] = {EKV_NEG_INF}, l[1] = {0.f}, o[1][8];
#pragma unroll
      for (int i = 0; i < 8; ++i) o[0][i] = 0.f;
      ekv_decode_plane_loop<D, NW, kResident>(a.v, head_row, E, EkvNoop(), [&](uint4 (&vr)[8], const int j0) {
        const unsigned dead8 = (unsigned)s_dead[j0 >> 3];
        float s[8];
        if (dead8 == 0xFFu) {      // (nothing live here; past the extent there are no logits to read either)
#pragma unroll
          for (int u = 0; u < 8; ++u) s[u] = EKV_NEG_INF;
        } else {
          const float4 s0 = *reinterpret_cast<const float4*>(s_logit + j0), s1 = *reinterpret_cast<const float4*>(s_logit + j0 + 4);
          s[0] = s0.x, s[1] = s0.y, s[2] = s0.z, s[3] = s0.w, s[4] = s1.x, s[5] = s1.y, s[6] = s1.z, s[7] = s1.w;
        }
        if (dead8 != 0u) {
#pragma unroll
          for (int u = 0; u < 8; ++u)
            if ((dead8 >> u) & 1u) {
              vr[u] = uint4{0, 0, 0, 0};
              s[u] = EKV_NEG_INF;
            }
        }
        float mx = s[0];
#pragma unroll
        for (int u = 1; u < 8; ++u) mx = fmaxf(mx, s[u]);
        const float mn = fmaxf(m[0], mx);
        if (mn == EKV_NEG_INF) return;
        const float alpha = exp2f((m[0] - mn) * EKV_LOG2E);
        l[0] *= alpha;
#pragma unroll
        for (int i = 0; i < 8; ++i) o[0][i] *= alpha;
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const float p = exp2f((s[u] - mn) * EKV_LOG2E);
          l[0] += p;
          ekv_axpy8(p, vr[u], o[0]);
        }
        m[0] = mn;
      }, res_rows);
      if (wave == 0 && grp == 0) {      // the appended row, last, as in ekv_decode_stream
        const uint4 vn = reinterpret_cast<const uint4*>(v_new_row)[sub];
        const float acc = s_logit[new_row];
        const float mn = fmaxf(m[0], acc);
        const float alpha = m[0] == EKV_NEG_INF ? 0.f : exp2f((m[0] - mn) * EKV_LOG2E);
        const float p = exp2f((acc - mn) * EKV_LOG2E);
        l[0] = l[0] * alpha + p;
#pragma unroll
        for (int i = 0; i < 8; ++i) o[0][i] *= alpha;
        ekv_axpy8(p, vn, o[0]);
        m[0] = mn;
      }
      ekv_decode_wave_combine<D, 1>(m, l, o);
      ekv_decode_stash<D, 1, NW>(s_part, m, l, o);
      __syncthreads();
      for (int d = tid; d < D; d += 64 * NW) {
        float mm, ls, os;
        ekv_decode_reduce<D, 1, NW>(s_part, 0, d, mm, ls, os);
        sc.out[((size_t)ll * a.n_q_heads + h) * D + d] = ekv_to_e(os / ls);
      }
      EKV_STAMP(5);
#ifdef EKV_TAIL_PROFILE
      if (tid == 0) {
        stamps[3] = 1;
        stamps[6] = __builtin_amdgcn_s_getreg(63492);
        stamps[7] = __builtin_amdgcn_s_getreg(63508);
      }
#endif
      return;
    }
  }

  // rows in flight per lane group: 8 for plain keys (REP = 1: neutral against 4, round 3; REP = 8: 114 vs 117 us despite 3..6 spilled
  // registers).  RoPE-on-read builds (EKV_ROPE_KU): rounds 1-5 kept 16 table floats per row next to the K / V registers (8 rows in flight
  // spilled 19 registers in the Llama-shape build: 284 us; 4 rows 221 us); since round 6 one (cos, sin) seed per iteration + 16 step
  // constants (ekv_decode_stream.h) — 124 VGPRs at 4 rows (46 spilled at 8), GQA x 2 144 (13 spilled at 8), GQA x 4 230 at 8 rows
  // without spills, GQA x 8 (per-row tables) 247
  constexpr int KUF = ROPE ? EKV_ROPE_KU(REP) : (EKV_KV164 && REP == 1 ? EKV_KV164_FUSED_KU1 : EKV_FUSED_KU);
  float m[REP], l[REP], o[REP][kEPL];
  EKV_SINK_ONLY(const float* const sink_row = sinks + (size_t)(a.layer_begin + ll) * a.n_q_heads;)      // (the sinks of this bank layer)
  if (PHYS)
    ekv_decode_stream<D, REP, ROPE, false, NW, PHYS, KUF, decltype(mask_ready), kEPL, kFMT, kResident>(a, slot_row, s_logit, l_pad, 0, T, ll, h, head_row, m, l, o,
                                                     reinterpret_cast<const uint8_t*>(s_deadw), mask_ready, nrep, h * nrep, res_rows EKV_SINK_ONLY(, sink_row) EKV_WIN_ONLY(, win));
  else
    ekv_decode_stream<D, REP, ROPE, false, NW, false, KUF, EkvNoop, kEPL, kFMT>(a, slot_row, s_logit, l_pad, 0, T, ll, h, head_row, m, l, o, nullptr,
                                                      EkvNoop(), nrep, h * nrep EKV_SINK_ONLY(, 0, sink_row) EKV_WIN_ALONE(, 0) EKV_WIN_ONLY(, win));
  if (scored) ekv_tail_prefetch_ragged<NW>(sc, head_row, W, roco, sS, sQ, sC, !SLOT);   // published by the barrier below
  // SLOT: count base and birth of this thread's rows, straight into registers (consumed after the softmax passes of the tail)
  float cC[SLOT ? ITEMS : 1];
  int32_t cB[SLOT ? ITEMS : 1];
  if (SLOT) {
    if constexpr (kLateHeadState) EKV_HEAD_STATE();
#pragma unroll
    for (int it = 0; it < (SLOT ? ITEMS : 1); ++it) {
      const int j = min(tid + it * 64 * NW, a.cap - 1);
      cC[it] = roco ? sc.score_cnt[head_row + j] : 0.f;
      cB[it] = sc.birth[head_row + j];
    }
  }

  EKV_STAMP(1);
  ekv_decode_wave_combine<D, REP>(m, l, o);
  ekv_decode_stash<D, REP, NW>(s_part, m, l, o);
  __syncthreads();  // publishes s_part, s_logit and (vmcnt(0) before the barrier) the DMA'd score rows
  for (int idx = tid; idx < nrep * D; idx += 64 * NW) {
    const int r = idx / D, d = idx % D;
    float mm, ls, os;
    ekv_decode_reduce<D, REP, NW>(s_part, r, d, mm, ls, os);
    sc.out[((size_t)ll * a.n_q_heads + h * nrep + r) * D + d] = ekv_to_e(os / ls);
  }

  // scratch of the roco select: histogram behind the dead-row bits; the candidate list reuses the wave partials (dead by now,
  // and every path through the tail passes a barrier before the list is written)
  uint32_t* s_hist = s_deadw + ekv_align(ekv_align((size_t)l_pad, 128) / 32, 4);
  if constexpr (SLOT) {
    ekv_decode_tail_slot<REP, ITEMS, NW>(sc, ll, h, head_row, T, E, s_logit, l_pad, sS, sQ, cC, cB, red, s_hist,
                                         reinterpret_cast<unsigned long long*>(s_part), Gm::NP * REP * Gm::PS / 2, s_part, Gm::NP, Gm::PS,
                                         s_deadw, slot_row[T - 1], g_old, c_new, nb, nrep EKV_SINK_ONLY(, sink_row + h * nrep));
  } else {
    ekv_decode_tail<REP, ITEMS, NW, PHYS>(sc, ll, h, head_row, T, off, W, s_logit, l_pad, sS, sQ, sC, red, s_hist,
                                          reinterpret_cast<unsigned long long*>(s_part), Gm::NP * REP * Gm::PS / 2, s_part, Gm::NP, Gm::PS, nrep
                                          EKV_SINK_ONLY(, sink_row + h * nrep));
  }
  EKV_STAMP(5);
#ifdef EKV_TAIL_PROFILE
  if (tid == 0) {
    stamps[6] = __builtin_amdgcn_s_getreg(63492);   // HW_REG_HW_ID
    stamps[7] = __builtin_amdgcn_s_getreg(63508);   // HW_REG_XCC_ID
  }
#endif
}

#undef EKV_HEAD_STATE

template <int REP>
hipError_t launch(const EkvAttnArgs& a EKV_TB_DECL EKV_SINK_ONLY(, const float* sinks) EKV_WIN_ONLY(, const EkvWinArgs& win) EKV_HEADS_ONLY(, const EkvHeadsArgs& heads), int layer_count, hipStream_t s) {
  using Gm = EkvDecodeGeom<EKV_D>;
  const size_t part = (size_t)Gm::NP * REP * Gm::PS * 4;
  const int rep_all = a.n_q_heads / a.n_kv_heads;
  const dim3 grid(a.n_split * ((rep_all + REP - 1) / REP), a.n_kv_heads, layer_count);
  if ((a.cap & 3) == 0 && a.cap >= 16) {
    hipLaunchKernelGGL((ekv_attn_decode_kernel<EKV_D, REP, EKV_ROPE, false>), grid, dim3(256), part, s, a EKV_TB_PASS EKV_SINK_ONLY(, sinks) EKV_WIN_ONLY(, win) EKV_HEADS_ONLY(, heads));
  } else {
    const size_t lds = ekv_align((size_t)a.rows_per_split * 4, 16) + part;
    if (lds > 48 * 1024)
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&ekv_attn_decode_kernel<EKV_D, REP, EKV_ROPE, true>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL((ekv_attn_decode_kernel<EKV_D, REP, EKV_ROPE, true>), grid, dim3(256), lds, s, a EKV_TB_PASS EKV_SINK_ONLY(, sinks) EKV_WIN_ONLY(, win) EKV_HEADS_ONLY(, heads));
  }
  return hipGetLastError();
}

#if !EKV_HEADS      // (no one-launch heads build)
template <int REP, int NW = 8>
size_t fused_lds(int t_pad, int l_pad, int n_state) { return ekv_fused_lds<EKV_D, REP, NW>(t_pad, l_pad, n_state); }

template <int REP, int ITEMS, int NW, bool SLOT>
hipError_t launch_fused_k(const EkvAttnArgs& a, const EkvScoreArgs& sc EKV_TB_DECL EKV_SINK_ONLY(, const float* sinks) EKV_WIN_ONLY(, const EkvWinArgs& win), int layer_count, hipStream_t s) {
  // (slot-indexed rows: S / Q over the physical rows [0, E) in LDS, count base and birth in registers)
  const size_t lds = SLOT ? fused_lds<REP, NW>(a.phys_extent, a.l_pad, sc.policy == EKV_POLICY_ROCO ? 2 : 1)
                          : fused_lds<REP, NW>(a.t_pad, a.l_pad, sc.policy == EKV_POLICY_ROCO ? 3 : 1);
  if (lds > 48 * 1024)
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&ekv_decode_fused_kernel<EKV_D, REP, EKV_ROPE, ITEMS, NW, SLOT>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL((ekv_decode_fused_kernel<EKV_D, REP, EKV_ROPE, ITEMS, NW, SLOT>), dim3(1, a.n_kv_heads, layer_count),
                     dim3(64 * NW), lds, s, a, sc EKV_TB_PASS EKV_SINK_ONLY(, sinks) EKV_WIN_ONLY(, win));
  return hipGetLastError();
}

// NW = waves per workgroup of the fused kernel; ITEMS = ceil(max row width / threads).
//   NW = 4: four workgroups per CU when every CU gets >= 4 heads (Llama2-7B shape: 1024 heads per 32-layer launch).
//   NW = 8: for launches with only 1-2 heads per CU (GQA: Mistral's 8 KV heads x 32 layers = 256 heads): the same number
//           of waves per CU streams one head, instead of leaving the CU to a single 4-wave workgroup.
template <int REP, int NW>
hipError_t launch_fused_nw(const EkvAttnArgs& a, const EkvScoreArgs& sc EKV_TB_DECL EKV_SINK_ONLY(, const float* sinks) EKV_WIN_ONLY(, const EkvWinArgs& win), int layer_count, hipStream_t s) {
  constexpr int NT = 64 * NW, I0 = (2304 + NT - 1) / NT, I1 = (6144 + NT - 1) / NT;
  if (sc.birth != nullptr) {      // slot-indexed rows: the thread-owned columns are the physical rows [0, E) (ekv_decode_slot_rows_supported)
    if constexpr (!EKV_ROPE && !EKV_BATCH && REP <= 4) {      // (a batch runs on the ordered layout)
      if (a.phys_extent <= NT * I0) return launch_fused_k<REP, I0, NW, true>(a, sc EKV_TB_PASS EKV_SINK_ONLY(, sinks) EKV_WIN_ONLY(, win), layer_count, s);
      // extents up to 6144 rows: 12 (8-wave) / 24 (4-wave) columns per thread in registers; the 4-wave build gives up the fourth
      // workgroup per CU for them (LDS would not have allowed it at these row counts anyway)
      // (8 waves, 16-bit rows, head_dim 128, one query head per KV head: a launch that asks for order K at these extents runs the
      //  13-column build, the one that has both orders there; the 12-column build stays what it was)
      if constexpr (NW == 8 && REP == 1 && EKV_D == 128 && !EKV_G8 && !EKV_MX && !EKV_KV164 && !EKV_SINK && !EKV_WINDOW && !EKV_SOFTCAP)
        if ((a.fused_order & 3) != 0 && a.phys_extent <= NT * I1) return launch_fused_k<REP, I1 + 1, NW, true>(a, sc EKV_TB_PASS EKV_SINK_ONLY(, sinks) EKV_WIN_ONLY(, win), layer_count, s);
      if (a.phys_extent <= NT * I1) return launch_fused_k<REP, I1, NW, true>(a, sc EKV_TB_PASS EKV_SINK_ONLY(, sinks) EKV_WIN_ONLY(, win), layer_count, s);
    }
    return hipErrorInvalidValue;
  }
  if (a.n_slots <= NT * I0) return launch_fused_k<REP, I0, NW, false>(a, sc EKV_TB_PASS EKV_SINK_ONLY(, sinks) EKV_WIN_ONLY(, win), layer_count, s);
  return launch_fused_k<REP, I1, NW, false>(a, sc EKV_TB_PASS EKV_SINK_ONLY(, sinks) EKV_WIN_ONLY(, win), layer_count, s);
}
template <int REP>
hipError_t launch_fused(const EkvAttnArgs& a, const EkvScoreArgs& sc EKV_TB_DECL EKV_SINK_ONLY(, const float* sinks) EKV_WIN_ONLY(, const EkvWinArgs& win), int layer_count, int nw, hipStream_t s) {
  return nw == 8 ? launch_fused_nw<REP, 8>(a, sc EKV_TB_PASS EKV_SINK_ONLY(, sinks) EKV_WIN_ONLY(, win), layer_count, s) : launch_fused_nw<REP, 4>(a, sc EKV_TB_PASS EKV_SINK_ONLY(, sinks) EKV_WIN_ONLY(, win), layer_count, s);
}

#endif

}  // namespace

#if EKV_HEADS
// the heads instances: their launcher takes the table's pointer and growth where the others take the table of a batch (EKV_FN_HEADS:
// element type, head_dim); GQA factors up to 8, one query-head group per KV head (the planner refuses wider ones)
hipError_t EKV_FN_HEADS(ekv_launch_attn_decode, EKV_ELEM, EKV_D)(const EkvAttnArgs& a, const EkvHeadsArgs& hd, int rep, int layer_count, hipStream_t s) {
  if (rep < 1 || rep > 8 || hd.rows == nullptr) return hipErrorInvalidValue;
  switch (rep) {
    case 1: return launch<1>(a, hd, layer_count, s);
    case 2: return launch<2>(a, hd, layer_count, s);
    case 3: case 4: return launch<4>(a, hd, layer_count, s);
    default: return launch<8>(a, hd, layer_count, s);
  }
}
#elif EKV_WINDOW
// the window instances (EKV_FN_WIN; with sinks EKV_FN_SINK_WIN): one signature for both, `sinks` unused (NULL) in the window-alone ones
#if EKV_SINK
#define EKV_WSYM(fn) EKV_FN_SINK_WIN(fn, EKV_ELEM, EKV_D)
#else
#define EKV_WSYM(fn) EKV_FN_WIN(fn, EKV_ELEM, EKV_D)
#endif
hipError_t EKV_WSYM(ekv_launch_attn_decode)(const EkvAttnArgs& a, const float* sinks, const EkvWinArgs& win, int rep, int layer_count, hipStream_t s) {
  if (rep < 1 || (sinks == nullptr) != !EKV_SINK || win.tok_pos == nullptr || win.windows == nullptr) return hipErrorInvalidValue;
  switch (rep) {
    case 1: return launch<1>(a EKV_SINK_ONLY(, sinks), win, layer_count, s);
    case 2: return launch<2>(a EKV_SINK_ONLY(, sinks), win, layer_count, s);
    case 3: case 4: return launch<4>(a EKV_SINK_ONLY(, sinks), win, layer_count, s);
    default: return launch<8>(a EKV_SINK_ONLY(, sinks), win, layer_count, s);
  }
}

hipError_t EKV_WSYM(ekv_launch_decode_fused)(const EkvAttnArgs& a, const EkvScoreArgs& sc, const float* sinks, const EkvWinArgs& win, int rep,
                                             int layer_count, int nw, hipStream_t s) {
  if ((sinks == nullptr) != !EKV_SINK || win.tok_pos == nullptr || win.windows == nullptr) return hipErrorInvalidValue;
  switch (rep) {
    case 1: return launch_fused<1>(a, sc EKV_SINK_ONLY(, sinks), win, layer_count, nw, s);
    case 2: return launch_fused<2>(a, sc EKV_SINK_ONLY(, sinks), win, layer_count, nw, s);
    case 3: case 4: return launch_fused<4>(a, sc EKV_SINK_ONLY(, sinks), win, layer_count, nw, s);
    case 5: case 6: case 7: case 8: return launch_fused<8>(a, sc EKV_SINK_ONLY(, sinks), win, layer_count, nw, s);
    default: return hipErrorInvalidValue;
  }
}
#elif EKV_SINK
// the sink instances: their launchers take the sinks where the others take the table of a batch (EKV_FN_SINK: element type, head_dim)
hipError_t EKV_FN_SINK(ekv_launch_attn_decode, EKV_ELEM, EKV_D)(const EkvAttnArgs& a, const float* sinks, int rep, int layer_count, hipStream_t s) {
  if (rep < 1 || sinks == nullptr) return hipErrorInvalidValue;
  switch (rep) {
    case 1: return launch<1>(a, sinks, layer_count, s);
    case 2: return launch<2>(a, sinks, layer_count, s);
    case 3: case 4: return launch<4>(a, sinks, layer_count, s);
    default: return launch<8>(a, sinks, layer_count, s);
  }
}

hipError_t EKV_FN_SINK(ekv_launch_decode_fused, EKV_ELEM, EKV_D)(const EkvAttnArgs& a, const EkvScoreArgs& sc, const float* sinks, int rep,
                                                                 int layer_count, int nw, hipStream_t s) {
  if (sinks == nullptr) return hipErrorInvalidValue;
  switch (rep) {
    case 1: return launch_fused<1>(a, sc, sinks, layer_count, nw, s);
    case 2: return launch_fused<2>(a, sc, sinks, layer_count, nw, s);
    case 3: case 4: return launch_fused<4>(a, sc, sinks, layer_count, nw, s);
    case 5: case 6: case 7: case 8: return launch_fused<8>(a, sc, sinks, layer_count, nw, s);
    default: return hipErrorInvalidValue;
  }
}
#else
#if EKV_SOFTCAP
#define EKV_KEYS cap      // (plain keys, soft-capped logits)
#elif EKV_ROPE
#define EKV_KEYS rope
#else
#define EKV_KEYS plain
#endif
#define EKV_SYM(fn) EKV_FN_DECODE(fn, EKV_D, EKV_KEYS, EKV_ELEM, EKV_ROWS, EKV_BATCHING)

// tb: the table of a batched step for the batch instances, unused (NULL) otherwise
hipError_t EKV_SYM(ekv_launch_attn_decode)(const EkvAttnArgs& a, const EkvSeqTable* tb, int rep, int layer_count, hipStream_t s) {
  if (rep < 1) return hipErrorInvalidValue;
  switch (rep) {
    case 1: return launch<1>(a EKV_TB_DEREF, layer_count, s);
    case 2: return launch<2>(a EKV_TB_DEREF, layer_count, s);
    case 3: case 4: return launch<4>(a EKV_TB_DEREF, layer_count, s);
#if EKV_MX
    default: return hipErrorInvalidValue;      // (no REP = 8 build: 256 output registers per lane)
#else
    default: return launch<8>(a EKV_TB_DEREF, layer_count, s);      // 5..8: one group of 8; wider factors: ceil(rep / 8) groups per KV head
#endif
  }
}

hipError_t EKV_SYM(ekv_launch_decode_fused)(const EkvAttnArgs& a, const EkvScoreArgs& sc, const EkvSeqTable* tb, int rep, int layer_count,
                                            int nw, hipStream_t s) {
  switch (rep) {
    case 1: return launch_fused<1>(a, sc EKV_TB_DEREF, layer_count, nw, s);
    case 2: return launch_fused<2>(a, sc EKV_TB_DEREF, layer_count, nw, s);
    case 3: case 4: return launch_fused<4>(a, sc EKV_TB_DEREF, layer_count, nw, s);
#if !EKV_MX
    case 5: case 6: case 7: case 8: return launch_fused<8>(a, sc EKV_TB_DEREF, layer_count, nw, s);
#endif
    default: return hipErrorInvalidValue;
  }
}
#endif
