// K2: strided-prefill chunk attention (q_len = n > 1) over the retained slots, MFMA 16x16x32 f16 / bf16.
// Compiled once per (EKV_D, EKV_CHUNK_MODE, element type) by the ekv_attn_chunk_d*.hip stubs; the bf16 instances (EKV_BF16)
// build plain keys only (the hi / lo fp16 planes of RoPE-on-read are fp16 by design).
//
// Replaces easykv/llama_patch.py:198-222 (mistral_patch.py:144-169) for q_len = stride (and the dense
// prefix prefill, q_len = r_idx), the K/V append of DynamicCache.update (llama_patch.py:193-196) and,
// with rope_on_read, llama_patch.py:310-327.
//
// One workgroup (4 waves) per (key-range split x query block, KV head, layer).  K/V super-tiles of 64
// positions are staged global -> registers -> LDS (loads of tile t+1 are issued before tile t is
// consumed; rows are 16 B per lane, coalesced along head-dim, gathered through the slot map).
// Waves: wk = wave&1 owns 32 of the 64 keys, wq = wave>>1 owns the query tiles {wq, wq+2, ...};
// a query tile is 16 rows of the (rep x n) GQA-folded query block, so the K/V tile is read from HBM
// once for all query heads of the group.
//   S^T[key][q] = K_tile . Q^T     A = K rows (ds_read_b128), B = Q rows (global/L1)
//   O^T[d][q]  += V^T . P^T        A = V column gathers (8 x ds_read_u16), B = P^T straight from the S^T
//                                   accumulators (key slot (g,e) <-> keys {4g+e, 16+4g+e}: no shuffle)
// Softmax is online per query (exp2), the running max is shared by the 4 lane groups of a query with two
// cross-lane steps per tile.  Raw logits (-inf where causally masked) are exported for the scorer.
// Arithmetic intensity is rep*n flop/B << the ~300 flop/B ridge: HBM-bound; MFMA is the instruction, not
// the bound (SURVEY.md §8d).
//
// EKV_CHUNK_MODE (one per translation unit):
//   0  one pass, online softmax, raw logits exported for the scorer (small query blocks: the logits are a few % of K/V)
//   1  statistics pass of the two-pass scheme: K only, per-row (max, sum exp) partials, nothing else
//   2  exact pass of the two-pass scheme: with the final row statistics p = exp(s - M)/L is exact on the fly, so the
//      kernel accumulates O += P.V without rescaling AND the per-key column sums  sum_i pbar_ij, sum_i pbar_ij^2  of the
//      GQA-folded probabilities (easykv/easykv.py:443-457) right from the MFMA accumulators; the rep x n x T logits
//      (as large as K+V at rep*n = 64..128) never touch HBM.  Costs one extra read of K.
#include <algorithm>
#include <type_traits>

#include "ekv_common.h"
#include "ekv_kernels.h"
// EKV_SOFTCAP = 1 (the EKV_CHUNK_CAP lines of the manifest): soft-capped logits (ekv_softcap, ekv_common.h).  Every accumulator element
// of S^T becomes s = cap * tanh((q.k / sm_div) / cap) before the causal mask, the running maximum and the exponent, in all three modes and
// by the same operations: the quotient (the reference's, as the exported logits have it), then ekv_softcap.  So the capped builds never
// fold 1 / sm_div into the exponent (need_div below is always on), the statistics pass and the exact pass see the same s from the same
// accumulators, and what leaves the kernel — logits, (m, l, o) partials, row statistics, column sums — is in capped units.  Plain keys, the
// one-tile build alone (blocks of <= 32 folded rows, as head_dim 256 plans them: ekv_chunk_blocks), at head_dim 128 and 256.
#ifndef EKV_SOFTCAP
#define EKV_SOFTCAP 0
#endif
// EKV_SINK = 1 (the EKV_CHUNK_SINK lines of the manifest): attention sinks (ekv_common.h).  The kernel takes the sinks as its last argument;
// the wave that owns the first key half of the first split (split 0, wk 0: ONE of the 2 * n_split partials of a query row) starts the row's
// running (m, l) at (a, 1) in lane group 0 instead of (-inf, 0), in the one pass and in the statistics pass alike, so partials, the
// in-kernel fold, the row statistics, the statistics the exact pass folds and with them its probabilities and column sums all carry the
// virtual key.  The exact pass, whose partials are sums of normalised probabilities, adds the virtual key's own probability to the same
// lane's sum (its value is 0: the output gains nothing).  Plain keys, the one-tile build alone (as the capped instances), head_dim 64 / 128.
#if EKV_SINK && EKV_SOFTCAP
#error "sink chunk instances: uncapped logits"
#endif
// EKV_WINDOW != 0 (the EKV_CHUNK_WIN lines of the manifest, head_dim 128; = 2, with sinks, the EKV_CHUNK_SINK_WIN lines, head_dim 64): sliding-
// window masking (ekv_common.h).  The kernel takes EkvWinArgs as its last argument, behind the sinks.  Logical order is monotone in token
// position (the slot map keeps birth order), so the keys a query does not attend are a PREFIX of the logical positions: every lane finds
// the first attended position of its query row once, before the tile loop — a binary search over the token positions of the cached rows
// (slot map -> tok_pos, ~log2 T dependent pairs of loads per workgroup lifetime), joined with the bound among the chunk's own keys, whose
// positions are q_pos0 + i' (i - i' >= W is masked) — and the tile loop masks j < that bound next to the causal j >= jlim, under a
// wave-uniform test that keeps the compares out of every tile past the wave's largest bound.  The mask sits before the running maximum
// and the export, so all three modes, the exported logits, the row statistics, the partials and the column sums carry it; a (split, row)
// whose keys are all masked leaves the floor maximum and a zero sum, as a causally empty one does.  The rows the launch appends are
// stamped with their token positions at the append site.  Plain keys, the one-tile build alone (as the sink instances).
#if EKV_WINDOW && EKV_SOFTCAP
#error "window chunk instances: uncapped logits"
#endif
#if EKV_WINDOW && EKV_SINK && EKV_BF16
#define ekv_attn_chunk_kernel ekv_attn_chunk_kernel_sink_win_bf16
#elif EKV_WINDOW && EKV_SINK
#define ekv_attn_chunk_kernel ekv_attn_chunk_kernel_sink_win
#elif EKV_WINDOW && EKV_BF16
#define ekv_attn_chunk_kernel ekv_attn_chunk_kernel_win_bf16
#elif EKV_WINDOW
#define ekv_attn_chunk_kernel ekv_attn_chunk_kernel_win
#elif EKV_BF16   // (bf16 instances: the same kernel under a tagged name)
#if EKV_SOFTCAP
#define ekv_attn_chunk_kernel ekv_attn_chunk_kernel_cap_bf16
#elif EKV_SINK
#define ekv_attn_chunk_kernel ekv_attn_chunk_kernel_sink_bf16
#else
#define ekv_attn_chunk_kernel ekv_attn_chunk_kernel_bf16
#endif
#elif EKV_SOFTCAP
#define ekv_attn_chunk_kernel ekv_attn_chunk_kernel_cap
#elif EKV_SINK
#define ekv_attn_chunk_kernel ekv_attn_chunk_kernel_sink
#endif

#if EKV_CHUNK_MODE == 0
// FUSE: an unsplit head's scorer (exact softmax of the exported logits, accumulate, select, compaction) runs as the tail of the
// workgroup that streamed the head — same code as ekv_score_select_kernel, 256 threads
#define EKV_SS_NT 256
#define EKV_SS_DEVICE_ONLY
#include "ekv_score_select.inc"
#endif

// P operand of the PV product: one fp16 per probability (what the reference's own GPU path multiplies with: softmax(...).to(fp16),
// llama_patch.py:218) or an fp16 pair hi + lo (~2^-21).  The single form halves the PV MFMAs; outputs stay within the 1e-3 bound
// of the parity tests with a factor ~4 to spare (|error| <= 2^-12 * sum_j p_j |v_j|).
#ifndef EKV_CHUNK_PSPLIT
#define EKV_CHUNK_PSPLIT 0
#endif

// Query block in LDS or in registers (QPW x D/32 x 4 VGPRs per wave, a third of the LDS reads of a tile less).  Registers where
// they fit: the 1-tile variants, and every variant of the statistics pass (no output accumulators).
#define EKV_Q_LDS(qpw, rope, nw) (EKV_CHUNK_MODE == 1 ? ((rope) && (qpw) >= 2) : ((nw) == 8 || ((qpw) >= 2 && (rope))))

namespace {

typedef float ekv_f4 __attribute__((ext_vector_type(4)));
typedef float ekv_f2 __attribute__((ext_vector_type(2)));

// All-reduce (sum) of 16 values over the 16 lanes of each DPP row, in place.  hipcc fuses only a fifth of the
// `x += update_dpp(x)` steps into v_add_f32_dpp and emits v_mov_b32_dpp + v_add_f32 for the rest (160 + 116 of the ~1000 VALU
// instructions of a two-tile round of the exact pass); written out, it is one instruction per step and value.  Steps are
// value-major within a step, so a DPP source was written 16 instructions earlier (the 2 wait states a DPP read needs after a
// VALU write are covered; s_nop 1 covers the first step against whatever the compiler scheduled just before).
__device__ __forceinline__ void ekv_row_sum16(float (&x)[8], float (&y)[8]) {
#define EKV_RS_STEP(ctl)                                                                                                        \
  "v_add_f32_dpp %0, %0, %0 " ctl " row_mask:0xf bank_mask:0xf\n v_add_f32_dpp %1, %1, %1 " ctl " row_mask:0xf bank_mask:0xf\n"   \
  "v_add_f32_dpp %2, %2, %2 " ctl " row_mask:0xf bank_mask:0xf\n v_add_f32_dpp %3, %3, %3 " ctl " row_mask:0xf bank_mask:0xf\n"   \
  "v_add_f32_dpp %4, %4, %4 " ctl " row_mask:0xf bank_mask:0xf\n v_add_f32_dpp %5, %5, %5 " ctl " row_mask:0xf bank_mask:0xf\n"   \
  "v_add_f32_dpp %6, %6, %6 " ctl " row_mask:0xf bank_mask:0xf\n v_add_f32_dpp %7, %7, %7 " ctl " row_mask:0xf bank_mask:0xf\n"   \
  "v_add_f32_dpp %8, %8, %8 " ctl " row_mask:0xf bank_mask:0xf\n v_add_f32_dpp %9, %9, %9 " ctl " row_mask:0xf bank_mask:0xf\n"   \
  "v_add_f32_dpp %10, %10, %10 " ctl " row_mask:0xf bank_mask:0xf\n v_add_f32_dpp %11, %11, %11 " ctl " row_mask:0xf bank_mask:0xf\n" \
  "v_add_f32_dpp %12, %12, %12 " ctl " row_mask:0xf bank_mask:0xf\n v_add_f32_dpp %13, %13, %13 " ctl " row_mask:0xf bank_mask:0xf\n" \
  "v_add_f32_dpp %14, %14, %14 " ctl " row_mask:0xf bank_mask:0xf\n v_add_f32_dpp %15, %15, %15 " ctl " row_mask:0xf bank_mask:0xf\n"
  asm volatile("s_nop 1\n" EKV_RS_STEP("quad_perm:[1,0,3,2]") EKV_RS_STEP("quad_perm:[2,3,0,1]") EKV_RS_STEP("row_half_mirror")
                   EKV_RS_STEP("row_mirror")
               : "+v"(x[0]), "+v"(x[1]), "+v"(x[2]), "+v"(x[3]), "+v"(x[4]), "+v"(x[5]), "+v"(x[6]), "+v"(x[7]), "+v"(y[0]), "+v"(y[1]),
                 "+v"(y[2]), "+v"(y[3]), "+v"(y[4]), "+v"(y[5]), "+v"(y[6]), "+v"(y[7]));
#undef EKV_RS_STEP
}

__device__ __forceinline__ float ekv_max3(float x, float y, float z) {
  float r;
  asm("v_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(x), "v"(y), "v"(z));
  return r;
}

constexpr int kKT = 64;   // positions per super-tile
constexpr int kPadH = 16;  // LDS row padding in halfs (32 B): conflict-free ds_read_b128 row gathers AND ds_read_b64_tr_b16 of 4 rows x 32 B

// NW = 4: 2 x 2 waves (wk x wq), up to 2 workgroups per CU, one K/V tile in flight per workgroup.
// NW = 16: 2 x 8 waves x ONE query tile for query blocks of 65..128 rows without rope-on-read (one-pass kernel only):
//         the same 128 rows per workgroup as NW = 8, but <= 128 VGPRs per wave, i.e. four waves per SIMD; Q operands in registers.
// NW = 8: 2 x 4 waves for query blocks of 65..128 rows: every wave still owns only QPW = 2 query tiles (the 4-tile
//         variant of a 4-wave workgroup needs > 256 registers, and a single scratch reload inside the tile loop waits
//         for the prefetched K/V loads as well, which serialises the stream), one workgroup per CU, two tiles in flight.
template <int QPW, bool ROPE, int NW, bool FUSE = false>
// (the statistics pass has no output accumulators: <= 128 VGPRs, so two 8-wave workgroups per CU — two workgroups drift out of
// phase and their VALU / LDS / MFMA phases overlap, which the lock-stepped waves of ONE workgroup never do)
__global__ void __launch_bounds__(64 * NW, (NW == 16 || (NW == 8 && EKV_CHUNK_MODE != 1)) ? 1 : 2) ekv_attn_chunk_kernel(const EkvAttnArgs a, const EkvScoreArgs sc EKV_SINK_ONLY(, const float* const sinks) EKV_WIN_ONLY(, const EkvWinArgs win)) {
  constexpr int D = EKV_D;
  constexpr int MODE = EKV_CHUNK_MODE;
  constexpr int NT = 64 * NW;               // threads
  constexpr int NWQ = NW / 2;               // waves along the query tiles
  constexpr int PF = NW == 8 ? 2 : 1;       // K/V super-tiles in flight (register staging sets)
  constexpr int PPR = D / 8;                // 16-byte pieces per row
  // pieces are dealt to threads in rows of PPT slots: PPT = PPR, except head_dim 96 where a row takes 16 slots of which 12 hold a
  // piece — the RoPE rotation exchanges a piece with the one D/2 further inside ONE wave, so a row must not straddle waves
  constexpr int PPT = (PPR & (PPR - 1)) ? 16 : PPR;
  constexpr int LPT = (kKT * PPT + NT - 1) / NT;   // piece slots per thread per tensor per super-tile
  constexpr int RS = D + kPadH;             // LDS row stride (halfs)
  constexpr int KB = D / 32;                // MFMA k-steps of QK^T
  constexpr int DB = D / 16;                // d-blocks of O^T
  constexpr int PS = D + 2;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  int32_t* s_slot = reinterpret_cast<int32_t*>(smem);
  ekv_e* sK = reinterpret_cast<ekv_e*>(smem + ekv_align((size_t)a.rows_per_split * 4, 16));
  ekv_e* sV = sK + kKT * RS;
  ekv_e* sKl = sV + (MODE == 1 ? 0 : kKT * RS);   // (the statistics pass stages no V tile)  ROPE only: low part of the rotated keys (k' = hi + lo, ~2^-21 relative)
  // The query block lives in LDS (or, for the 1-tile variant, in registers) for the whole kernel.  Loading the Q operands
  // from global memory inside the tile loop is doubly bad: vmcnt retires in order, so waiting for a Q operand also waits
  // for the K/V tile prefetched just before it (no overlap left), and a 128-row block does not even fit L1.
  constexpr bool Q_LDS = EKV_Q_LDS(QPW, ROPE, NW);   // otherwise the Q operands stay in registers (Q_REG below)
  constexpr int QROWS = 16 * QPW * NWQ;
  ekv_e* sQh = sKl + (ROPE ? kKT * RS : 0);
  ekv_e* sQl = sQh + QROWS * RS;   // ROPE only

  const int n = a.q_len, T = a.n_slots;
  const int rep = a.n_q_heads / a.n_kv_heads;
  // heads fastest: the query blocks of one (head, key range) get linear workgroup ids n_kv_heads apart — the same XCD when
  // n_kv_heads is a multiple of 8 (workgroup -> XCD is id % 8), dispatched together — so the K/V tiles the second block reads
  // are in that XCD's L2
  // Query blocks in DESCENDING order: block b of a causal prefix streams (b + 1) x qb_rows keys, and workgroups are dispatched in id
  // order — longest first leaves the short ones to fill the tail.
  const int qb = a.n_qblocks - 1 - (int)(blockIdx.y % a.n_qblocks), split = blockIdx.y / a.n_qblocks;
  const int h = blockIdx.x, ll = blockIdx.z;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // (scalar: wave-uniform tests
                                                                                                  //  become s_cbranch, not exec masks)
  const int g = lane >> 4, c = lane & 15;
  const int wk = wave & 1, wq = wave >> 1;
  const int i0 = qb * a.qb_rows, nb = min(a.qb_rows, n - i0);   // queries [i0, i0+nb) of the chunk
  const int NR = rep * nb;                                      // rows of this block: row = (i-i0)*rep + r
  const int t0 = split * a.rows_per_split;
  const int t1 = min(min(T, t0 + a.rows_per_split), T - n + i0 + nb);   // causal bound of the block
  const size_t head_row = ((size_t)(a.layer_begin + ll) * a.n_kv_heads + h) * a.cap;
  const int t_new = T - n;                                      // first position of the chunk itself
  const int nse = a.n_split * 2;
  const float inv_sm_div = 1.f / a.sm_div;
  // The exported logits, the row statistics the scorer reads and the probabilities of the exact pass are built on the reference's
  // quotients s / sqrt(D).  A launch that only produces the attention output, and the statistics pass (whose row maximum is
  // converted exactly at the end: the quotient of the maximum IS the maximum of the quotients), work on the raw accumulators.
  const bool need_div = EKV_SOFTCAP || MODE == 2 || a.logits != nullptr || a.row_stats != nullptr;      // (capped builds: always — the cap takes the quotient)
  const float cexp = need_div ? EKV_LOG2E : EKV_LOG2E * inv_sm_div;
  constexpr float kMFloor = -1.0e30f;

  for (int i = tid; i < t1 - t0; i += NT) s_slot[i] = a.slot_of_pos[head_row + t0 + i];
  if (Q_LDS) {
    for (int piece = tid; piece < QROWS * PPR; piece += NT) {
      const int row = piece / PPR, sub = piece % PPR;
      uint4 qh = {0, 0, 0, 0}, ql = {0, 0, 0, 0};
      if (row < NR) {
        // (the rotated queries of ekv_rope_q_kernel are dense; the caller's own rows sit at ekv_step.q_*_stride)
        const size_t qoff = (((size_t)ll * a.n_q_heads + h * rep + row % rep) * n + i0 + row / rep) * D;
        const size_t qsrc = (size_t)ll * a.n_q_heads * n * D + (size_t)(h * rep + row % rep) * a.q_hs + (size_t)(i0 + row / rep) * a.q_ts;
        qh = reinterpret_cast<const uint4*>(ROPE ? a.q_rot_hi + qoff : a.q + qsrc)[sub];
        if (ROPE) ql = reinterpret_cast<const uint4*>(a.q_rot_lo + qoff)[sub];
      }
      *reinterpret_cast<uint4*>(sQh + row * RS + sub * 8) = qh;
      if (ROPE) *reinterpret_cast<uint4*>(sQl + row * RS + sub * 8) = ql;
    }
  }
  __syncthreads();

  // per-wave state ---------------------------------------------------------------------------------
  ekv_f4 oacc[QPW][DB];
  float m_run[QPW], l_run[QPW], inv_l[QPW];
  int row_r[QPW], row_i[QPW];   // (query head in group, query index in chunk) of this lane's query column
  bool row_ok[QPW];
#pragma unroll
  for (int t = 0; t < QPW; ++t) {
    const int row = (wq + NWQ * t) * 16 + c;
    row_ok[t] = row < NR;
    row_r[t] = row_ok[t] ? row % rep : 0;        // the rep query heads of one query sit in adjacent lanes
    row_i[t] = row_ok[t] ? i0 + row / rep : i0;
    m_run[t] = EKV_NEG_INF;
    l_run[t] = 0.f;
#pragma unroll
    for (int db = 0; db < DB; ++db) oacc[t][db] = ekv_f4{0.f, 0.f, 0.f, 0.f};
    if (MODE == 2) {
      // final statistics of this lane's query row: fold the (max, sum exp) partials of the statistics pass
      float mm = EKV_NEG_INF, ls = 0.f;
      if (row_ok[t]) {
        const float* sp = a.stats + (((size_t)ll * a.n_q_heads + h * rep + row_r[t]) * n + row_i[t]) * nse * 2;
        for (int i = 0; i < nse; ++i) mm = fmaxf(mm, sp[2 * i]);
        for (int i = 0; i < nse; ++i) {
          const float mi = sp[2 * i];
          if (mi != EKV_NEG_INF) ls += sp[2 * i + 1] * exp2f((mi - mm) * EKV_LOG2E);
        }
      }
      m_run[t] = row_ok[t] ? mm : 0.f;          // MODE 2: m_run = M (fixed), inv_l = 1/L (0 for rows past the block)
      inv_l[t] = row_ok[t] ? 1.f / ls : 0.f;
    }
  }

#if EKV_SINK
  // attention sinks: the virtual key of this lane's query row, counted once per row — in lane group 0 of the wave that owns the first key
  // half of the first split.  m_run is in the units of this launch's logits (raw accumulators unless need_div).  In raw units the seed is
  // fl(a * sm_div), which the conversion at the end takes back to fl(fl(a * sm_div) / sm_div): where the sink is the row's maximum the
  // exported M may differ from a by an ulp, while the exact pass forms the sink's own probability from a itself — a relative 1e-7 on that
  // one term, not bit-for-bit agreement between the two passes on it (the real keys' terms do agree: both passes use the exported M).
  if (split == 0 && wk == 0) {
#pragma unroll
    for (int t = 0; t < QPW; ++t) {
      const float sink_a = sinks[(size_t)(a.layer_begin + ll) * a.n_q_heads + h * rep + row_r[t]];
      if (MODE == 2) {      // (m_run = M and inv_l = 1 / L have the virtual key: the statistics pass seeded it)
        if (row_ok[t] && g == 0) l_run[t] = exp2f((sink_a - m_run[t]) * EKV_LOG2E) * inv_l[t];
      } else {
        m_run[t] = need_div ? sink_a : sink_a * a.sm_div;
        l_run[t] = g == 0 ? 1.f : 0.f;
      }
    }
  }
#endif

#if EKV_WINDOW
  // sliding window: win_lo[t] = first logical position this lane's query attends (0: no window here); win_lo_wave = the wave's largest
  const int win_w = win.windows[a.layer_begin + ll];
  int win_lo[QPW], win_lo_wave = 0;
#pragma unroll
  for (int t = 0; t < QPW; ++t) {
    int lo = 0;
    if (win_w > 0 && row_ok[t]) {
      const int pq = win.q_pos0 + row_i[t];      // token position of the query
      int b0 = t_new;                            // cached rows [0, t_new): the first whose key lies within the window
      while (lo < b0) {
        const int mid = (lo + b0) >> 1;
        const int tp = win.tok_pos[head_row + a.slot_of_pos[head_row + mid]];
        if (ekv_win_masked(pq, tp, win_w)) lo = mid + 1;
        else b0 = mid;
      }
      lo = max(lo, t_new + row_i[t] - win_w + 1);      // the chunk's own keys: position t_new + i' is token q_pos0 + i'
    }
    win_lo[t] = lo;
    win_lo_wave = max(win_lo_wave, lo);
  }
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) win_lo_wave = max(win_lo_wave, __shfl_xor(win_lo_wave, off, 64));
  win_lo_wave = __builtin_amdgcn_readfirstlane(win_lo_wave);
#endif

  // append: the (split, query block) that owns the new positions [t_new+i0, t_new+i0+nb) within its key range copies their
  // K/V rows into the cache slots.  Done here, not inside the tile loads: predicated stores in the load sequence made the
  // compiler wait on the loads in flight (and spill the store addresses).  Nobody reads these slots in this launch —
  // new rows are always taken from k_new / v_new.
  if (MODE != 1) {
    const int j_lo = max(t_new + i0, t0), j_hi = min(t_new + i0 + nb, t1);
    for (int piece = tid; piece < (j_hi - j_lo) * PPR; piece += NT) {
      const int j = j_lo + piece / PPR, sub = piece % PPR;
      const size_t off = (head_row + s_slot[j - t0]) * D;
      const size_t noff = (size_t)ll * a.n_kv_heads * n * D + (size_t)h * a.kv_hs + (size_t)(j - t_new) * a.kv_ts;
      reinterpret_cast<uint4*>(a.k_w + off)[sub] = reinterpret_cast<const uint4*>(a.k_new + noff)[sub];
      reinterpret_cast<uint4*>(a.v_w + off)[sub] = reinterpret_cast<const uint4*>(a.v_new + noff)[sub];
      EKV_WIN_ONLY(if (sub == 0) win.tok_pos[head_row + s_slot[j - t0]] = win.q_pos0 + (j - t_new);)      // (the row's token position, with the row)
    }
  }

  // 1-tile variant: Q operands of this lane's query row, loaded once (loop invariant)
  ekv_h8 qreg[QPW][KB], qreg_lo[QPW][KB];
  if (!Q_LDS) {
#pragma unroll
    for (int t = 0; t < QPW; ++t) {
      const size_t qoff = (((size_t)ll * a.n_q_heads + h * rep + row_r[t]) * n + row_i[t]) * D;
      const size_t qsrc = (size_t)ll * a.n_q_heads * n * D + (size_t)(h * rep + row_r[t]) * a.q_hs + (size_t)row_i[t] * a.q_ts;
#pragma unroll
      for (int kb = 0; kb < KB; ++kb) {
        qreg[t][kb] = __builtin_bit_cast(ekv_h8, reinterpret_cast<const uint4*>((ROPE ? a.q_rot_hi + qoff : a.q + qsrc) + kb * 32)[g]);
        qreg_lo[t][kb] = ekv_h8{0, 0, 0, 0, 0, 0, 0, 0};
        if (ROPE) qreg_lo[t][kb] = __builtin_bit_cast(ekv_h8, reinterpret_cast<const uint4*>(a.q_rot_lo + qoff + kb * 32)[g]);
        if (!row_ok[t]) qreg[t][kb] = qreg_lo[t][kb] = ekv_h8{0, 0, 0, 0, 0, 0, 0, 0};
      }
    }
  }

  // staging -------------------------------------------------------------------------------------------
  // register staging: the loads of tile t+1 are issued right after tile t has been written to LDS and stay in
  // flight while tile t is consumed
  // Addresses: one wave-uniform base per tensor and source (cache rows of this head / the launch's new rows of this head) and a
  // 32-bit byte offset per lane.  (64-bit per-lane arithmetic from the global bases was ~100 of the ~290 VALU instructions of a tile.)
  const char* const k_old = reinterpret_cast<const char*>(a.k + head_row * D);
  const char* const v_old = reinterpret_cast<const char*>(a.v + head_row * D);
  const char* const k_nw = reinterpret_cast<const char*>(a.k_new + (size_t)ll * a.n_kv_heads * n * D + (size_t)h * a.kv_hs);
  const char* const v_nw = reinterpret_cast<const char*>(a.v_new + (size_t)ll * a.n_kv_heads * n * D + (size_t)h * a.kv_hs);
  const uint32_t kvrs = (uint32_t)a.kv_ts * 2u;      // bytes between two of this launch's new rows (ekv_step.kv_token_stride; dense: 2 * D)
  uint4 stK[PF][LPT], stV[PF][LPT];
  // Three workgroup-uniform cases, the same number of loads in each (hipcc's s_waitcnt bookkeeping stays exact across the join):
  // a tile of cache rows only (slot map -> row, scalar base + 32-bit lane offset), a tile of this launch's new rows only (the
  // dense prefix: contiguous, the lane offset is loop-invariant), and the one tile that straddles t_new or the end of the range.
  auto stage_load = [&](const int buf, int kt) {
    // the three cases only compute ADDRESSES; the loads themselves sit behind the join, once (loads inside the branches come back
    // as one register copy per loaded dword at every join)
    const char* kp[LPT];
    ptrdiff_t v_minus_k[LPT];
    if (kt + kKT <= min(t_new, t1)) {
#pragma unroll
      for (int p = 0; p < LPT; ++p) {
        const bool live = tid + p * NT < kKT * PPT;
        const int piece = live ? tid + p * NT : tid % PPT;
        kp[p] = k_old + ((uint32_t)s_slot[kt - t0 + piece / PPT] * (uint32_t)(D * 2) + (uint32_t)min(piece % PPT, PPR - 1) * 16u);
        v_minus_k[p] = v_old - k_old;
      }
    } else if (kt >= t_new && kt + kKT <= t1) {
      const char* const kb = k_nw + (size_t)(kt - t_new) * kvrs;
#pragma unroll
      for (int p = 0; p < LPT; ++p) {
        const bool live = tid + p * NT < kKT * PPT;
        const int piece = live ? tid + p * NT : tid % PPT;
        kp[p] = kb + ((uint32_t)(piece / PPT) * kvrs + (uint32_t)min(piece % PPT, PPR - 1) * 16u);
        v_minus_k[p] = v_nw - k_nw;
      }
    } else {
#pragma unroll
      for (int p = 0; p < LPT; ++p) {
        const bool live = tid + p * NT < kKT * PPT;
        const int piece = live ? tid + p * NT : tid % PPT;
        const int row = piece / PPT, sub = min(piece % PPT, PPR - 1);
        const int j = min(kt + row, t1 - 1);
        const int sl = s_slot[j - t0];
        const bool is_new = j >= t_new;
        // (`is_new ? a.k_new + noff : a.k + off` once made hipcc pick the pointer FIELD per lane and fetch it from the
        // kernel-argument block with a vector load + s_waitcnt vmcnt(0) in front of every tile load, which drained the
        // prefetched tile before the next one was even issued: the bases are plain locals here)
        kp[p] = (is_new ? k_nw : k_old) + ((is_new ? (uint32_t)(j - t_new) * kvrs : (uint32_t)sl * (uint32_t)(D * 2)) + (uint32_t)sub * 16u);
        v_minus_k[p] = is_new ? v_nw - k_nw : v_old - k_old;
      }
    }
#pragma unroll
    for (int p = 0; p < LPT; ++p) {
      stK[buf][p] = __builtin_bit_cast(uint4, __builtin_nontemporal_load(reinterpret_cast<const ekv_u4*>(kp[p])));
      if (MODE != 1) stV[buf][p] = __builtin_bit_cast(uint4, __builtin_nontemporal_load(reinterpret_cast<const ekv_u4*>(kp[p] + v_minus_k[p])));
    }
  };
  auto stage_store = [&](const int buf, int kt) {
#pragma unroll
    for (int p = 0; p < LPT; ++p) {
      const bool in_tile = tid + p * NT < kKT * PPT;          // D = 32 with 8 waves: only half the threads hold a piece
      const int piece = in_tile ? tid + p * NT : tid % PPT;   // (idle lanes keep a consistent sub for the shuffles below)
      const int row = piece / PPT, sub = piece % PPT;
      const bool live = in_tile && sub < PPR;                 // (head_dim 96: slots 12..15 of a row hold a copy of piece 11, never stored)
      uint4 kv = stK[buf][p];
      if (ROPE) {
        // keys are cached un-rotated; rotate by the position index at read time (llama_patch.py:312, :327):
        // k' = k*cos[j] + rotate_half(k)*sin[j]; the partner d +- D/2 sits in lane (sub ^ PPR/2)
        const int j = min(kt + row, t1 - 1);
        const ekv_h8 x = __builtin_bit_cast(ekv_h8, kv);
        ekv_h8 y, yl;
        uint4 other;
        if (PPT != PPR) {      // partner piece PPR / 2 slots away inside the row's 16 slots (one wave): ds_bpermute
          const int src = (lane & ~(PPT - 1)) | (sub < PPR / 2 ? sub + PPR / 2 : (sub < PPR ? sub - PPR / 2 : sub));
          other.x = __shfl(kv.x, src, 64);
          other.y = __shfl(kv.y, src, 64);
          other.z = __shfl(kv.z, src, 64);
          other.w = __shfl(kv.w, src, 64);
        } else {
          other.x = __shfl_xor(kv.x, PPR / 2, 64);
          other.y = __shfl_xor(kv.y, PPR / 2, 64);
          other.z = __shfl_xor(kv.z, PPR / 2, 64);
          other.w = __shfl_xor(kv.w, PPR / 2, 64);
        }
        const ekv_h8 o8 = __builtin_bit_cast(ekv_h8, other);
        const float* cs = a.rope_cos + (size_t)j * D + (min(sub, PPR - 1) % (PPR / 2)) * 8;   // cat(freqs, freqs): read the first half only
        const float* sn = a.rope_sin + (size_t)j * D + (min(sub, PPR - 1) % (PPR / 2)) * 8;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float rh = (sub < PPR / 2) ? -(float)o8[e] : (float)o8[e];
          const float kr = (float)x[e] * cs[e] + rh * sn[e];
          y[e] = (ekv_e)kr;
          yl[e] = (ekv_e)(kr - (float)y[e]);
        }
        kv = __builtin_bit_cast(uint4, y);
        if (live) *reinterpret_cast<uint4*>(sKl + row * RS + sub * 8) = __builtin_bit_cast(uint4, yl);
      }
      if (!live) continue;
      *reinterpret_cast<uint4*>(sK + row * RS + sub * 8) = kv;
      if (MODE != 1) *reinterpret_cast<uint4*>(sV + row * RS + sub * 8) = stV[buf][p];
    }
  };

  // consume(kt): everything between the two barriers of one super-tile
  auto consume = [&](int kt) {
    const int kg = wk * 32;   // this wave's 32 keys of the super-tile
    if (kt + kg < t1) {
      float cs[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, cq[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};   // MODE 2
      // ---- S^T = K . Q^T: two 16-key tiles x the wave's query tiles; a K operand is read from LDS once per k-step and used for
      // all of them.  A wave whose last query tile lies past the block runs the variant without it (wave-uniform branch OUTSIDE
      // the k-loop: inside, every join copies the accumulators).
      // ROPE: q' = q*cos[pos] + rotate_half(q)*sin[pos], pos = T-n+i (llama_patch.py:311, :326) was rotated once by
      // ekv_rope_q_kernel and is read as an fp16 pair hi + lo
      ekv_f4 S[QPW][2];
#pragma unroll
      for (int t = 0; t < QPW; ++t) S[t][0] = S[t][1] = ekv_f4{0.f, 0.f, 0.f, 0.f};
      auto qk = [&](auto ntc) {
        constexpr int nt = decltype(ntc)::value;
#pragma unroll
        for (int kb = 0; kb < KB; ++kb) {
          const ekv_h8 a0 = *reinterpret_cast<const ekv_h8*>(sK + (kg + c) * RS + kb * 32 + g * 8);
          const ekv_h8 a1 = *reinterpret_cast<const ekv_h8*>(sK + (kg + 16 + c) * RS + kb * 32 + g * 8);
          ekv_h8 l0 = {0, 0, 0, 0, 0, 0, 0, 0}, l1 = {0, 0, 0, 0, 0, 0, 0, 0};
          if (ROPE) {
            l0 = *reinterpret_cast<const ekv_h8*>(sKl + (kg + c) * RS + kb * 32 + g * 8);
            l1 = *reinterpret_cast<const ekv_h8*>(sKl + (kg + 16 + c) * RS + kb * 32 + g * 8);
          }
#pragma unroll
          for (int t = 0; t < nt; ++t) {
            const int qt = wq + NWQ * t;
            ekv_h8 bq, bql = {0, 0, 0, 0, 0, 0, 0, 0};
            if (Q_LDS) {   // rows past the block are zero in LDS
              bq = *reinterpret_cast<const ekv_h8*>(sQh + (qt * 16 + c) * RS + kb * 32 + g * 8);
              if (ROPE) bql = *reinterpret_cast<const ekv_h8*>(sQl + (qt * 16 + c) * RS + kb * 32 + g * 8);
            } else {
              bq = qreg[t][kb];
              if (ROPE) bql = qreg_lo[t][kb];
            }
            S[t][0] = EKV_MFMA_16x16x32(a0, bq, S[t][0], 0, 0, 0);
            S[t][1] = EKV_MFMA_16x16x32(a1, bq, S[t][1], 0, 0, 0);
            if (ROPE) {   // (kh + kl).(qh + ql) ~= kh.qh + kh.ql + kl.qh
              S[t][0] = EKV_MFMA_16x16x32(a0, bql, S[t][0], 0, 0, 0);
              S[t][1] = EKV_MFMA_16x16x32(a1, bql, S[t][1], 0, 0, 0);
              S[t][0] = EKV_MFMA_16x16x32(l0, bq, S[t][0], 0, 0, 0);
              S[t][1] = EKV_MFMA_16x16x32(l1, bq, S[t][1], 0, 0, 0);
            }
          }
        }
      };
      if (QPW == 1 || (wq + NWQ * (QPW - 1)) * 16 < NR) qk(std::integral_constant<int, QPW>{});
      else qk(std::integral_constant<int, (QPW > 1 ? QPW - 1 : 1)>{});
      ekv_h8 bPs[QPW], bPls[QPW];   // P^T operands (fp16 pair hi + lo) of every query tile of the wave
      float alphas[QPW];
      bool rescale_any = false;
#pragma unroll
      for (int t = 0; t < QPW; ++t) {
        const int qt = wq + NWQ * t;
        bPs[t] = bPls[t] = ekv_h8{0, 0, 0, 0, 0, 0, 0, 0};
        alphas[t] = 1.f;
        if (qt * 16 >= NR) continue;   // wave-uniform
        const ekv_f4 s0 = S[t][0], s1 = S[t][1];
        // ---- scale, causal mask, export -------------------------------------------------------------
        // (this kernel is VALU-bound at wide strides and on the dense prefix: 16 VALU instructions per MFMA, rocprofv3
        // SQ_INSTS_VALU / SQ_INSTS_MFMA and the static count of the tile loop; a wave64 VALU instruction occupies the SIMD for
        // 4 cycles, an MFMA 16x16x32 for 16 — everything per logit below is counted in single instructions)
        float sv[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) sv[e] = e < 4 ? s0[e] : s1[e - 4];
        if (need_div) {   // kernel-uniform: the logits / row statistics leave the kernel, so they are the reference's quotients
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            // s / sqrt(D) as the reference divides (llama_patch.py:198): reciprocal multiply + one residual correction = the
            // correctly rounded quotient for every normal operand, 3 instructions instead of the 11 of v_div_scale/fmas/fixup
            const float q0 = sv[e] * inv_sm_div;
            sv[e] = fmaf(fmaf(-a.sm_div, q0, sv[e]), inv_sm_div, q0);
#if EKV_SOFTCAP
            sv[e] = ekv_softcap(sv[e], a.softcap);
#endif
          }
        }
        // masking is needed only where the 32 keys of this wave reach the chunk's own positions or the end of the range: a
        // wave-uniform test keeps the 8 compare / select pairs out of all other tiles
        if (kt + kg + 32 > min(t1, t_new + i0 + 1)) {
          const int jlim = min(t1, t_new + row_i[t] + 1);   // first masked position for this query
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const int j = kt + kg + (e < 4 ? 4 * g + e : 16 + 4 * g + (e - 4));
            if (j >= jlim) sv[e] = EKV_NEG_INF;
          }
        }
#if EKV_WINDOW
        if (kt + kg < win_lo_wave) {      // wave-uniform: tiles past every bound of the wave skip the compares
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const int j = kt + kg + (e < 4 ? 4 * g + e : 16 + 4 * g + (e - 4));
            if (j < win_lo[t]) sv[e] = EKV_NEG_INF;
          }
        }
#endif
        // (fmaxf() canonicalises both operands first under IEEE mode, v_max_f32 x, x: 3 instructions per maximum)
        float mx = ekv_max3(ekv_max3(ekv_max3(sv[0], sv[1], sv[2]), sv[3], sv[4]), ekv_max3(sv[5], sv[6], sv[7]), EKV_NEG_INF);
        if (MODE == 0 && a.logits != nullptr && row_ok[t]) {
          // the S^T layout gives each lane 4 consecutive keys per tile: two 16-byte stores (rows are 256-B aligned and
          // t_pad covers whole 64-position tiles; positions >= T just receive -inf)
          float* lrow = a.logits + (((size_t)ll * a.n_q_heads + h * rep + row_r[t]) * n + row_i[t]) * a.t_pad + kt + kg + 4 * g;
          *reinterpret_cast<float4*>(lrow) = make_float4(sv[0], sv[1], sv[2], sv[3]);
          *reinterpret_cast<float4*>(lrow + 16) = make_float4(sv[4], sv[5], sv[6], sv[7]);
        }
        ekv_h8 bP = {0, 0, 0, 0, 0, 0, 0, 0}, bPl = {0, 0, 0, 0, 0, 0, 0, 0};   // p = hi + lo (fp16 pair)
        float alpha = 1.f;
        if (MODE == 2) {
          // ---- exact probabilities from the final statistics; column sums of the GQA-folded p ----------
          // p = 2^(s*log2e - M*log2e) / L: one fma, one v_exp_f32 and one multiply per logit (M*log2e and 1/L per row, hoisted)
          const float nm = -m_run[t] * EKV_LOG2E;
          const ekv_f2 c2 = {EKV_LOG2E, EKV_LOG2E}, nm2 = {nm, nm}, il2 = {inv_l[t], inv_l[t]};
          ekv_f2 lsv = {0.f, 0.f};
#pragma unroll
          for (int e = 0; e < 8; e += 2) {
            const ekv_f2 arg = __builtin_elementwise_fma(ekv_f2{sv[e], sv[e + 1]}, c2, nm2);
            const ekv_f2 p2 = ekv_f2{__builtin_amdgcn_exp2f(arg[0]), __builtin_amdgcn_exp2f(arg[1])} * il2;
            lsv += p2;
            bP[e] = (ekv_e)p2[0];
            bP[e + 1] = (ekv_e)p2[1];
            if (EKV_CHUNK_PSPLIT) {
              bPl[e] = (ekv_e)(p2[0] - (float)bP[e]);
              bPl[e + 1] = (ekv_e)(p2[1] - (float)bP[e + 1]);
            }
            // sum over the rep query heads of the query: they sit in adjacent lanes (c = i*rep + r)
            ekv_f2 vb = p2;
            if (rep >= 2) vb += ekv_f2{ekv_dpp<0xB1>(vb[0]), ekv_dpp<0xB1>(vb[1])};
            if (rep >= 4) vb += ekv_f2{ekv_dpp<0x4E>(vb[0]), ekv_dpp<0x4E>(vb[1])};
            if (rep >= 8) vb += ekv_f2{ekv_dpp<0x141>(vb[0]), ekv_dpp<0x141>(vb[1])};
            if (rep >= 16) vb += ekv_f2{ekv_dpp<0x140>(vb[0]), ekv_dpp<0x140>(vb[1])};
            const ekv_f2 vq = vb * vb;      // (p^2 is rounded before it is summed, as the reference's (p ** 2).sum)
            cs[e] += vb[0];
            cs[e + 1] += vb[1];
            cq[e] += vq[0];
            cq[e + 1] += vq[1];
          }
          l_run[t] += lsv[0] + lsv[1];
        } else {
          // ---- online softmax; the 4 lane groups of a query share the running max -------------------
          // p = 2^(s*c - m*c): ONE fma and one v_exp_f32 per logit (c = log2 e, or log2 e / sqrt(D) straight on the MFMA
          // accumulators when nothing but the output leaves the kernel).  The floor keeps a row whose keys so far are all
          // masked out of the -inf - -inf corner without a branch: 2^(-inf + huge) = 0 either way.
          mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
          mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
          const float mn = fmaxf(fmaxf(m_run[t], mx), kMFloor);
          alpha = __builtin_amdgcn_exp2f((m_run[t] - mn) * cexp);
          const float nm = -mn * cexp;
          const ekv_f2 c2 = {cexp, cexp}, nm2 = {nm, nm};
          ekv_f2 lsv = {0.f, 0.f};
#pragma unroll
          for (int e = 0; e < 8; e += 2) {
            const ekv_f2 arg = __builtin_elementwise_fma(ekv_f2{sv[e], sv[e + 1]}, c2, nm2);
            const ekv_f2 p2 = {__builtin_amdgcn_exp2f(arg[0]), __builtin_amdgcn_exp2f(arg[1])};
            lsv += p2;
            bP[e] = (ekv_e)p2[0];
            bP[e + 1] = (ekv_e)p2[1];
            if (EKV_CHUNK_PSPLIT) {
              bPl[e] = (ekv_e)(p2[0] - (float)bP[e]);
              bPl[e + 1] = (ekv_e)(p2[1] - (float)bP[e + 1]);
            }
          }
          l_run[t] = l_run[t] * alpha + (lsv[0] + lsv[1]);
          m_run[t] = mn;
        }
        bPs[t] = bP;
        bPls[t] = bPl;
        alphas[t] = alpha;
        rescale_any = rescale_any || __builtin_amdgcn_ballot_w64(alpha != 1.f) != 0ull;
      }
      // ---- O^T = O^T*alpha + V^T . P^T: the V^T operand of a d-block is gathered ONCE for all query tiles ---------
      if (MODE != 1) {
        // the running maximum of a row settles after a few tiles: the rescale of the accumulator blocks is skipped (wave-uniform
        // branch) whenever no lane of the wave moved its maximum.  The empty asm keeps hipcc from turning the branch back into
        // "multiply always, then select" (4 v_cndmask per accumulator block: 96 of the 356 VALU instructions of a tile).
        if (MODE == 0 && rescale_any) {
          asm volatile("" ::: "memory");
#pragma unroll
          for (int t = 0; t < QPW; ++t)
#pragma unroll
            for (int db = 0; db < DB; ++db) oacc[t][db] = oacc[t][db] * alphas[t];
        }
#pragma unroll
        for (int db = 0; db < DB; ++db) {
          // slots e<4 -> key 4g+e, e>=4 -> key 16+4g+(e-4): matches the S^T accumulator layout, no shuffle
          // two transposing LDS reads (ds_read_b64_tr_b16: the 16 lanes of group g fetch the 4-key x 16-column block of rows
          // 4g .. 4g+3 row-wise, 8 bytes each, and lane c receives column c) instead of eight ds_read_u16 gathers
          typedef short ekv_s4 __attribute__((ext_vector_type(4)));
          typedef ekv_e ekv_h4 __attribute__((ext_vector_type(4)));
          const ekv_e* vp = sV + (kg + 4 * g + (c >> 2)) * RS + db * 16 + 4 * (c & 3);
          const ekv_h4 v_lo = __builtin_bit_cast(ekv_h4, __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) ekv_s4*)vp));
          const ekv_h4 v_hi = __builtin_bit_cast(ekv_h4, __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) ekv_s4*)(vp + 16 * RS)));
          const ekv_h8 aV = {v_lo[0], v_lo[1], v_lo[2], v_lo[3], v_hi[0], v_hi[1], v_hi[2], v_hi[3]};
#pragma unroll
          for (int t = 0; t < QPW; ++t) {
            if ((wq + NWQ * t) * 16 >= NR) continue;   // wave-uniform
            oacc[t][db] = EKV_MFMA_16x16x32(aV, bPs[t], oacc[t][db], 0, 0, 0);
            if (EKV_CHUNK_PSPLIT) oacc[t][db] = EKV_MFMA_16x16x32(aV, bPls[t], oacc[t][db], 0, 0, 0);
          }
        }
      }
      if (MODE == 2) {
        // column sums of this wave's query tiles for its 32 keys: reduce over the 16 query lanes, lane c == 0 stores.
        // cs holds rep * pbar per (query, head) lane -> sum_i pbar = total / rep^2, sum_i pbar^2 = total / rep^3
        const float k1 = 1.f / (float)(rep * rep), k2 = k1 / (float)rep;
        ekv_row_sum16(cs, cq);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          cs[e] *= k1;
          cq[e] *= k2;
        }
        if (c == 0) {
          float* dst = a.colsum + ((((size_t)ll * a.n_kv_heads + h) * a.n_col_parts + qb * NWQ + wq) * 2) * a.t_pad + kt + kg + 4 * g;
          *reinterpret_cast<float4*>(dst) = make_float4(cs[0], cs[1], cs[2], cs[3]);
          *reinterpret_cast<float4*>(dst + 16) = make_float4(cs[4], cs[5], cs[6], cs[7]);
          *reinterpret_cast<float4*>(dst + a.t_pad) = make_float4(cq[0], cq[1], cq[2], cq[3]);
          *reinterpret_cast<float4*>(dst + a.t_pad + 16) = make_float4(cq[4], cq[5], cq[6], cq[7]);
        }
      }
    }
  };

  if (t0 < t1) stage_load(0, t0);
  if (PF == 2 && t0 + kKT < t1) stage_load(1, t0 + kKT);
  for (int kt0 = t0; kt0 < t1; kt0 += PF * kKT) {
#pragma unroll
    for (int buf = 0; buf < PF; ++buf) {
      const int kt = kt0 + buf * kKT;
      if (kt >= t1) break;      // workgroup-uniform
      ekv_lds_barrier();        // previous tile fully consumed
      stage_store(buf, kt);
      ekv_lds_barrier();
      if (kt + PF * kKT < t1) stage_load(buf, kt + PF * kKT);   // in flight while this and the next tile are consumed
      consume(kt);
    }
  }

  if (MODE != 2) {   // running maxima back to the units every consumer below expects: quotient logits, -inf = "no key seen"
#pragma unroll
    for (int t = 0; t < QPW; ++t) {
      const float q0 = m_run[t] * inv_sm_div;
      const float mq = fmaf(fmaf(-a.sm_div, q0, m_run[t]), inv_sm_div, q0);   // correctly rounded m / sqrt(D), as in the tile loop
      m_run[t] = m_run[t] <= kMFloor ? EKV_NEG_INF : (need_div ? m_run[t] : mq);
    }
  }

  // ---- logits beyond this block's causal bound ---------------------------------------------------------
  // The scorer reads every row over all T positions.  A query block that ends before the chunk does stops at its own
  // causal bound t1, so the positions after its last 32-key half tile (and whole key splits beyond t1) get their -inf here.
  if (MODE == 0 && a.logits != nullptr) {
    const int t_end = min(T, t0 + a.rows_per_split);
    const int fill_lo = t0 < t1 ? t0 + (t1 - t0 + 31) / 32 * 32 : t0;   // consume() works in 32-key halves
    const int w = t_end - fill_lo;
    if (w > 0) {
      for (int idx = tid; idx < NR * w; idx += NT) {
        const int row = idx / w, j = fill_lo + idx % w;
        a.logits[(((size_t)ll * a.n_q_heads + h * rep + row % rep) * n + i0 + row / rep) * a.t_pad + j] = EKV_NEG_INF;
      }
    }
  }

  if (MODE == 2) {   // same for the column sums: both parts (wq = 0, 1) of this query block are zero past its bound
    const int t_end = min(T, t0 + a.rows_per_split);
    const int fill_lo = t0 < t1 ? t0 + (t1 - t0 + 31) / 32 * 32 : t0;
    const int w = t_end - fill_lo;
    float* dst = a.colsum + ((((size_t)ll * a.n_kv_heads + h) * a.n_col_parts + qb * NWQ) * 2) * a.t_pad + fill_lo;
    for (int idx = tid; idx < 2 * NWQ * w; idx += NT) dst[(size_t)(idx / w) * a.t_pad + idx % w] = 0.f;
  }

  // ---- unsplit heads whose scorer does not need the partial statistics: fold the two key halves right here ----------
  // (the dense prefix spent 40 % of its time in a separate fold kernel reading 0.5 GB of partials back)
  if (MODE != 1 && a.out_direct != nullptr) {
    constexpr int XS = DB * 4 + 2;                       // floats per lane: (m, l, o[DB][4])
    float* xch = reinterpret_cast<float*>(sK);           // the K/V tile buffers are free now: NWQ x 64 x XS floats fit exactly
#pragma unroll
    for (int t = 0; t < QPW; ++t) {
      float l = l_run[t];
      l += __shfl_xor(l, 16, 64);
      l += __shfl_xor(l, 32, 64);
      const float mt = MODE == 2 ? 0.f : m_run[t];
      ekv_lds_barrier();                                 // tiles (t = 0) / the previous exchange (t > 0) fully consumed
      float* mine = xch + (size_t)(wq * 64 + lane) * XS;
      if (wk == 1) {
        mine[0] = mt;
        mine[1] = l;
#pragma unroll
        for (int db = 0; db < DB; ++db)
#pragma unroll
          for (int e = 0; e < 4; ++e) mine[2 + db * 4 + e] = oacc[t][db][e];
      }
      ekv_lds_barrier();
      if (wk == 0 && row_ok[t]) {
        const float m1 = mine[0], l1 = mine[1];
        const float mm = fmaxf(mt, m1);
        const float w0 = mt == EKV_NEG_INF ? 0.f : exp2f((mt - mm) * EKV_LOG2E);
        const float w1 = m1 == EKV_NEG_INF ? 0.f : exp2f((m1 - mm) * EKV_LOG2E);
        const float lsum = l * w0 + l1 * w1;
        const float inv = 1.f / lsum;
        if (MODE == 0 && a.row_stats != nullptr && g == 0) {   // final softmax statistics of the row, for the scorer
          float* rs = a.row_stats + (((size_t)ll * a.n_q_heads + h * rep + row_r[t]) * n + row_i[t]) * 2;
          rs[0] = mm;
          rs[1] = lsum;
        }
        __half* orow = a.out_direct + (size_t)ll * a.n_q_heads * n * D + (size_t)(h * rep + row_r[t]) * a.o_hs + (size_t)row_i[t] * a.o_ts;
#pragma unroll
        for (int db = 0; db < DB; ++db) {
          __half2 lo = ekv_to_e2((oacc[t][db][0] * w0 + mine[2 + db * 4 + 0] * w1) * inv,
                                 (oacc[t][db][1] * w0 + mine[2 + db * 4 + 1] * w1) * inv);
          __half2 hi = ekv_to_e2((oacc[t][db][2] * w0 + mine[2 + db * 4 + 2] * w1) * inv,
                                 (oacc[t][db][3] * w0 + mine[2 + db * 4 + 3] * w1) * inv);
          uint2 pk;
          pk.x = __builtin_bit_cast(unsigned int, lo);
          pk.y = __builtin_bit_cast(unsigned int, hi);
          *reinterpret_cast<uint2*>(orow + db * 16 + 4 * g) = pk;
        }
      }
    }
#if EKV_CHUNK_MODE == 0
    if (FUSE) {
      // Scorer tail.  This workgroup wrote every logit, the row statistics and the new K/V rows of the head itself; the
      // barrier (workgroup-scope fence, stores drained) makes them visible to all of its waves.  The K/V tile buffers, the
      // slot indices and the query block in LDS are dead: the scorer's arrays take their place.
      __syncthreads();
      ekv_score_select_body(sc, h, ll, smem);
    }
#endif
    return;
  }

  // ---- partials: one per (split, wk) ------------------------------------------------------------------
#pragma unroll
  for (int t = 0; t < QPW; ++t) {
    float l = l_run[t];
    l += __shfl_xor(l, 16, 64);
    l += __shfl_xor(l, 32, 64);
    if (!row_ok[t]) continue;
    const size_t prow = (((size_t)ll * a.n_q_heads + h * rep + row_r[t]) * n + row_i[t]) * nse + split * 2 + wk;
    if (MODE == 1) {   // statistics pass: (max, sum exp) of this wave's keys, nothing else
      if (g == 0) {
        a.stats[prow * 2] = m_run[t];
        a.stats[prow * 2 + 1] = l;
      }
      continue;
    }
    float* dst = a.partials + prow * PS;
    if (g == 0) {
      dst[0] = MODE == 2 ? 0.f : m_run[t];   // MODE 2: p is already normalised, the partials simply add up
      dst[1] = l;
    }
#pragma unroll
    for (int db = 0; db < DB; ++db) {
      float* o = dst + 2 + db * 16 + 4 * g;
      o[0] = oacc[t][db][0];
      o[1] = oacc[t][db][1];
      o[2] = oacc[t][db][2];
      o[3] = oacc[t][db][3];
    }
  }
}

template <int QPW, bool ROPE, int NW>
hipError_t launch_k(const EkvAttnArgs& a, int layer_count, hipStream_t s, const EkvScoreArgs* fuse_sc EKV_SINK_ONLY(, const float* sinks) EKV_WIN_ONLY(, const EkvWinArgs& win)) {
  // slot entries | tiles | the query block; the 16-wave in-kernel fold exchanges NWQ x 64 x (D + 2) floats (ekv_geometry.h, where the planner reads it too)
  static_assert(kKT == kChunkKT && kPadH == kChunkPadH && EKV_Q_LDS(QPW, ROPE, NW) == ekv_chunk_q_in_lds(EKV_CHUNK_MODE, QPW, ROPE, NW),
                "the LDS plan of ekv_geometry.h is this kernel's");
  size_t lds = ekv_chunk_kernel_lds(EKV_D, EKV_CHUNK_MODE, QPW, ROPE, NW, a.rows_per_split, a.out_direct != nullptr);
  const dim3 grid(a.n_kv_heads, a.n_split * a.n_qblocks, layer_count);
#if EKV_CHUNK_MODE == 0
  if (fuse_sc != nullptr) {
    if (NW != 4 || a.n_split != 1 || a.n_qblocks != 1 || a.out_direct == nullptr) return hipErrorInvalidValue;
    lds = std::max(lds, ekv_score_lds_bytes(256, *fuse_sc));
    if (lds > 48 * 1024)
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&ekv_attn_chunk_kernel<QPW, ROPE, 4, true>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL((ekv_attn_chunk_kernel<QPW, ROPE, 4, true>), grid, dim3(256), lds, s, a, *fuse_sc EKV_SINK_ONLY(, sinks) EKV_WIN_ONLY(, win));
    return hipGetLastError();
  }
#endif
  if (lds > 48 * 1024)
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&ekv_attn_chunk_kernel<QPW, ROPE, NW>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL((ekv_attn_chunk_kernel<QPW, ROPE, NW>), grid, dim3(64 * NW), lds, s, a, EkvScoreArgs{} EKV_SINK_ONLY(, sinks) EKV_WIN_ONLY(, win));
  return hipGetLastError();
}

}  // namespace

// rows per query block = rep * qb_rows <= 32 * qpw
#if EKV_SOFTCAP
// the capped instances: plain keys, the one-tile build alone, at either head_dim (the planner blocks their steps as head_dim 256's)
hipError_t EKV_FN_CHUNK_CAP(EKV_D, EKV_CHUNK_MODE, EKV_ELEM)(const EkvAttnArgs& a, int qpw, int layer_count, hipStream_t s,
                                                             const EkvScoreArgs* fuse_sc) {
  static_assert(EKV_D == 128 || EKV_D == kChunkNarrowD, "capped chunk instances: head_dim 128 and 256");
  if (a.rope_cos != nullptr || qpw != 1 || !(a.softcap > 0.f)) return hipErrorInvalidValue;
  return launch_k<1, false, 4>(a, layer_count, s, fuse_sc);
}
#elif EKV_WINDOW
// the window instances, alone (head_dim 128) and with sinks (head_dim 64): one signature, `sinks` NULL in the window-alone ones; plain
// keys, the one-tile build alone (the planner blocks their steps as the sink call's)
#if EKV_SINK
#define EKV_WCHUNK_SYM EKV_FN_CHUNK_SINK_WIN(EKV_D, EKV_CHUNK_MODE, EKV_ELEM)
#else
#define EKV_WCHUNK_SYM EKV_FN_CHUNK_WIN(EKV_D, EKV_CHUNK_MODE, EKV_ELEM)
#endif
hipError_t EKV_WCHUNK_SYM(const EkvAttnArgs& a, const float* sinks, const EkvWinArgs& win, int qpw, int layer_count, hipStream_t s,
                          const EkvScoreArgs* fuse_sc) {
  static_assert(EKV_D == 64 || EKV_D == 128, "window chunk instances: head_dim 64 and 128");
  if (a.rope_cos != nullptr || qpw != 1 || (sinks == nullptr) != !EKV_SINK || win.tok_pos == nullptr || win.windows == nullptr) return hipErrorInvalidValue;
  return launch_k<1, false, 4>(a, layer_count, s, fuse_sc EKV_SINK_ONLY(, sinks), win);
}
#elif EKV_SINK
// the sink instances: plain keys, the one-tile build alone (the planner blocks their steps as head_dim 256's), head_dim 64 and 128
hipError_t EKV_FN_CHUNK_SINK(EKV_D, EKV_CHUNK_MODE, EKV_ELEM)(const EkvAttnArgs& a, const float* sinks, int qpw, int layer_count, hipStream_t s,
                                                              const EkvScoreArgs* fuse_sc) {
  static_assert(EKV_D == 64 || EKV_D == 128, "sink chunk instances: head_dim 64 and 128");
  if (a.rope_cos != nullptr || qpw != 1 || sinks == nullptr) return hipErrorInvalidValue;
  return launch_k<1, false, 4>(a, layer_count, s, fuse_sc, sinks);
}
#else
hipError_t EKV_FN_CHUNK(EKV_D, EKV_CHUNK_MODE, EKV_ELEM)(const EkvAttnArgs& a, int qpw, int layer_count, hipStream_t s,
                                                                                    const EkvScoreArgs* fuse_sc) {
  const bool rope = a.rope_cos != nullptr;
  constexpr bool R = !EKV_BF16 && EKV_D < kChunkNarrowD;   // (RoPE-on-read builds: fp16 only, head_dim <= 128)
  if (rope && !R) return hipErrorInvalidValue;
#if EKV_D >= 256
  // head_dim 256: the one-tile build alone (ekv_chunk_blocks plans blocks of <= 32 rows).  Its 16 output blocks, 16 staged pieces and 8
  // query operands per lane are 254-255 VGPRs without scratch; the two-tile builds spill (448+ bytes of scratch per lane) and are not built.
  static_assert(EKV_D == kChunkNarrowD && EKV_D % 32 == 0, "head_dim 256 is the narrow-block head_dim of ekv_geometry.h");
  if (qpw != 1) return hipErrorInvalidValue;
  return launch_k<1, false, 4>(a, layer_count, s, fuse_sc);
#else
  switch (qpw) {
    case 1: return rope ? launch_k<1, R, 4>(a, layer_count, s, fuse_sc) : launch_k<1, false, 4>(a, layer_count, s, fuse_sc);
    case 2: return rope ? launch_k<2, R, 4>(a, layer_count, s, fuse_sc) : launch_k<2, false, 4>(a, layer_count, s, fuse_sc);
    case 4: if (fuse_sc != nullptr) return hipErrorInvalidValue;   // the fused scorer is the 256-thread build
      return rope ? launch_k<2, R, 8>(a, layer_count, s, nullptr) : launch_k<2, false, 8>(a, layer_count, s, nullptr);   // 8 waves x 2 tiles
#if EKV_CHUNK_MODE == 0
    case 8: if (fuse_sc != nullptr || rope) return hipErrorInvalidValue;   // 16 waves x 1 tile: four waves per SIMD (ekv_attn_chunk.hip)
      return launch_k<1, false, 16>(a, layer_count, s, nullptr);
#endif
    default: return hipErrorInvalidValue;
  }
#endif
}
#endif
