// K2w: chunk / dense-prefix attention for WIDE query blocks (33..128 GQA-folded rows) on mfma_f32_32x32x16_f16.
// Compiled once per (EKV_D, EKV_WIDE_MODE) by the ekv_attn_wide_d*_m*.hip stubs.
//
// Same contract as ekv_attn_chunk.inc (easykv/llama_patch.py:198-222, mistral_patch.py:144-169 for q_len = stride and for the
// dense prefix q_len = r_idx; the K/V append of DynamicCache.update, llama_patch.py:193-196) for the launches whose query block
// is wide enough that the MFMA kernel itself — not HBM — bounds the step (rep * stride = 96: 96 flop per K/V byte, and the
// two-pass scheme adds a third product): dense prefix, BASELINE configs[3] / [4]-shaped chunk steps, stride 64.  The 16x16x32
// kernel of ekv_attn_chunk.inc spent 5.7 VALU instructions per MFMA and half of its wave cycles waiting (two barriers per
// 64-key tile, 16-row query tiles, a single LDS tile buffer); this one is built the way the attention kernels that reach
// ~1 PFLOP/s on this chip are (cdna_hip_programming.md, Appendix B "fused attention prefill"):
//
//   * 32-row query tiles per wave, 32x32x16 MFMA: half the LDS operand bytes per flop of 16x16x32 and the shape that reaches
//     the MFMA peak; a workgroup is NWQ query waves x NWK key waves, every wave owns 32 rows x 32 keys of a TK = 32 * NWK
//     key tile, so a K/V tile in LDS is shared by all query waves.
//   * K/V tiles double-buffered in LDS, ONE barrier per tile, register staging split into "issue early / write late" (T14):
//     the loads of tile t+2 are issued in the middle of tile t and written to LDS in the middle of tile t+1.  Slot-map entries
//     (position -> physical row) are prefetched one tile further ahead into registers; nothing but K, V and the slot entries
//     is loaded inside the loop, and those loads are unconditional (clamped), so hipcc's vmcnt bookkeeping stays exact.
//   * K rows padded by 16 B (conflict-free ds_read_b128 row gathers), V rows unpadded with an XOR swizzle of the 16-byte
//     chunk index by the row (conflict-free ds_read_b64_tr_b16 of 4 rows x 64 B).
//
// EKV_WIDE_MODE (one per translation unit):
//   0  one pass over K and V, online softmax, output (unscored steps: the dense prefix; and the FIRST launch of a scored step).
//      S^T = K.Q^T (keys in registers, query = lane): row statistics are lane-local + one half-wave exchange, and the P^T operand of
//      O^T += V^T.P^T comes straight from the S^T accumulators.  With a.stats != nullptr it also leaves every row's final
//      (max, sum of exponentials) in log2 units — the statistics the column-sum pass needs (round 4: rounds 2-3 ran a K-only
//      statistics pass first and an "exact" pass with O, P and the column sums in one kernel, which sat at 256 VGPRs with 26-30
//      spilled registers and had no room for a rotated second Q).
//   2  column-sum pass (K only; the SECOND launch of a scored step): S = Q.K^T (queries in registers, key = lane) so that the
//      per-key column sums sum_i pbar_ij, sum_i pbar_ij^2 of the GQA-folded probabilities (easykv/easykv.py:443-457, :173-186)
//      are LANE-LOCAL adds; p = 2^(s*c - lse2_i) is final (one fma + one v_exp_f32 per probability).  No V, no output
//      accumulators, no P tile: <= 128 VGPRs.  The query waves' column sums are combined through LDS in fixed order and the owner
//      lane of a key column accumulates them in global memory: ONE partial row per head whatever the number of query waves or
//      query blocks — the workgroup of a (head, key range) walks all query blocks of a scored dense prefix itself
//      (keep_attention) — where the 16x16 kernel left 4 rows per query block to the scorer.
//
// EKV_WIDE_ROPE = 1 (own translation units): RoPE-on-read, `streaming=True` (easykv/llama_patch.py:310-327, mistral_patch.py:225-241) —
// keys are cached UN-rotated and rotated by their CURRENT position index on every read.  The K tile lands raw by LDS-DMA and is
// rotated in LDS at the top of its iteration by the whole workgroup: a thread owns the (d, d + D/2) chunk pair of a row (the XOR
// swizzle maps the pair to physical chunks pc, pc ^ PPR/2 of the same row), k' = k*cos[j] + rotate_half(k)*sin[j] in fp32 exactly
// as the reference's separate torch ops, and k' is split into fp16 hi + lo planes — hi overwrites the raw tile IN PLACE (a thread
// reads and writes only its own two chunks), lo goes to a third buffer; every product is three MFMAs, kh.qh + kl.qh + kh.ql, on
// the queries ekv_rope_q_kernel rotated once per step (fp16-rounded rotated keys alone sit 5e-4 from the fp32 reference: the
// eviction ids would not survive).  The table values of the NEXT tile (fp32, L2-resident, 16 floats per chunk pair) are requested
// at the END of an iteration, after the PV registers have died and ahead of the wait for that tile's DMA — they are live across
// the barrier only, not across the MFMA / softmax phases (mode 0 has 239 of 256 registers in use with the second Q).  Rounds 1-3 ran
// this path on the 16x16 kernel in one pass with 2.6 GB of fp32 logits exported per configs[4] step and read back by the scorer.
#ifndef EKV_WIDE_ROPE
#define EKV_WIDE_ROPE 0
#endif
#include <algorithm>

#include "ekv_common.h"
#include "ekv_kernels.h"
#if EKV_BF16   // (bf16 instances, plain keys only: the same kernel under a tagged name)
static_assert(!EKV_WIDE_ROPE, "RoPE-on-read keeps hi / lo fp16 planes: no bf16 build");
#define ekv_attn_wide_kernel ekv_attn_wide_kernel_bf16
#endif

#define EKW_HAS_TAIL (EKV_WIDE_MODE == 2 && !EKV_WIDE_ROPE)      // (RoPE-on-read steps keep the stand-alone scorer: ekv_wide_tail.h)
#if EKW_HAS_TAIL
// the scorer as the tail of the column-sum pass (ekv_wide_tail.h) reuses the stand-alone scorer's exact selects
#define EKV_SS_NT 256
#define EKV_SS_DEVICE_ONLY
#include "ekv_score_select.inc"
#include "ekv_wide_tail.h"
#endif

namespace {

typedef float ekv_f16v __attribute__((ext_vector_type(16)));
typedef short ekv_s4 __attribute__((ext_vector_type(4)));
typedef float ekv_f4w __attribute__((ext_vector_type(4)));
typedef ekv_e ekv_h4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float ekw_max3(float x, float y, float z) {
  float r;
  asm("v_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(x), "v"(y), "v"(z));
  return r;
}

// x of this lane and of lane ^ 32 (v_permlane32_swap: lanes 32..63 of the first operand <-> lanes 0..31 of the second):
// first = the lower half's value, second = the upper half's, in every lane — so a sum is formed in the same order in both halves.
__device__ __forceinline__ void ekw_halves(float x, float& lo, float& hi) {
  const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
  lo = __uint_as_float(r[0]);
  hi = __uint_as_float(r[1]);
}

// 16 bytes per lane global -> LDS without passing through registers (global_load_lds_dwordx4): lds_dst is the wave-uniform base of a
// 1 KB piece, lane i lands at + 16 * i.  (A __device__ function on purpose: the builtin inside a LAMBDA of the kernel makes the
// host pass of hipcc drop the kernel's stub without a diagnostic — the library then fails to load with an undefined symbol.)
// stream = rows this workgroup is the only reader of in this launch (a chunk step: one query block per head): non-temporal (nt),
// MI355X_MICROARCH.md "nt-weights": issued -> landed -18 % on data one CU reads once; the dense prefix's rows are re-read by every
// query block from L2 and keep the default policy.
#ifndef EKW_NT
#define EKW_NT 1
#endif
// Two forms.  Through the builtin (default) hipcc models the DMA as a store to LDS that any later LDS read may alias: it puts an
// `s_waitcnt vmcnt(0)` in front of the first ds_read_b64_tr_b16 after the issue, i.e. in the middle of the tile.  The inline-asm form
// (EKW_ASM_DMA=1; cdna_hip_programming.md §5.7: M0 written in the statement that reads it) hides the DMA from hipcc, so the only
// wait is the explicit one in ekw_tile_barrier() — measured SLOWER (dense prefix 688 vs 707 TFLOP/s, configs[3] step 1052 vs 1008
// us, same box, interleaved): the DMA of an HBM-fed tile is not done at the end of the tile either way, and the asm form costs a
// readfirstlane, an M0 save / restore and a "memory" clobber per piece.
// experiment builds (tools/experiments/build_variant.sh): 1 = staging only (DMA + barriers, nothing consumed), 2 = compute only (no tile DMA);
// RoPE builds (mocks: wrong results, same structure): 4 = no table loads (constant cos / sin), 5 = rotation without its arithmetic (LDS
// reads / writes and the barrier stay), 6 = no rotation at all (raw tile as hi plane, no second barrier), 7 = one MFMA per product instead of three;
// 9 = the one pass without its partial stores (split heads); dense-prefix mocks of the one pass, 10 + a bit mask - 1 (10…16):
// bit 1 = no softmax arithmetic (S^T converted as it is), 2 = no PV (neither the transposing V reads nor their MFMAs), 4 = no QK^T (S^T = cheap
// lane values, no K fragment reads)
#ifndef EKW_EXP
#define EKW_EXP 0
#endif
#ifndef EKW_NODMA
#define EKW_NODMA 0      // (mocks) 1: no tile DMA; 2: one piece in LPT (same waits, 1/LPT of the bytes); 3: every tile re-reads the range's first (cache-hot) rows
#endif
#ifndef EKW_DM      // (or given directly; bit 8 = ONE K / V fragment read per key block, reused by all of its MFMAs: prices the LDS fragment traffic)
#define EKW_DM ((EKW_EXP >= 10 && EKW_EXP <= 16) ? EKW_EXP - 9 : 0)
#endif
#ifndef EKW_ROT_CLS
#define EKW_ROT_CLS 1      // (0: the rotation's mapping of rounds 3-5, for A/B runs)
#endif
#ifndef EKW_KPREFETCH
#define EKW_KPREFETCH 0
#endif
#ifndef EKW_ASM_DMA
#define EKW_ASM_DMA 0
#endif
__device__ __forceinline__ void ekw_dma16(const char* src, char* lds_dst, const bool stream) {
#if EKW_ASM_DMA
  const uint32_t ldsa = __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)lds_dst);
  unsigned keep;
  if (EKW_NT && stream)
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off nt\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(src), "s"(ldsa) : "memory");
  else
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(src), "s"(ldsa) : "memory");
#else
  if (EKW_NT && stream) __builtin_amdgcn_global_load_lds(src, (__attribute__((address_space(3))) void*)lds_dst, 16, 0, 2);
  else __builtin_amdgcn_global_load_lds(src, (__attribute__((address_space(3))) void*)lds_dst, 16, 0, 0);
#endif
}

// A wave-uniform pointer pinned to scalar registers and made opaque: the DMA then takes the form "SGPR base + 32-bit lane offset".
// Left transparent, hipcc reassociates `base + tile offset + lane offset` into a hoisted per-lane 64-bit pointer per piece and
// tensor (8 VGPRs in the column-sum pass — spilled at 128 — and a v_lshl_add_u64 per DMA).
__device__ __forceinline__ const char* ekw_uniform(const char* p) {
  uint32_t lo = (uint32_t)reinterpret_cast<uintptr_t>(p), hi = (uint32_t)(reinterpret_cast<uintptr_t>(p) >> 32);
  asm volatile("" : "+s"(lo), "+s"(hi));
  return reinterpret_cast<const char*>((static_cast<uintptr_t>(hi) << 32) | lo);
}

// every LDS-DMA and every other load of the wave has landed, then the workgroup barrier
__device__ __forceinline__ void ekw_tile_barrier() {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  ekv_lds_barrier();
}

// A/B knob: raise the wave's priority around its MFMA clusters (cdna_hip_programming.md T5)
#ifndef EKW_SETPRIO
#define EKW_SETPRIO 0
#endif
#if EKW_SETPRIO
#define EKW_PRIO(x) __builtin_amdgcn_s_setprio(x)
#else
#define EKW_PRIO(x) do { } while (0)
#endif

constexpr float kWFloor = -1.0e30f;

// NWQ query waves (32 rows each) x NWK key waves, every wave takes KPW blocks of 32 keys of a TK = 32 * NWK * KPW key tile.
//   <4, 1, 2>  65..128 rows: 4 waves, each 32 rows x all 64 keys of the tile (32 MFMAs per wave and barrier)
//   <2, 2, 1>  33..64 rows: 2 x 2 waves, each 32 rows x 32 keys
// Both are 256-thread workgroups with <= 80 KB of LDS: TWO workgroups per CU, which drift out of phase, so that one's MFMA
// phases overlap the other's softmax / staging phases (the lock-stepped waves of ONE workgroup never do that for each other).
// workgroups per CU of the column-sum pass: 4 (<= 128 VGPRs) — the pass has ONE 16 KB tile in flight per workgroup and is bound by
// the bytes in flight per CU (configs[3] shape: 372 us at 3 workgroups, 299 at 4) — except where that would spill: 3 for GQA x4 on
// four query waves and for the run-time GQA factors 8 / 16
#ifndef EKW_M2_ROPE_WGS
#define EKW_M2_ROPE_WGS 2
#endif
#define EKW_M2_WGS(NWQ, REP) ((REP) == 0 || ((REP) == 4 && (NWQ) == 4) ? 3 : 4)
// REP (MODE 2): the GQA factor as a compile-time constant (1 / 2 / 4; 0 = 8 or 16, read at run time) — with a run-time factor hipcc
// if-converts the five fold variants (all computed, results selected: +32 VGPRs, and the per-register causal limits are hoisted: +36)
template <int NWQ, int NWK, int KPW, int REP>
// (the column-sum pass stages K only and keeps no output accumulators: <= 128 VGPRs and ~37 KB of LDS, i.e. FOUR workgroups per
//  CU — it streams K once and is bound by the bytes in flight per CU: one 16 KB tile per workgroup)
__global__ void __launch_bounds__(64 * NWQ * NWK, EKV_WIDE_MODE == 2 ? (EKV_WIDE_ROPE ? EKW_M2_ROPE_WGS : EKW_M2_WGS(NWQ, REP)) : 2) ekv_attn_wide_kernel(const EkvAttnArgs a, const EkvScoreArgs sc) {
  constexpr int D = EKV_D, MODE = EKV_WIDE_MODE;
  constexpr int NW = NWQ * NWK, NT = 64 * NW, TK = 32 * NWK * KPW, NKB = NWK * KPW;
  constexpr int PPR = D / 8, KS = D / 16, DB = D / 32, PS = D + 2;
  constexpr int RSK = 2 * D, RSV = 2 * D;                  // LDS row strides in BYTES: unpadded, XOR-swizzled 16-byte chunks
  constexpr int LPT = TK * PPR / NT;                       // LDS-DMA instructions (1 KB each) per wave, tile and tensor
  constexpr int RPI = 64 / PPR;                            // rows one LDS-DMA instruction covers
  static_assert((TK * PPR) % NT == 0 && LPT >= 1, "tile does not divide over the workgroup");
  static_assert(D == 64 || D == 128, "head_dim 64 / 128");
  constexpr int KBUF = TK * RSK, VBUF = TK * RSV;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  static_assert(MODE == 0 || MODE == 2, "modes: 0 (one pass, output [+ row statistics]) and 2 (column sums)");
  char* const sK = smem;                                   // [2][TK][RSK]
  char* const sV = sK + 2 * KBUF;                          // [2][TK][RSV]               (MODE 2: absent)
  constexpr bool ROPE = EKV_WIDE_ROPE != 0;
  char* const sKlo = sV + (MODE == 0 ? 2 * VBUF : 0);      // ROPE: [TK][RSK] lo plane of the rotated tile being consumed
  float* const sX = reinterpret_cast<float*>(sKlo + (ROPE ? KBUF : 0));           // MODE 2: column-sum exchange [2][NKB][NWQ][64]
  float* const sLse = sX + (MODE == 2 ? 2 * NKB * NWQ * 64 : 0);                  // MODE 2: [NWQ * 32] -log2 sum exp of the block's rows

  const int n = a.q_len, T = a.n_slots;
  const int rep = (MODE == 2 && REP > 0) ? REP : a.n_q_heads / a.n_kv_heads;
  // REP == -1 (RoPE builds of the one pass only): the instance that exports the raw logits and the row statistics of a one-pass scored
  // step — its own instance because the RoPE one pass sits at the 256-register ceiling: compiled into the common instance, the export's
  // bookkeeping spilled an LDS address of the QK loop of EVERY RoPE step
  constexpr bool LOGITS = EKV_WIDE_ROPE && MODE == 0 && REP == -1;
  const int h = blockIdx.x, ll = blockIdx.z;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wq = wave % NWQ, wk = wave / NWQ;
  const int hi = lane >> 5, c31 = lane & 31, G = lane >> 4, c = lane & 15;
  // MODE 2: a workgroup walks the query blocks qg, qg + QG, ... of its (head, key range) and owns partial column-sum row qg
  // (QG = a.n_col_parts: 1 when the launch has enough (head, layer) pairs to fill the chip, more for one-layer launches)
  const int QG = MODE == 2 ? a.n_col_parts : 1;
  const int qg = MODE == 2 ? (int)blockIdx.y % QG : 0;
  const int split = MODE == 2 ? (int)blockIdx.y / QG : (int)blockIdx.y / a.n_qblocks;
  const int t0 = split * a.rows_per_split;
  const int t_new = T - n;                                  // first position of the chunk itself
  const int t_end = min(T, t0 + a.rows_per_split);
  // partials per query row: one per key-range split of the ONE PASS.  (The column-sum pass of a deferred flush runs with its own,
  // coarser split of the key range — a.n_stat_parts then says how many (max, sum) pairs per row the one pass of each layer left.)
  const int NPART = (MODE == 2 && a.n_stat_parts > 0) ? a.n_stat_parts : a.n_split;
  const size_t head_row = ((size_t)(a.layer_begin + ll) * a.n_kv_heads + h) * a.cap;
  const int32_t* const slot_row = a.slot_of_pos + head_row;
  const float cexp = EKV_LOG2E * (1.f / a.sm_div);          // p = 2^(s_raw * cexp - ...)
  const bool stream_once = a.n_qblocks == 1;                // every K/V row is read by exactly one workgroup of this launch

  const char* const k_old = reinterpret_cast<const char*>(a.k + head_row * D);
  const char* const v_old = reinterpret_cast<const char*>(a.v + head_row * D);
  // this launch's new rows of the head: row i at + i * kvrs bytes (ekv_step.kv_*_stride; dense: kvrs = 2 * D)
  const char* const k_nw = reinterpret_cast<const char*>(a.k_new + (size_t)ll * a.n_kv_heads * n * D + (size_t)h * a.kv_hs);
  const char* const v_nw = reinterpret_cast<const char*>(a.v_new + (size_t)ll * a.n_kv_heads * n * D + (size_t)h * a.kv_hs);
  const uint32_t kvrs = (uint32_t)a.kv_ts * 2u;

  // K/V tiles go global -> LDS by LDS-DMA (global_load_lds_dwordx4: no staging registers, no ds_write): instruction p of wave w
  // fills the 1 KB piece w * LPT + p of the tile = RPI whole rows, lane i -> 16-byte chunk i of the piece.  The LDS image is
  // lane-linear, so the swizzle sits on the SOURCE address: the lane that fills physical chunk c of row r fetches logical chunk
  // c ^ swz(r) (cdna_hip_programming.md rule 21).  K: swz = r & 15 (D = 128; conflict-free ds_read_b128 row gathers: 16 lanes
  // with 16 different rows hit 16 different chunks), V: swz = (r & 3) << 2 (conflict-free ds_read_b64_tr_b16 of 4 rows x 64 B).
  // Piece p of this wave = rows row0 + p * RPI (+ the lane's row inside the piece is part of row0).  A wave's LPT pieces are 16
  // consecutive rows starting at a multiple of 16, so the swizzles split into a lane part and a per-piece CONSTANT:
  //   K chunk of piece p = k16 ^ KX(p),  V chunk = v16 for every piece
  // — three loop-invariant registers instead of 3 * LPT (which the exact pass could not afford: it ran on the per-lane general
  // address form alone, ~180 of its ~365 VALU instructions per tile).
  static_assert((LPT * RPI) % 16 == 0, "a wave stages a multiple of 16 consecutive rows per tile");
  const int row0 = wave * (LPT * RPI) + lane / PPR;
  const int k16 = ((lane % PPR) ^ (D == 128 ? ((lane / PPR) & 15) : (((lane / PPR) >> 1) & 7))) * 16;
  const int v16 = ((lane % PPR) ^ ((D == 128 ? ((lane / PPR) & 3) : (((lane / PPR) >> 1) & 1)) << 2)) * 16;
#define EKW_KX(p) (D == 128 ? (((p) & 3) << 6) : (((p) & 1) << 6))
  // this lane's K row of a key block (ds_read_b128 of logical chunk 2*ks + hi)
  const int ksw_l = D == 128 ? (c31 & 15) : ((c31 >> 1) & 7);
  // V^T operand reads (ds_read_b64_tr_b16): the 16 lanes of group G fetch 4 key rows x 16 columns (d = db*32 + 16*(G&1) + c),
  // lane c supplies row (c >> 2), 8-byte piece (c & 3).  The 16-byte chunk index is XORed with the row's swizzle.
  const int vsw_l = D == 128 ? (c >> 2) : ((c >> 3) & 1);
  const int v_lane = (c >> 2) * RSV + 32 * (G & 1) + 16 * ((c & 3) >> 1) + 8 * (c & 1);
  // key rows of the wave's 32-key block a PV operand takes (P^T from the S^T accumulators): k-slots j < 4 <-> keys
  // 16m + 4hi + j, j >= 4 <-> 16m + 8 + 4hi + (j - 4)
  const int v_r0 = 4 * hi, v_r1 = 8;

  // MODE 2: this workgroup's slice of the column sums starts at zero; the owner lane of a column (wave (0, wk), lane & 31 of
  // the tile that holds it; upper half-wave = the squares) accumulates into it
  float* const col_base = MODE == 2 ? a.colsum + ((((size_t)ll * a.n_kv_heads + h) * a.n_col_parts + qg) * 2 + hi) * a.t_pad : nullptr;
  // (a chunk step — ONE query block per head — writes every column sum exactly once: no zero-fill, no read-modify-write.  Round 5: the
  //  fill + the re-read were 84 MB of traffic per configs[3] step and 12 us of the pass, measured by a mock.)
  const bool cs_once = MODE == 2 && a.n_qblocks == 1;
  if (MODE == 2 && wq == 0 && !cs_once) {
    for (int kt = t0; kt < t_end; kt += TK) {
#pragma unroll
      for (int kb = 0; kb < KPW; ++kb) {
        const int j = kt + (wk * KPW + kb) * 32 + c31;
        if (j < a.t_pad) col_base[j] = 0.f;
      }
    }
  }

  const int nqb_loop = MODE == 2 ? (a.n_qblocks - qg + QG - 1) / QG : 1;
  for (int qi = 0; qi < nqb_loop; ++qi) {
    // (one-pass / statistics launches: query blocks in DESCENDING order of their id — block b of a causal prefix streams
    //  (b + 1) x qb_rows keys and workgroups are dispatched in id order, longest first)
    const int qb = MODE == 2 ? qg + qi * QG : a.n_qblocks - 1 - (int)(blockIdx.y % a.n_qblocks);
    const int i0 = qb * a.qb_rows, nb = min(a.qb_rows, n - i0);   // queries [i0, i0 + nb) of the chunk
    const int NR = rep * nb;                                       // rows of this block: row = (i - i0) * rep + r
    const int t1 = min(t_end, t_new + i0 + nb);                    // causal bound of the block
    const int n_tiles = t1 > t0 ? (t1 - t0 + TK - 1) / TK : 0;

    // "query = lane" view (B operand of S^T, columns of the S^T / O^T accumulators)
    const int rowL = wq * 32 + c31;
    const bool okL = rowL < NR;
    const int rL = okL ? rowL % rep : 0, iL = okL ? i0 + rowL / rep : i0;

    // keys at or beyond this position are masked for EVERY row of this wave (its last query's causal bound): key blocks starting
    // there are skipped outright — on the two diagonal tiles of a dense-prefix block that is 6 of 16 (wave, key block) units
    const int kb_lim = min(t1, t_new + i0 + (min(NR, wq * 32 + 32) - 1) / rep + 1);

    // Q operand of this lane's query row: d = 16*ks + 8*hi + [0, 8) — the same registers serve as B of K.Q^T and A of Q.K^T
    ekv_h8 qreg[KS], qlo[ROPE ? KS : 1];
    {
      // (wave-uniform base of the KV head's rep query heads + a 32-bit lane offset: a per-lane 64-bit pointer here is hoisted out of
      //  the query-block loop and was the last spilled pair of the column-sum pass)
      const char* const qb_ = ekw_uniform(reinterpret_cast<const char*>(a.q + (size_t)ll * a.n_q_heads * n * D + (size_t)(h * rep) * a.q_hs));
      const uint32_t qoff = (uint32_t)(rL * a.q_hs + iL * a.q_ts + 8 * hi) * 2u;      // (ekv_step.q_*_stride; dense: (rL * n + iL) * D)
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        qreg[ks] = *reinterpret_cast<const ekv_h8*>(qb_ + (qoff + 32u * ks));
        if (!okL) qreg[ks] = ekv_h8{0, 0, 0, 0, 0, 0, 0, 0};
      }
      if (MODE == 0 && a.q_keep != nullptr && okL && split == 0 && wk == 0) {
        // deferred column-sum pass: the layer's (raw) queries are kept in the workspace slice of this layer
        char* const kb_ = reinterpret_cast<char*>(a.q_keep + ((size_t)ll * a.n_q_heads + h * rep) * n * D);
        const uint32_t koff = (uint32_t)((rL * n + iL) * D + 8 * hi) * 2u;      // (the kept copies are dense)
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) *reinterpret_cast<ekv_h8*>(kb_ + (koff + 32u * ks)) = qreg[ks];
      }
      if (ROPE) {
        // q' = q*cos[pos] + rotate_half(q)*sin[pos] at the query's position pos = T - n + i (llama_patch.py:311, :326), fp32 with the
        // reference's rounding, split into fp16 hi + lo — IN the lane: fragment ks holds d = 16*ks + 8*hi + e, its partner d + D/2 is
        // fragment ks + KS/2 of the same lane.  (Rounds 1-3 and the 16x16 kernel: ekv_rope_q_kernel + a [2][rows][D] workspace — one
        // more launch per step, 60 us of table-bound traffic at the configs[4] shape, 7 us per one-layer call.)
        const int pos = t_new + iL;
        const float* cb = a.rope_cos + (size_t)pos * D + 8 * hi;
        const float* sb = a.rope_sin + (size_t)pos * D + 8 * hi;
#pragma unroll
        for (int ks = 0; ks < KS / 2; ++ks) {
          const ekv_f4w c0 = *reinterpret_cast<const ekv_f4w*>(cb + 16 * ks), c1 = *reinterpret_cast<const ekv_f4w*>(cb + 16 * ks + 4);
          const ekv_f4w s0 = *reinterpret_cast<const ekv_f4w*>(sb + 16 * ks), s1 = *reinterpret_cast<const ekv_f4w*>(sb + 16 * ks + 4);
          const ekv_h8 x = qreg[ks], y = qreg[ks + KS / 2];
          ekv_h8 xh, xl, yh, yl;
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const float cv = e < 4 ? c0[e & 3] : c1[e & 3], sv = e < 4 ? s0[e & 3] : s1[e & 3];
            const float lo_ = (float)x[e] * cv + (-(float)y[e]) * sv;
            const float hi_ = (float)y[e] * cv + (float)x[e] * sv;
            xh[e] = (ekv_e)lo_;
            xl[e] = (ekv_e)(lo_ - (float)xh[e]);
            yh[e] = (ekv_e)hi_;
            yl[e] = (ekv_e)(hi_ - (float)yh[e]);
          }
          qreg[ks] = xh;
          qlo[ks] = xl;
          qreg[ks + KS / 2] = yh;
          qlo[ks + KS / 2] = yl;
        }
      }
    }

    // MODE 2: -log2(sum_j exp(s_ij)) of the block's rows, from the (max, sum) partials of the statistics pass — computed once per
    // row by the first threads and handed to the lanes through LDS ("query = register" view: accumulator register r <-> row
    // wq*32 + (r&3) + 8*(r>>2) + 4*hi needs 16 of them per lane; 16 pointer chains per lane cost 150 spilled registers)
    const int rsh = REP == 1 ? 0 : (REP == 2 ? 1 : (REP == 4 ? 2 : 31 - __builtin_clz((unsigned)rep)));      // MODE 2 runs with rep in {1, 2, 4, 8, 16}
    if (MODE == 2) {
      for (int row = tid; row < NWQ * 32; row += NT) {
        float v = EKV_NEG_INF;
        if (row < NR) {
          const float* sp = a.stats + (((size_t)ll * a.n_q_heads + h * rep + (row & (rep - 1))) * n + i0 + (row >> rsh)) * NPART * 2;
          float mm = kWFloor;
          for (int i = 0; i < NPART; ++i) mm = fmaxf(mm, sp[2 * i]);
          float ls = 0.f;
          for (int i = 0; i < NPART; ++i) ls += sp[2 * i + 1] * __builtin_amdgcn_exp2f(sp[2 * i] - mm);
          v = -(mm + __builtin_amdgcn_logf(ls));       // v_log_f32 = log2
        }
        sLse[row] = v;
      }
    }

    // append: the (split, query block) that owns the new positions [t_new+i0, t_new+i0+nb) within its key range copies their
    // K/V rows into the cache slots.  Nobody reads these slots in this launch: new rows are always taken from k_new / v_new.
    if (MODE == 0 && EKW_EXP != 3) {
      const int j_lo = max(t_new + i0, t0), j_hi = min(t_new + i0 + nb, t1);
      const int n_pieces = (j_hi - j_lo) * PPR;              // 16-byte pieces of the block's new rows inside this key range
      if (n_pieces > 0) {                                    // (workgroup-uniform)
        // Every piece's slot entry and its K / V bytes are requested TOGETHER, then stored: one round trip.  (Round 5: the plain loop
        // `for piece: slot -> load -> store` was a chain of three dependent round trips per iteration, six iterations for a 96-row
        // block — ~15 us in front of the first tile of the one workgroup of a head that owns the new rows; a one-layer launch ends
        // when that workgroup does.)
        constexpr int APT = (128 * PPR + NT - 1) / NT;       // pieces per thread (a block has at most 128 / rep <= 128 new rows)
        int a_slot[APT];
        ekv_u4 a_k[APT], a_v[APT];                           // (ext-vector type: a HIP uint4 struct array lands in the private segment)
#pragma unroll
        for (int u = 0; u < APT; ++u) {
          const int piece = min(tid + u * NT, n_pieces - 1);   // unconditional (clamped) loads
          a_slot[u] = slot_row[j_lo + piece / PPR];
          const uint32_t po = (uint32_t)(j_lo - t_new + piece / PPR) * kvrs + (uint32_t)(piece % PPR) * 16u;
          a_k[u] = *reinterpret_cast<const ekv_u4*>(k_nw + po);
          a_v[u] = *reinterpret_cast<const ekv_u4*>(v_nw + po);
        }
#pragma unroll
        for (int u = 0; u < APT; ++u) {
          const int piece = tid + u * NT;
          if (piece < n_pieces) {
            const size_t off = (head_row + a_slot[u]) * D;
            reinterpret_cast<ekv_u4*>(a.k_w + off)[piece % PPR] = a_k[u];
            reinterpret_cast<ekv_u4*>(a.v_w + off)[piece % PPR] = a_v[u];
          }
        }
      }
    }

    // ---- staging ------------------------------------------------------------------------------------------------------
    int slot_nx[LPT];
    const int kt_last = t0 + (n_tiles > 0 ? n_tiles - 1 : 0) * TK;
    // cache rows of this range end here; rows from there on are the launch's new rows.  a.new_in_cache (the DEFERRED column-sum pass
    // of a layer-per-call model: the one pass of each layer appended its rows long ago, k_new is gone): every row is a cache row,
    // read through the slot map — the causal limits still use t_new
    const int t_src = (MODE == 2 && a.new_in_cache) ? T : t_new;
    const int hi_old = min(t1, t_src);
    auto load_slots = [&](int kt) __attribute__((always_inline)) {        // slot entries of tile kt (clamped: tiles past the range re-read the last one)
      kt = min(kt, kt_last);
#pragma unroll
      for (int p = 0; p < LPT; ++p) slot_nx[p] = slot_row[max(min(kt + row0 + p * RPI, hi_old - 1), 0)];
    };
    // Three workgroup-uniform address cases (the DMAs themselves are the same 2 * LPT per tile in each):
    //   all new   the tile lies inside this launch's own rows (every tile of a dense prefix): contiguous, no slot map —
    //             uniform base + a loop-invariant lane offset
    //   all old   the tile lies inside the cache rows: slot entry * row bytes + the lane's chunk
    //   mixed     the tile that straddles t_new or the end of the range: per-lane clamp and select
    // (the per-lane form alone was 113 of the ~275 VALU instructions of a dense-prefix tile)
    auto stage_dma = [&](int kt, const int buf) __attribute__((always_inline)) {        // needs slot_nx of tile kt
      kt = min(kt, kt_last);
      char* const kdst = sK + buf * KBUF + wave * LPT * 1024;      // wave-uniform; piece p at + p * 1024, lane i at + 16 * i
      char* const vdst = sV + buf * VBUF + wave * LPT * 1024;
      if (kt >= t_src && kt + TK <= t1) {
        const char* const kb_ = ekw_uniform(k_nw + (size_t)(kt - t_new) * kvrs);
        const char* const vb_ = MODE == 0 ? ekw_uniform(v_nw + (size_t)(kt - t_new) * kvrs) : nullptr;
#pragma unroll
        for (int p = 0; p < (EKW_NODMA == 2 ? 1 : LPT); ++p) {
          const uint32_t ro = (uint32_t)(row0 + p * RPI) * kvrs;
          ekw_dma16(kb_ + (ro + (uint32_t)(k16 ^ EKW_KX(p))), kdst + p * 1024, stream_once);
          if (MODE == 0) ekw_dma16(vb_ + (ro + (uint32_t)v16), vdst + p * 1024, stream_once);
        }
      } else if (kt + TK <= hi_old) {
#pragma unroll
        for (int p = 0; p < LPT; ++p) {
          const uint32_t off = (uint32_t)slot_nx[p] * (uint32_t)(2 * D);
          ekw_dma16(k_old + (off + (uint32_t)(k16 ^ EKW_KX(p))), kdst + p * 1024, stream_once);
          if (MODE == 0) ekw_dma16(v_old + (off + (uint32_t)v16), vdst + p * 1024, stream_once);
        }
      } else {
#pragma unroll
        for (int p = 0; p < LPT; ++p) {
          const int j = max(min(kt + row0 + p * RPI, t1 - 1), 0);
          const bool is_new = j >= t_src;
          const uint32_t off = is_new ? (uint32_t)(j - t_new) * kvrs : (uint32_t)slot_nx[p] * (uint32_t)(2 * D);
          // two DMAs under complementary exec masks, each from a wave-uniform base + a 32-bit lane offset (a per-lane SELECT of the
          // base pointer is a 64-bit VGPR pair per piece and tensor that hipcc hoists out of the tile loop: 16 registers, spilled at
          // 128); the empty asm keeps SimplifyCFG from sinking the two calls back into one with a selected pointer
          if (is_new) {
            ekw_dma16(k_nw + (off + (uint32_t)(k16 ^ EKW_KX(p))), kdst + p * 1024, stream_once);
            if (MODE == 0) ekw_dma16(v_nw + (off + (uint32_t)v16), vdst + p * 1024, stream_once);
            asm volatile("" ::: "memory");
          } else {
            ekw_dma16(k_old + (off + (uint32_t)(k16 ^ EKW_KX(p))), kdst + p * 1024, stream_once);
            if (MODE == 0) ekw_dma16(v_old + (off + (uint32_t)v16), vdst + p * 1024, stream_once);
          }
        }
      }
    };
    // ---- ROPE: table prefetch + in-place rotation of a landed tile -----------------------------------------------------------
    // thread -> row rr = tid / 4 of the tile and IPT chunk pairs of it; item u: physical chunk pc (low-half side plow, high-half
    // side plow ^ HC), head-dim offset d0 of its low half
    constexpr int HC = PPR / 2, IPT = ROPE ? (TK * HC) / NT : 1;
    static_assert(!ROPE || (TK * HC) % NT == 0, "rotation items do not divide over the workgroup");
    const int rr = tid / (HC / IPT);                         // HC / IPT threads per row
    const int rsw = D == 128 ? (rr & 15) : ((rr >> 1) & 7);  // the row's K swizzle (see k16)
    // Conflict classes of the rotation's LDS accesses (D = 128, two items per thread).  A `ds_read_b128` is served in four groups of four
    // lane quads — rows {0,3,5,6}, {1,2,4,7}, {8,11,13,14}, {9,10,12,15} of a wave's sixteen —, a `ds_write_b128` in groups of two
    // consecutive rows over 128-byte bank rows.  With every row taking the same physical chunks (even ones for item 0, odd ones for
    // item 1, low-half chunk first) the four rows of a read group met on the same four slots (4-way) and the two rows of a write group on
    // the same four (2-way): a third of the RoPE passes' LDS cycles (`SQ_LDS_BANK_CONFLICT` 47 M per launch, rounds 3-5).  Row class
    // rr & 3 — distinct within every read group, of different parity within every write group — now picks the item order (bit 0) and
    // which chunk of a pair comes first (bit 1): sixteen distinct slots per read group, eight per write group.  Same rows per
    // instruction as before, so the table loads keep their 16-row footprint (round 4's one-row-per-lane mapping lost 4.5 % to them).
    constexpr bool kRotCls = ROPE && D == 128 && IPT == 2 && EKW_ROT_CLS;
    const int rot_odd = kRotCls ? (rr & 1) : 0;
    const bool rot_flip = kRotCls && (rr & 2);
    const float rot_sgn = rot_flip ? -1.f : 1.f;             // (a multiplication by +-1, exact, so that hipcc packs it: a select was 16 v_cndmask per tile)
    ekv_f4w tcs[IPT][2], tsn[IPT][2];                        // cos / sin of the row's position at d0 .. d0 + 7
    auto rope_tables = [&](int kt) __attribute__((always_inline)) {       // request the table values of tile kt (clamped like the tile itself)
      if (ROPE && (EKW_EXP == 4 || EKW_EXP == 6)) {
#pragma unroll
        for (int u = 0; u < IPT; ++u) tcs[u][0] = tcs[u][1] = ekv_f4w{1.f, 1.f, 1.f, 1.f}, tsn[u][0] = tsn[u][1] = ekv_f4w{0.f, 0.f, 0.f, 0.f};
      } else if (ROPE) {
        kt = min(kt, kt_last);
        const int j = min(kt + rr, t1 - 1);
        const float* cb = a.rope_cos + (size_t)j * D;
        const float* sb = a.rope_sin + (size_t)j * D;
#pragma unroll
        for (int u = 0; u < IPT; ++u) {
          const int pc = (tid % (HC / IPT)) * IPT + (u ^ rot_odd);
          const int d0 = ((pc ^ rsw) & (HC - 1)) * 8;
          tcs[u][0] = *reinterpret_cast<const ekv_f4w*>(cb + d0);
          tcs[u][1] = *reinterpret_cast<const ekv_f4w*>(cb + d0 + 4);
          tsn[u][0] = *reinterpret_cast<const ekv_f4w*>(sb + d0);
          tsn[u][1] = *reinterpret_cast<const ekv_f4w*>(sb + d0 + 4);
        }
      }
    };
    auto rope_rotate = [&](const int buf) __attribute__((always_inline)) {   // needs the table values of the tile in `buf`; ends with a barrier
      if (ROPE && EKW_EXP != 6) {
        char* const krow = sK + buf * KBUF + rr * RSK;
        char* const lrow = sKlo + rr * RSK;
#pragma unroll
        for (int u = 0; u < IPT; ++u) {
          const int pc = (tid % (HC / IPT)) * IPT + (u ^ rot_odd);
          // x: the chunk this thread reads first — the physical chunk that holds d0 .. d0 + 7 (rows of classes 0 / 1) or its partner
          // d0 + D/2 .. (classes 2 / 3); y: the other one
          const int plow = (pc ^ ((pc ^ rsw) & HC)) ^ (rot_flip ? HC : 0);
          const ekv_h8 x = *reinterpret_cast<const ekv_h8*>(krow + plow * 16);
          const ekv_h8 y = *reinterpret_cast<const ekv_h8*>(krow + (plow ^ HC) * 16);
          ekv_h8 xh, xl, yh, yl;
          if (EKW_EXP == 5) {
            xh = x, yh = y, xl = y, yl = x;
          } else
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const float cv = tcs[u][e >> 2][e & 3], sv0 = tsn[u][e >> 2][e & 3];
            // k' = k*cos + rotate_half(k)*sin, rotate_half = (-k[d + D/2], k[d - D/2]) (llama_patch.py:13-17, :312, :327): the low-half
            // element takes -sin of its partner, the high-half element +sin — the sign goes with the chunk read first (exact: a sign flip)
            const float sv = kRotCls ? sv0 * rot_sgn : sv0;
            const float lo_ = (float)x[e] * cv + (-(float)y[e]) * sv;
            const float hi_ = (float)y[e] * cv + (float)x[e] * sv;
            xh[e] = (ekv_e)lo_;
            xl[e] = (ekv_e)(lo_ - (float)xh[e]);
            yh[e] = (ekv_e)hi_;
            yl[e] = (ekv_e)(hi_ - (float)yh[e]);
          }
          *reinterpret_cast<ekv_h8*>(krow + plow * 16) = xh;
          *reinterpret_cast<ekv_h8*>(krow + (plow ^ HC) * 16) = yh;
          *reinterpret_cast<ekv_h8*>(lrow + plow * 16) = xl;
          *reinterpret_cast<ekv_h8*>(lrow + (plow ^ HC) * 16) = yl;
        }
        ekv_lds_barrier();
      }
    };
    // per-wave state
    ekv_f16v oacc[DB];
#pragma unroll
    for (int db = 0; db < DB; ++db)
#pragma unroll
      for (int r = 0; r < 16; ++r) oacc[db][r] = 0.f;
    float m_run = kWFloor, l_run = 0.f;      // MODE 0 / 1: running max (raw logits) and this lane's share of the row sum

    ekv_lds_barrier();                       // tile buffers free (previous query block / epilogue exchange fully consumed)
    if (n_tiles > 0) {
      load_slots(t0);
      stage_dma(t0, 0);
      load_slots(t0 + TK);
      rope_tables(t0);
      ekw_tile_barrier();
    }

    for (int t = 0; t < n_tiles; ++t) {
      const int kt = t0 + t * TK, buf = t & 1, kg = wk * KPW * 32;   // kg: first key of this wave's KPW blocks within the tile
      // wave-uniform: this wave's keys start inside the range (later blocks are masked) and it has rows at all (a 96-row chunk
      // leaves the fourth query wave of a 128-row workgroup without work: it only takes its share of the LDS-DMA)
      const bool active = EKW_EXP != 1 && kt + kg < t1 && wq * 32 < NR;
      // tiles that reach the chunk's own positions or the end of the range need the causal / range mask (wave-uniform test)
      const bool edge = kt + kg + 32 * KPW > min(t1, t_new + i0 + 1);

      // MODE 2: the column sums the query waves left for the PREVIOUS tile are picked up by the owner lanes.  The global
      // read-modify-write is ISSUED here, ahead of this iteration's tile loads, unconditionally (clamped address: loads inside a
      // branch upset hipcc's vmcnt bookkeeping), and COMPLETED where the staged tile is awaited anyway (vmcnt retires in order).
      float xsum[KPW], gprev[KPW];
      const int acc_j = max(kt - TK + kg + c31, 0);      // column of key block 0 of the previous tile (block kb: + 32 * kb)
      bool do_acc = false;
      if (MODE == 2) {
        do_acc = wq == 0 && t > 0 && (kt - TK + kg < t1);
#pragma unroll
        for (int kb = 0; kb < KPW; ++kb) {
          // (unconditional load — loads inside a branch upset hipcc's vmcnt bookkeeping — of one shared word when nothing is to be re-read)
          const float gv = col_base[cs_once ? 0 : acc_j + 32 * kb];
          gprev[kb] = cs_once ? 0.f : gv;
          xsum[kb] = 0.f;
        }
        if (do_acc) {
#pragma unroll
          for (int kb = 0; kb < KPW; ++kb) {
            const float* xp = sX + ((((t - 1) & 1) * NKB + wk * KPW + kb) * NWQ) * 64 + lane;
#pragma unroll
            for (int w = 0; w < NWQ; ++w)
              if (w * 32 < NR) xsum[kb] += xp[w * 64];      // (query waves without rows wrote nothing)
          }
        }
      }

      ekv_f16v s[KPW];
      ekv_h8 bP[KPW][2];
      float alpha = 1.f;
      auto qk = [&](const int kb) __attribute__((always_inline)) {      // S^T (MODE 0 / 1) or S (MODE 2) of key block kb
        const char* kbase = sK + buf * KBUF + (kg + 32 * kb + c31) * RSK;
#pragma unroll
        for (int r = 0; r < 16; ++r) s[kb][r] = 0.f;
        EKW_PRIO(1);
#if EKW_KPREFETCH
        // all K fragments of the block first (KS x 4 VGPRs), then the MFMA chain: hipcc otherwise cycles two fragment registers
        // and every second MFMA waits for a fresh LDS round trip
        ekv_h8 kfv[KS];
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) kfv[ks] = *reinterpret_cast<const ekv_h8*>(kbase + (((2 * ks + hi) ^ ksw_l) << 4));
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
          if (MODE == 2) s[kb] = EKV_MFMA_32x32x16(qreg[ks], kfv[ks], s[kb], 0, 0, 0);
          else s[kb] = EKV_MFMA_32x32x16(kfv[ks], qreg[ks], s[kb], 0, 0, 0);
        }
#else
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
          const ekv_h8 kf = *reinterpret_cast<const ekv_h8*>(kbase + (((2 * ((EKW_DM & 8) ? 0 : ks) + hi) ^ ksw_l) << 4));
          if (MODE == 2) s[kb] = EKV_MFMA_32x32x16(qreg[ks], kf, s[kb], 0, 0, 0);   // S[q][key]
          else s[kb] = EKV_MFMA_32x32x16(kf, qreg[ks], s[kb], 0, 0, 0);            // S^T[key][q]
          if (ROPE && EKW_EXP != 7) {   // (kh + kl).(qh + ql) ~= kh.qh + kl.qh + kh.ql
            const ekv_h8 kl = *reinterpret_cast<const ekv_h8*>(sKlo + (kg + 32 * kb + c31) * RSK + (((2 * ks + hi) ^ ksw_l) << 4));
            if (MODE == 2) {
              s[kb] = EKV_MFMA_32x32x16(qreg[ks], kl, s[kb], 0, 0, 0);
              s[kb] = EKV_MFMA_32x32x16(qlo[ks], kf, s[kb], 0, 0, 0);
            } else {
              s[kb] = EKV_MFMA_32x32x16(kl, qreg[ks], s[kb], 0, 0, 0);
              s[kb] = EKV_MFMA_32x32x16(kf, qlo[ks], s[kb], 0, 0, 0);
            }
          }
        }
#endif
        EKW_PRIO(0);
      };
      auto pv = [&](const int kb) __attribute__((always_inline)) {      // O^T += V^T . P^T over key block kb
        const char* vb = sV + buf * VBUF + (kg + 32 * kb + v_r0) * RSV + v_lane;
        EKW_PRIO(1);
        if (EKW_DM & 8) {
          const char* vp = vb + (vsw_l << 6);
          const ekv_h4 v_lo = __builtin_bit_cast(ekv_h4, __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) ekv_s4*)(vp)));
          const ekv_h4 v_hi = __builtin_bit_cast(ekv_h4, __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) ekv_s4*)(vp + v_r1 * RSV)));
          const ekv_h8 aV = {v_lo[0], v_lo[1], v_lo[2], v_lo[3], v_hi[0], v_hi[1], v_hi[2], v_hi[3]};
#pragma unroll
          for (int db = 0; db < DB; ++db)
#pragma unroll
            for (int m = 0; m < 2; ++m) oacc[db] = EKV_MFMA_32x32x16(aV, bP[kb][m], oacc[db], 0, 0, 0);
          EKW_PRIO(0);
          return;
        }
#pragma unroll
        for (int db = 0; db < DB; ++db) {
          const int vo = (db ^ vsw_l) << 6;
#pragma unroll
          for (int m = 0; m < 2; ++m) {
            const char* vp = vb + (16 * m) * RSV + vo;
            const ekv_h4 v_lo = __builtin_bit_cast(ekv_h4, __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) ekv_s4*)(vp)));
            const ekv_h4 v_hi = __builtin_bit_cast(ekv_h4, __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) ekv_s4*)(vp + v_r1 * RSV)));
            const ekv_h8 aV = {v_lo[0], v_lo[1], v_lo[2], v_lo[3], v_hi[0], v_hi[1], v_hi[2], v_hi[3]};
            oacc[db] = EKV_MFMA_32x32x16(aV, bP[kb][m], oacc[db], 0, 0, 0);
          }
        }
        EKW_PRIO(0);
      };
      // tile t+1 -> the other LDS buffer (last read in iteration t-1; it lands while this tile is consumed), slot entries of tile t+2
      // ROPE: the landed tile is rotated in place (hi) and into sKlo (lo) by the whole workgroup; the lo buffer and this tile's raw
      // rows were last touched before the barrier that ended the previous iteration
      // (issued BEFORE the rotation — table registers touched first so that hipcc's wait for them does not drain the DMAs, raw barrier in
      //  the rotation —, the DMA flies during the rotation too: correct, and slower, configs[4] one pass 1198-1200 vs 1174 us same box)
      rope_rotate(buf);
      if (EKW_EXP != 2 && EKW_NODMA != 1) stage_dma(EKW_NODMA == 3 ? t0 : kt + TK, buf ^ 1);
      load_slots(kt + 2 * TK);
      // (the next tile's table values (L2) are requested by mode 0 in front of its PV phase, when the S^T registers have died —
      //  at the end of the iteration their round trip is exposed: configs[4] pass 1382 -> 1307 us — and by the column-sum pass at its
      //  end: requested here, across the whole tile, that pass went 869 -> 1054 us)

      if (MODE != 2) {
        if (active) {
#pragma unroll
          for (int kb = 0; kb < KPW; ++kb) {
            if (EKW_DM & 4) {
              const float tv = (float)(kt & 63) * 1e-3f;
#pragma unroll
              for (int r = 0; r < 16; ++r) s[kb][r] = tv + (float)(r + 16 * kb) * 1e-2f;
            } else if (kt + kg + 32 * kb < kb_lim) qk(kb);
            else {
#pragma unroll
              for (int r = 0; r < 16; ++r) s[kb][r] = EKV_NEG_INF;
            }
          }
          // ---- online softmax, query = lane; register r of block kb <-> key kt + kg + 32*kb + (r&3) + 8*(r>>2) + 4*hi ------------
          if (edge) {
            asm volatile("" ::: "memory");     // (keeps the branch a branch: if-converted, the mask is 45 VALU instructions on EVERY tile)
            const int jlim = min(t1, t_new + iL + 1) - (kt + kg + 4 * hi);   // first masked key offset for this query
#pragma unroll
            for (int kb = 0; kb < KPW; ++kb)
#pragma unroll
              for (int r = 0; r < 16; ++r)
                if (32 * kb + (r & 3) + 8 * (r >> 2) >= jlim) s[kb][r] = EKV_NEG_INF;
          }
          // One-pass scored steps under RoPE-on-read (TOVA, or a plan that forces one pass) leave the raw logits for the scorer, as the
          // 16x16 kernel does for small query blocks — single-block steps only, where every key of the range is visited.  Quotient units
          // by the SAME multiplication as the row statistics below, so that the row maximum the scorer subtracts is the maximum of what
          // it reads.  One 16-byte store per register quad: the two half-waves of a query complete 32 bytes, the four quads of a key
          // block a 128-byte line.  The row bookkeeping is rebuilt from an opaque lane id inside the branch: kept alive across the tile
          // loop it was two spilled registers of the 256-register build.
          // (Measured at the configs[4] shape, same box: the export costs what 2.6 GB of writes cost — one pass 1155 -> 1590 us — and the
          //  scorer's sweep over the logits 600 us: 2190 us per step against 2205 us with the column-sum pass, so roco / h2o steps keep
          //  the two passes; a key-major workspace whose stores are full 128-byte lines was SLOWER, 1640-1750 us: not the coalescing.)
          if (LOGITS && a.logits != nullptr) {
            int lx = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
            asm volatile("" : "+v"(lx));      // (opaque: not hoisted out of the tile loop)
            const int rowX = wq * 32 + (lx & 31);
            if (rowX < NR) {
              float smd = a.sm_div;
              asm volatile("" : "+v"(smd));
              const float inv = 1.f / smd;
              // (rep is a power of two <= 16 here — ekv_chunk_wide —: the division by a run-time rep was a hoisted magic number, one more
              //  live register and with it a spilled LDS address in the QK loop of EVERY RoPE step)
              const int xsh = 31 - __builtin_clz((unsigned)rep);
              float* lrow = a.logits + (((size_t)ll * a.n_q_heads + h * rep + (rowX & (rep - 1))) * n + (i0 + (rowX >> xsh))) * a.t_pad + (kt + kg + 4 * (lx >> 5));
#pragma unroll
              for (int kb = 0; kb < KPW; ++kb)
#pragma unroll
                for (int q4 = 0; q4 < 4; ++q4)
                  *reinterpret_cast<ekv_f4w*>(lrow + 32 * kb + 8 * q4) =
                      ekv_f4w{s[kb][4 * q4] * inv, s[kb][4 * q4 + 1] * inv, s[kb][4 * q4 + 2] * inv, s[kb][4 * q4 + 3] * inv};
            }
          }
          if (EKW_DM & 1) {
            l_run += s[0][0];
#pragma unroll
            for (int kb = 0; kb < KPW; ++kb)
#pragma unroll
              for (int m = 0; m < 2; ++m)
#pragma unroll
                for (int j = 0; j < 8; ++j) bP[kb][m][j] = (ekv_e)s[kb][8 * m + j];
          } else {
          float mx = kWFloor;
#pragma unroll
          for (int kb = 0; kb < KPW; ++kb) {
            const float m0 = ekw_max3(ekw_max3(s[kb][0], s[kb][1], s[kb][2]), ekw_max3(s[kb][3], s[kb][4], s[kb][5]), ekw_max3(s[kb][6], s[kb][7], s[kb][8]));
            const float m1 = ekw_max3(ekw_max3(s[kb][9], s[kb][10], s[kb][11]), ekw_max3(s[kb][12], s[kb][13], s[kb][14]), s[kb][15]);
            mx = ekw_max3(m0, m1, mx);
          }
          float mlo, mhi;
          ekw_halves(mx, mlo, mhi);
          const float mn = ekw_max3(mlo, mhi, m_run);
          alpha = __builtin_amdgcn_exp2f((m_run - mn) * cexp);
          const float nm = -mn * cexp;
          float ls = 0.f;
#pragma unroll
          for (int kb = 0; kb < KPW; ++kb)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
              const float p = __builtin_amdgcn_exp2f(fmaf(s[kb][r], cexp, nm));
              s[kb][r] = p;
              ls += p;
            }
          l_run = l_run * alpha + ls;
          m_run = mn;
          if (MODE == 0) {
#pragma unroll
            for (int kb = 0; kb < KPW; ++kb)
#pragma unroll
              for (int m = 0; m < 2; ++m)
#pragma unroll
                for (int j = 0; j < 8; ++j) bP[kb][m][j] = (ekv_e)s[kb][8 * m + j];
          }
          }
        }
        if (MODE == 0) rope_tables(kt + TK);
        // ---- O^T = O^T * alpha + V^T . P^T --------------------------------------------------------------------------------
        if (MODE == 0 && active) {
          if (__builtin_amdgcn_ballot_w64(alpha != 1.f) != 0ull) {
            asm volatile("" ::: "memory");
#pragma unroll
            for (int db = 0; db < DB; ++db) oacc[db] = oacc[db] * alpha;
          }
#pragma unroll
          for (int kb = 0; kb < KPW; ++kb)
            if (EKW_DM & 2) oacc[kb & (DB - 1)][0] += (float)bP[kb][0][0] + (float)bP[kb][1][3];
            else if (kt + kg + 32 * kb < kb_lim) pv(kb);
        }
      } else {
        // ---- column-sum pass, key = lane; register r <-> query row wq*32 + (r&3) + 8*(r>>2) + 4*hi.  One key block at a time
#pragma unroll
        for (int kb = 0; kb < KPW; ++kb) {
          const bool kb_on = active && kt + kg + 32 * kb < kb_lim;
          if (active && !kb_on) sX[(((t & 1) * NKB + wk * KPW + kb) * NWQ + wq) * 64 + lane] = 0.f;
          if (kb_on) {
            qk(kb);
            const int j = kt + kg + 32 * kb + c31;
            if (edge) {
              asm volatile("" ::: "memory");
              // row of register r = base + c_r with base = wq*32 + 4*hi, c_r = (r&3) + 8*(r>>2): (base + c_r) >> rsh = (base >> rsh) +
              // (c_r >> rsh) for every rep <= 16 (no carry out of the low bits) — ONE lane value against 16 scalar constants, nothing
              // per register that hipcc could hoist out of the tile loop
              const int jj = j >= t1 ? 0x7fffffff : j - (t_new + i0 + 1 + ((wq * 32 + 4 * hi) >> rsh));
#pragma unroll
              for (int r = 0; r < 16; ++r)
                if (jj >= (((r & 3) + 8 * (r >> 2)) >> rsh)) s[kb][r] = EKV_NEG_INF;
            }
            // (-lse2 of this lane's 16 rows: four 16-byte LDS reads instead of 16 live registers)
#pragma unroll
            for (int q4 = 0; q4 < 4; ++q4) {
              const ekv_f4w nl = *reinterpret_cast<const ekv_f4w*>(sLse + wq * 32 + 8 * q4 + 4 * hi);
              // (two v_pk_fma_f32 instead of four v_fma_f32: the same per-element result)
              typedef float ekw_f2 __attribute__((ext_vector_type(2)));
              const ekw_f2 a01 = __builtin_elementwise_fma(ekw_f2{s[kb][4 * q4], s[kb][4 * q4 + 1]}, ekw_f2{cexp, cexp}, ekw_f2{nl[0], nl[1]});
              const ekw_f2 a23 = __builtin_elementwise_fma(ekw_f2{s[kb][4 * q4 + 2], s[kb][4 * q4 + 3]}, ekw_f2{cexp, cexp}, ekw_f2{nl[2], nl[3]});
              s[kb][4 * q4] = __builtin_amdgcn_exp2f(a01.x);
              s[kb][4 * q4 + 1] = __builtin_amdgcn_exp2f(a01.y);
              s[kb][4 * q4 + 2] = __builtin_amdgcn_exp2f(a23.x);
              s[kb][4 * q4 + 3] = __builtin_amdgcn_exp2f(a23.y);
            }
            // column sums of the GQA-folded probabilities over this lane's 16 rows (rows 4q .. 4q+3 are consecutive: the rep
            // query heads of a query sit in one register quad for rep <= 4, in the two half-waves' quads for 8 / 16); p^2 is rounded before it is summed, as the
            // reference's (p ** 2).sum
            float cs = 0.f, cq = 0.f;
            if (REP == 1) {
              // packed: even and odd registers summed side by side (v_pk_mul_f32 / v_pk_add_f32), the two halves added at the end
              typedef float ekw_f2 __attribute__((ext_vector_type(2)));
              ekw_f2 cs2 = {0.f, 0.f}, cq2 = {0.f, 0.f};
#pragma unroll
              for (int r = 0; r < 16; r += 2) {
                const ekw_f2 p2 = {s[kb][r], s[kb][r + 1]};
                cs2 += p2;
                cq2 += p2 * p2;
              }
              cs = cs2.x + cs2.y;
              cq = cq2.x + cq2.y;
            } else if (REP == 2) {
#pragma unroll
              for (int r = 0; r < 16; r += 2) {
                const float pb = (s[kb][r] + s[kb][r + 1]) * 0.5f;
                cs += pb;
                cq += pb * pb;
              }
            } else if (REP == 4) {
#pragma unroll
              for (int r = 0; r < 16; r += 4) {
                const float pb = (((s[kb][r] + s[kb][r + 1]) + s[kb][r + 2]) + s[kb][r + 3]) * 0.25f;
                cs += pb;
                cq += pb * pb;
              }
            } else {
              // rep 8 / 16: a query's heads span BOTH half-waves (rows 8g .. 8g+3 in the lower half, 8g+4 .. 8g+7 in the upper; two
              // register quads each for 16): the halves' partial sums are exchanged and the lower half counts the query
              const float inv = 1.f / (float)rep;
#pragma unroll
              for (int g2 = 0; g2 < 2; ++g2) {
                float part[2];
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                  const int r = 8 * g2 + 4 * u;
                  part[u] = ((s[kb][r] + s[kb][r + 1]) + s[kb][r + 2]) + s[kb][r + 3];
                }
                if (rep == 16) part[0] += part[1];
                float l0, h0, l1, h1;
                ekw_halves(part[0], l0, h0);
                ekw_halves(part[1], l1, h1);
                const float pb0 = (l0 + h0) * inv, pb1 = (l1 + h1) * inv;
                if (hi == 0) {
                  cs += pb0;
                  cq += pb0 * pb0;
                  if (rep == 8) {
                    cs += pb1;
                    cq += pb1 * pb1;
                  }
                }
              }
            }
            float clo, chi, qlo, qhi;
            ekw_halves(cs, clo, chi);
            ekw_halves(cq, qlo, qhi);
            sX[(((t & 1) * NKB + wk * KPW + kb) * NWQ + wq) * 64 + lane] = hi == 0 ? clo + chi : qlo + qhi;
          }
        }
      }
      if (MODE == 2 && do_acc) {
#pragma unroll
        for (int kb = 0; kb < KPW; ++kb) col_base[acc_j + 32 * kb] = gprev[kb] + xsum[kb];
      }
      if (MODE == 2) rope_tables(kt + TK);
      ekw_tile_barrier();
    }

    // MODE 2: column sums of the last tile
    if (MODE == 2 && n_tiles > 0) {
      const int t = n_tiles, kt = t0 + t * TK, kg = wk * KPW * 32;
      if (wq == 0 && (kt - TK + kg < t1)) {
#pragma unroll
        for (int kb = 0; kb < KPW; ++kb) {
          float* acc_ptr = col_base + (kt - TK + kg + 32 * kb + c31);
          const float* xp = sX + ((((t - 1) & 1) * NKB + wk * KPW + kb) * NWQ) * 64 + lane;
          float xsum = 0.f;
#pragma unroll
          for (int w = 0; w < NWQ; ++w)
            if (w * 32 < NR) xsum += xp[w * 64];
          *acc_ptr = cs_once ? xsum : *acc_ptr + xsum;
        }
      }
    }

    if (MODE == 2) continue;       // (the column sums are this pass's only product; a.score_tail: the scorer follows the loop)
    // ---- fold the key waves of a query wave through LDS (the tile buffers are free), then write ------------------------------------
    float llo, lhi;
    ekw_halves(l_run, llo, lhi);
    float l_tot = llo + lhi;
    constexpr int XS = DB * 16 + 2;       // floats per lane: (m, l, o[DB][16])
    float* const xch = reinterpret_cast<float*>(smem);
    for (int src = 1; src < NWK; ++src) {
      ekv_lds_barrier();
      float* mine = xch + (size_t)(wq * 64 + lane) * XS;
      if (wk == src) {
        mine[0] = m_run;
        mine[1] = l_tot;
#pragma unroll
        for (int db = 0; db < DB; ++db)
#pragma unroll
          for (int r = 0; r < 16; ++r) mine[2 + db * 16 + r] = oacc[db][r];
      }
      ekv_lds_barrier();
      if (wk == 0) {
        const float m1 = mine[0], l1 = mine[1];
        const float mm = fmaxf(m_run, m1);
        const float w0 = __builtin_amdgcn_exp2f((m_run - mm) * cexp), w1 = __builtin_amdgcn_exp2f((m1 - mm) * cexp);
        l_tot = l_tot * w0 + l1 * w1;
        m_run = mm;
#pragma unroll
        for (int db = 0; db < DB; ++db)
#pragma unroll
          for (int r = 0; r < 16; ++r) oacc[db][r] = oacc[db][r] * w0 + mine[2 + db * 16 + r] * w1;
      }
    }

    // The row bookkeeping of the write-out is recomputed from a FRESH lane id (mbcnt: not CSE-able with threadIdx) instead of being
    // kept alive across the tile loop — in the RoPE build, which runs at the 256-register ceiling, those values were its spills
    const int lane_e = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
    const int hi_e = lane_e >> 5, rowE = wq * 32 + (lane_e & 31);
    const bool okE = rowE < NR;
    const size_t growE = ((size_t)ll * a.n_q_heads + h * rep + (okE ? rowE % rep : 0)) * n + (okE ? i0 + rowE / rep : i0);
    if (wk == 0 && okE) {
      const int hi = hi_e;
      const size_t growL = growE;
      const size_t prow = growL * NPART + split;
      // scored steps: the row's (max, sum of exponentials) over this key range in log2 units, for the column-sum pass
      if (a.stats != nullptr && hi == 0) {
        a.stats[prow * 2] = m_run <= kWFloor ? kWFloor : m_run * cexp;
        a.stats[prow * 2 + 1] = l_tot;
      }
      if (a.out_direct != nullptr) {
        if (LOGITS && a.row_stats != nullptr && hi == 0) {      // one-pass scored step: (max in quotient units, sum of exponentials) for the scorer
          float smd = a.sm_div;
          asm volatile("" : "+v"(smd));
          a.row_stats[growL * 2] = m_run <= kWFloor ? EKV_NEG_INF : m_run * (1.f / smd);
          a.row_stats[growL * 2 + 1] = l_tot;
        }
        // unsplit head: the final output row.  Register r of d-block db <-> d = db*32 + (r&3) + 8*(r>>2) + 4*hi
        const float inv = 1.f / l_tot;
        __half* orow = a.out_direct + (size_t)ll * a.n_q_heads * n * D + (size_t)(h * rep + rowE % rep) * a.o_hs + (size_t)(i0 + rowE / rep) * a.o_ts;
#pragma unroll
        for (int db = 0; db < DB; ++db)
#pragma unroll
          for (int q4 = 0; q4 < 4; ++q4) {
            const __half2 lo = ekv_to_e2(oacc[db][4 * q4] * inv, oacc[db][4 * q4 + 1] * inv);
            const __half2 hh = ekv_to_e2(oacc[db][4 * q4 + 2] * inv, oacc[db][4 * q4 + 3] * inv);
            uint2 pk;
            pk.x = __builtin_bit_cast(unsigned int, lo);
            pk.y = __builtin_bit_cast(unsigned int, hh);
            *reinterpret_cast<uint2*>(orow + db * 32 + 8 * q4 + 4 * hi) = pk;
          }
      } else if (EKW_EXP != 9) {      // (EKW_EXP 9: mock without the partial stores)
        // one partial (m, l, o[D]) per key-range split
        float* dst = a.partials + prow * PS;
        if (hi == 0) {
          float smd = a.sm_div;
          asm volatile("" : "+v"(smd));      // (opaque: 1 / sm_div is taken again HERE instead of living in a register across the tile loop)
          dst[0] = m_run <= kWFloor ? EKV_NEG_INF : m_run * (1.f / smd);
          dst[1] = l_tot;
        }
        // (four consecutive d per accumulator quad: ONE 16-byte store instead of four dword stores — 16 instead of 64 store instructions per
        //  lane; the epilogue of a split head is store-ISSUE-bound, cdna_hip_programming.md T21.  Rows are D + 2 floats apart: 8-byte aligned)
        typedef float ekw_f4u __attribute__((ext_vector_type(4), aligned(8)));
#pragma unroll
        for (int db = 0; db < DB; ++db)
#pragma unroll
          for (int q4 = 0; q4 < 4; ++q4)
            *reinterpret_cast<ekw_f4u*>(dst + 2 + db * 32 + 8 * q4 + 4 * hi) = ekw_f4u{oacc[db][4 * q4], oacc[db][4 * q4 + 1], oacc[db][4 * q4 + 2], oacc[db][4 * q4 + 3]};
      }
    }
  }
#if EKW_HAS_TAIL
  // ---- the scorer of this head as the tail of the pass (ekv_wide_tail.h): accumulate, select, compact — when this workgroup alone
  //      wrote the head's column sums (the dispatch sets score_tail only then) ----------------------------------------------------
  if (a.score_tail) {
    __syncthreads();               // this workgroup's own column sums are complete and visible to all of its threads
    ekw_score_tail<kTailItems>(sc, h, ll, smem);
  }
#endif
}

template <int NWQ, int NWK, int KPW, int REP>
hipError_t launch_wide(const EkvAttnArgs& a, int layer_count, hipStream_t s, const EkvScoreArgs* tail) {
  constexpr int D = EKV_D, MODE = EKV_WIDE_MODE, TK = 32 * NWK * KPW, NKB = NWK * KPW;
  size_t lds = 2 * (size_t)TK * 2 * D + (MODE == 0 ? 2 * (size_t)TK * 2 * D : 0) + (EKV_WIDE_ROPE ? (size_t)TK * 2 * D : 0) +
               (MODE == 2 ? (size_t)2 * NKB * NWQ * 64 * 4 + NWQ * 32 * 4 : 0);
  const size_t xch = MODE == 0 ? (size_t)NWQ * 64 * ((D / 32) * 16 + 2) * 4 : 0;     // epilogue exchange reuses the tile buffers
  lds = std::max(lds, xch);
  if (a.score_tail && !EKW_HAS_TAIL) return hipErrorInvalidValue;
#if EKW_HAS_TAIL
  if (a.score_tail) {
    if (tail == nullptr) return hipErrorInvalidValue;
    lds = std::max(lds, ekw_tail_lds_bytes(kNT, tail->n_slots - tail->score_off));      // (the tail's keys + select scratch alias the tile buffers)
  }
#endif
  const EkvScoreArgs sc = (MODE == 2 && tail != nullptr) ? *tail : EkvScoreArgs{};
  const dim3 grid(a.n_kv_heads, MODE == 2 ? a.n_split * a.n_col_parts : a.n_split * a.n_qblocks, layer_count);
  auto* fn = &ekv_attn_wide_kernel<NWQ, NWK, KPW, REP>;
  if (lds > 48 * 1024) (void)hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL(fn, grid, dim3(64 * NWQ * NWK), lds, s, a, sc);
  return hipGetLastError();
}

template <int NWQ, int NWK, int KPW>
hipError_t launch_wide_rep(const EkvAttnArgs& a, int layer_count, hipStream_t s, const EkvScoreArgs* tail) {
  if (EKV_WIDE_MODE == 2) {
    switch (a.n_q_heads / a.n_kv_heads) {
      case 1: return launch_wide<NWQ, NWK, KPW, EKV_WIDE_MODE == 2 ? 1 : 0>(a, layer_count, s, tail);
      case 2: return launch_wide<NWQ, NWK, KPW, EKV_WIDE_MODE == 2 ? 2 : 0>(a, layer_count, s, tail);
      case 4: return launch_wide<NWQ, NWK, KPW, EKV_WIDE_MODE == 2 ? 4 : 0>(a, layer_count, s, tail);
      default: break;
    }
  }
#if EKV_WIDE_ROPE && EKV_WIDE_MODE == 0
  if (a.logits != nullptr) return launch_wide<NWQ, NWK, KPW, -1>(a, layer_count, s, tail);
#else
  if (EKV_WIDE_MODE == 0 && a.logits != nullptr) return hipErrorInvalidValue;      // (only the RoPE builds of the one pass export logits)
#endif
  return launch_wide<NWQ, NWK, KPW, 0>(a, layer_count, s, tail);
}

}  // namespace

// nwq = query waves of 32 rows: 4 (65..128 rows) or 2 (33..64 rows); 256-thread workgroups
#if EKV_WIDE_ROPE
#define EKW_KEYS rope
#else
#define EKW_KEYS plain
#endif
hipError_t EKV_FN_WIDE(EKV_D, EKV_WIDE_MODE, EKW_KEYS, EKV_ELEM)(const EkvAttnArgs& a, int nwq, int layer_count, hipStream_t s, const EkvScoreArgs* tail) {
  switch (nwq) {
#ifndef EKW_M2_KPW
#define EKW_M2_KPW 2
#endif
    case 4: return launch_wide_rep<4, 1, (EKV_WIDE_MODE == 2 ? EKW_M2_KPW : 2)>(a, layer_count, s, tail);
#if EKV_WIDE_MODE == 0 && !EKV_WIDE_ROPE
    // 128-key tiles on 4 x 2 waves (512 threads, 128 KB of LDS: ONE workgroup per CU) for launches that put at most one workgroup on a
    // CU anyway — one layer of a decoder stack per call: 64 KB of K + V in flight per workgroup instead of 32, half as many tile
    // iterations per key range (round 5; the one pass of a one-layer configs[3]-shaped call was 34.5 us for 33 MB)
    case 8: return launch_wide_rep<4, 2, 2>(a, layer_count, s, tail);
    case 9: return launch_wide_rep<2, 4, 1>(a, layer_count, s, tail);      // 33..64 rows: 2 x 4 waves, 128-key tiles
#endif
    case 2: return launch_wide_rep<2, 2, 1>(a, layer_count, s, tail);
    default: return hipErrorInvalidValue;
  }
}
