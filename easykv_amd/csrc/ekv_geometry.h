// Geometry of the kernel families: the limits a family states and its LDS plan, in ONE place.  Plain C++17: the kernels and their
// launchers include it for the layout they run on, the step planner (ekv_plan.cpp, host-only) for the byte counts and bounds it decides
// on.  No intrinsics and no HIP type: includable from a translation unit that never sees hipcc.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/easykv_hip.h"

#if defined(__HIP__)
#define EKV_HD __host__ __device__
#else
#define EKV_HD
#endif

static inline EKV_HD size_t ekv_align(size_t x, size_t a) { return (x + a - 1) / a * a; }

// ---- decode stream and the one-launch decode kernel (ekv_decode_stream.h, ekv_attn_decode.inc) -------------------------------------
constexpr int kU = 8;   // rows in flight per lane group (K and V each)

// head_dim 96 (any head_dim that is a multiple of 16 but not a power of two): a row keeps a power-of-two lane group (LPR = 16) of
// which only the first LIVE = D / 8 lanes hold a 16-byte piece; the idle lanes carry zeros through the dot products and reductions.
// EPL = elements per 16-byte piece: 8 (16-bit rows) or 16 (FP8 rows, "kv8": a head_dim-128 row is 8 lanes, head_dim 64 is 4).
// head_dim 256 (16-bit rows): a row is 32 pieces, so the lane group is half a wave (LPR = 32) and a wave-load covers two rows.  Every
// lane still holds ONE piece of a row and 8 output floats per query head — the per-lane state is head_dim 128's — and the sums and
// maxima over a lane group take one step across the DPP row boundary (ekv_group_sum / ekv_group_max, ekv_common.h).
template <int D, int NW = 4, int KU = kU, int EPL = 8>
struct EkvDecodeGeom {
  static constexpr int LIVE = D / EPL;  // lanes of a row's lane group that hold a 16-byte piece
  static constexpr int LPR = LIVE <= 4 ? 4 : (LIVE <= 8 ? 8 : (LIVE <= 16 ? 16 : 32));   // lanes per row (power of two)
  static constexpr int G = 64 / LPR;  // rows per wave-load
  static constexpr int RW = G * KU;   // rows per wave per iteration
  static constexpr int NP = NW;       // partials per workgroup = waves (lane groups are combined in-wave)
  static constexpr int PS = D + 2;    // (m, l, o[D])
  // what the stream handles: one piece per lane, whole rows inside a wave, group reductions of at most half a wave
  static_assert(D % EPL == 0 && LIVE >= 1, "a row is a whole number of 16-byte pieces");
  static_assert(LIVE <= LPR, "a lane holds one piece of a row: a wider row needs a wider lane group, or the stream drops its end");
  static_assert(LPR <= 32 && G * LPR == 64, "a lane group is at most half a wave (ekv_group_sum / ekv_group_max stop at 32 lanes)");
};

// LDS bytes of the one-launch decode kernel (ekv_decode_fused_kernel, ekv_attn_decode.inc): host arithmetic over the geometry, the same
// for every element type, row format and batching.  n_state = score rows kept in LDS (3 with roco on the ordered layout).
template <int D, int REP, int NW = 8>
inline size_t ekv_fused_lds(int t_pad, int l_pad, int n_state) {
  using Gm = EkvDecodeGeom<D, NW>;
  const size_t part = ekv_align((size_t)Gm::NP * REP * Gm::PS, 4);
  return ((size_t)REP * l_pad + part + (size_t)n_state * ekv_align((size_t)t_pad, 256)) * 4 + 2 * NW * 8 * 8 +
         ekv_align(ekv_align((size_t)l_pad, 128) / 8, 16) + 264 * 4;   // + one dead-row bit per physical row + select histogram
}
// ... of the widest build a step of GQA factor `rep` on nw-wave workgroups can need (the planner: ekv_decode_fused_supported)
template <int D>
inline size_t ekv_fused_lds_max(int rep, int t_pad, int l_pad, int nw) {
  switch (rep) {
    case 1: return nw == 8 ? ekv_fused_lds<D, 1, 8>(t_pad, l_pad, 3) : ekv_fused_lds<D, 1, 4>(t_pad, l_pad, 3);
    case 2: return nw == 8 ? ekv_fused_lds<D, 2, 8>(t_pad, l_pad, 3) : ekv_fused_lds<D, 2, 4>(t_pad, l_pad, 3);
    case 3: case 4: return nw == 8 ? ekv_fused_lds<D, 4, 8>(t_pad, l_pad, 3) : ekv_fused_lds<D, 4, 4>(t_pad, l_pad, 3);
    default: return nw == 8 ? ekv_fused_lds<D, 8, 8>(t_pad, l_pad, 3) : ekv_fused_lds<D, 8, 4>(t_pad, l_pad, 3);
  }
}

// ---- split-path decode scorer (ekv_decode_score.inc) ---------------------------------------------------------------------------------
#ifndef EKV_SCORE_NW
#define EKV_SCORE_NW 8
#endif
constexpr int kSNW = EKV_SCORE_NW, kSNT = 64 * kSNW;   // waves / threads per scorer workgroup

// logits of the rep query heads | score rows | reduction scratch | histogram | candidate list
inline size_t ekv_decode_score_lds(int rep, int t_pad, int policy) {
  const size_t n_state = policy == EKV_POLICY_ROCO ? 3 : 1;
  return ((size_t)rep * t_pad + n_state * ekv_align((size_t)t_pad, 256)) * 4 + 2 * kSNW * 8 * 8 + 264 * 4 + kSNT * 8;
}

// ---- generic scorer (ekv_score_select.inc), nt threads per workgroup -------------------------------------------------------------------
// W score columns, `rows` logits rows swept per head (0 when column sums replace the logits); big: S / Q / C live in global scratch and
// only the selection keys in LDS.  Keys (+ rows) | reduction scratch | histogram | candidate list.
inline size_t ekv_score_lds_bytes(int nt, int64_t W, int64_t rows, bool big) {
  return ekv_align(((size_t)(big ? 1 : 4) * (size_t)W + 2 * (size_t)rows) * 4, 16) + 2 * (nt / 64) * 8 * 4 + 264 * 4 + nt * 8;
}
// ... of a launch's arguments (EkvScoreArgs, ekv_kernels.h; a template only so that this header needs no HIP type)
template <typename ScoreArgs>
inline size_t ekv_score_lds_bytes(int nt, const ScoreArgs& a) {
  const bool scored = a.policy == EKV_POLICY_H2O_HEAD || a.policy == EKV_POLICY_ROCO || a.policy == EKV_POLICY_TOVA;
  const int64_t W = (int64_t)a.n_slots - (scored ? a.score_off : 0);
  const int64_t rows = a.colsum != nullptr ? 0 : (int64_t)(a.n_q_heads / a.n_kv_heads) * a.q_len;   // (lrows of the kernel body)
  return ekv_score_lds_bytes(nt, W, rows, a.big_rows != nullptr);
}
// generic scorer: S / Q / C + keys of W columns do not fit 160 KB of LDS (decided at workspace-planning time, before the arguments
// exist: the 512-thread build with all four arrays in LDS)
inline bool ekv_score_rows_exceed_lds(int W, int rows) { return ekv_score_lds_bytes(512, W, rows, false) > 160 * 1024; }
// Threads per workgroup the generic scorer's dispatch picks for a launch of `pairs` (head, layer) pairs (ekv_score_select_dispatch.hip;
// its reasons are there).  The 512-thread build folds key-range partials in batches of 16, the other two in batches of 8 (a 1024-thread
// launch bound leaves 64 VGPRs): the long-row scorer folds in the batches of the build the plain call would have run, so that the
// row statistics and the folded output keep their bits.
inline int ekv_score_select_threads(int64_t pairs, int64_t W, int64_t rows, bool big) {
  if (big) return 1024;
  if (pairs >= 768 && ekv_score_lds_bytes(256, W, rows, false) <= 53 * 1024) return 256;
  const bool one_per_cu = pairs <= 256 || ekv_score_lds_bytes(512, W, rows, false) > 80 * 1024;
  if (one_per_cu && ekv_score_lds_bytes(1024, W, rows, false) <= 160 * 1024) return 1024;
  return 512;
}

// ---- pooled generic scorer (ekv_score_select.inc, EKV_POOL build; the ekv_pool_* calls), 512 or 1024 threads ----------------------------
// LDS plan: the unpooled scorer's, byte for byte (ekv_score_lds_bytes above).  The pooling stencil runs between accumulation and key
// formation: it READS the score row S where it already sits (LDS; global scratch when `big`) and WRITES the selection keys, which have a
// row of their own in LDS in either layout — the second row an out-of-place stencil needs is that key row, so nothing is added and no
// halo is kept per thread.  Access pattern: thread t owns columns t, t + nt, ...; at tap d the lanes of a wave read 64 consecutive
// words S[base + lane + d]: one LDS bank per lane, conflict-free, 2r + 1 reads per column.  Widest pooled row = the widest unpooled row:
// ~10 000 columns with S in LDS, ~38 400 with S in scratch; beyond that the planner refuses the step (EKV_E_UNSUPPORTED, no launch).
inline size_t ekv_score_pool_lds_bytes(int nt, int64_t W, int64_t rows, bool big) { return ekv_score_lds_bytes(nt, W, rows, big); }
// the dispatch's block size (ekv_score_select_dispatch.hip): there is no 256-thread pooled build
inline int ekv_score_pool_threads(int64_t pairs, int64_t W, int64_t rows, bool big) {
  return ekv_score_select_threads(pairs, W, rows, big) == 1024 ? 1024 : 512;
}

// ---- long-row scorer (ekv_score_long.inc): sweep over column tiles, then one select workgroup per head -------------------------------
constexpr int kLongSweepNT = 256;      // threads of a sweep workgroup, four consecutive columns each
constexpr int kLongTile = 4 * kLongSweepNT;      // columns per sweep workgroup
constexpr int kLongSelectNT = 1024;    // threads of the select workgroup
inline int64_t ekv_long_tiles(int64_t W) { return W <= 0 ? 0 : (W + kLongTile - 1) / kLongTile; }
// sweep: (M, 1 / L) of the `rows` logits rows (0 when column sums replace the logits) — its only LDS, whatever the width
inline size_t ekv_long_sweep_lds(int64_t rows) { return (size_t)2 * (size_t)rows * 4; }
// select: reduction scratch | histogram | candidate list (the keys are in global scratch)
constexpr size_t ekv_long_select_lds() { return 2 * (kLongSelectNT / 64) * 8 * 4 + 264 * 4 + kLongSelectNT * 8; }

// ---- scorer as the tail of the wide column-sum pass and of the logits-resident kernel (ekv_wide_tail.h), nt threads ------------------
inline size_t ekw_tail_lds_bytes(int nt, int W) {      // keys | reduction scratch | histogram | candidate list
  return ekv_align((size_t)W * 4, 16) + 2 * (nt / 64) * 8 * 4 + 264 * 4 + nt * 8;
}

// ---- small-row chunk step with the logits in LDS (ekv_chunk_lds.inc) --------------------------------------------------------------------
constexpr int kLNW = 4;                     // waves per workgroup
constexpr int kLItems = 10;                 // owned columns per thread: score rows up to 10 * 256 = 2560 positions
constexpr int kListCap = 256;               // candidate list of the select (entries)

struct LdsPlan {
  size_t e_bytes, key_off, stat_off, red_off, hist_off, dead_off, total;
};
// LDS: logits / probabilities [E16 + 16 keys][NQ] fp32 (the last 16 "keys" are the chunk's own) | keys of the fallback select |
// row statistics + their reduction scratch | block-reduction scratch | select histogram + candidate list | dead-row bits
template <int D, int NQ>
EKV_HD inline LdsPlan ekv_lds_plan(int e16, int W) {
  LdsPlan p;
  const size_t logits = (size_t)(e16 + 16) * NQ * 4;
  const size_t oscr = (size_t)kLNW * NQ * D * 4;   // cross-wave output reduction, aliases the (dead) logits at the very end
  p.e_bytes = ekv_align(logits > oscr ? logits : oscr, 16);
  p.key_off = p.e_bytes;
  const size_t stage = (size_t)kLNW * (D >= 128 ? 8 : 64 / (D / 8)) * D * 2;   // phase A's per-wave staging tiles (8 or G rows) alias the fallback select's key array
  p.stat_off = p.key_off + ekv_align((size_t)W * 4 > stage ? (size_t)W * 4 : stage, 16);
  p.red_off = p.stat_off + (2 * 16 + 2 * kLNW * 8) * 4;
  p.hist_off = p.red_off + 2 * kLNW * 8 * 2;
  p.dead_off = p.hist_off + 264 * 4 + kListCap * 8;
  p.total = p.dead_off + ekv_align((size_t)(e16 / 32 + 2) * 4, 16);
  return p;
}
// LDS bytes of a step of `rows` GQA-folded query rows (the 4-row or the 8-row build)
template <int D>
inline size_t ekv_chunk_lds_bytes(int rows, int phys_extent, int n_slots) {
  const int e16 = (phys_extent + 15) & ~15;
  return rows <= 4 ? ekv_lds_plan<D, 4>(e16, n_slots).total : ekv_lds_plan<D, 8>(e16, n_slots).total;
}

// ---- logits-resident scored chunk step (ekv_attn_resident.inc) --------------------------------------------------------------------------
constexpr int R_D = 128, R_NT = 512, R_TK = 128, R_NB = 3, R_MAXT = 10;      // R_MAXT: 32 x 32 logit blocks a wave keeps (160 registers)
constexpr int R_RS = 2 * R_D;                         // bytes per K / V row in LDS (unpadded, XOR-swizzled 16-byte chunks)
constexpr int R_TBUF = R_TK * R_RS;                   // 32 KB per ring slot
// Two shapes of the same kernel (the 320 KB of accumulator registers hold either):
//   LONG = false  up to 64 rows x 1280 keys: query-wave group wq owns rows wq*32 .. +32 of EVERY tile
//   LONG = true   up to 32 rows x 2560 keys: both groups hold rows 0 .. 31, group wq owns the tiles t with (t & 1) == wq; the V pass
//                 splits a tile's keys over the two groups and their O^T blocks are added once at the end
template <bool LONG>
struct RL {
  static constexpr int TILES = LONG ? 2 * R_MAXT : R_MAXT, TMAX = TILES * R_TK;
  static constexpr int PSTR = LONG ? 80 : 144;        // bytes per key row of a P^T tile: 32 / 64 queries x fp16 + 16 (an odd multiple of 16: conflict-free writes and transposing reads)
  static constexpr int PBUF = R_TK * PSTR;
  static constexpr int OFF_P = R_NB * R_TBUF;         // P^T tiles [2][128][PSTR]; LONG = false, behind the V pass: the query waves' column-sum exchange
  static constexpr int OFF_SLOT = OFF_P + 2 * PBUF;   // slot-map entries of the head's cache rows [TMAX]
  static constexpr int OFF_CS = OFF_SLOT + TMAX * 4;  // column sums [2][TMAX]
  static constexpr int OFF_RED = OFF_CS + 2 * TMAX * 4;   // row maxima [rows][NSH], row sums [rows][NSH] (256 words each), 1 / L [64]
  static constexpr int LDS = OFF_RED + (256 + 256 + 64) * 4;
  static constexpr int NSH = LONG ? 8 : 4;            // shares of a row's statistics: the waves that hold keys of the row
  static constexpr int TI = (TMAX + R_NT - 1) / R_NT; // score columns per thread of the scorer
  static_assert(LDS <= 160 * 1024, "one workgroup per CU");
  static_assert(2 * TMAX * 4 <= 2 * PBUF || LONG, "the column-sum exchange fits the P^T tile buffers");
};

// ---- query blocks of the chunk attention kernels (ekv_attn_chunk.inc, ekv_attn_wide.inc) ------------------------------------------------
// A query block is <= 128 GQA-folded rows (rep x qb_rows).  qpw = 1 or 2: 16-row query tiles per wave of a 4-wave
// workgroup (<= 32 / <= 64 rows); qpw = 4 selects the 8-wave workgroup (2 tiles per wave x 4 query-tile waves, <= 128 rows).
// head_dim 256 (kChunkNarrowD): blocks of <= 32 folded rows, ONE query tile per wave of the 4-wave workgroup (qpw = 1) — the only build
// of the 16x16x32 kernel whose 16 output blocks per tile, staged K/V pieces and query operands fit 256 VGPRs without scratch; the
// two-tile builds are not instantiated at that head_dim (ekv_attn_chunk.inc), so GQA factors above 32 are refused (ekv_plan.cpp).
constexpr int kChunkNarrowD = 256;
constexpr int kChunkNarrowRows = 32;
inline void ekv_chunk_blocks(int rep, int q_len, int* qb_rows, int* n_qblocks, int* qpw, int head_dim = 0) {
  if (head_dim >= kChunkNarrowD) {
    const int rows = (int64_t)rep * q_len > kChunkNarrowRows ? (kChunkNarrowRows / rep > 0 ? kChunkNarrowRows / rep : 1) : q_len;
    *qb_rows = rows;
    *n_qblocks = (int)(((int64_t)q_len + rows - 1) / rows);
    *qpw = 1;
    return;
  }
  int rows = q_len;
  if ((int64_t)rep * q_len > 128) rows = 128 / rep > 0 ? 128 / rep : 1;   // (64-row blocks on 4-wave workgroups: 324 vs 378 TFLOP/s on the dense prefix)
  // (65..128 rows stay ONE block on the 8-wave workgroup: two 4-wave blocks of <= 64 rows, even XCD-local so that the second K/V
  // read is an L2 hit, measured 1.55 vs 1.19 ms per C4 step)
  *qb_rows = rows;
  *n_qblocks = (int)(((int64_t)q_len + rows - 1) / rows);
  const int64_t r = (int64_t)rep * rows;
  *qpw = r <= 32 ? 1 : (r <= 64 ? 2 : 4);
}
// partial column-sum rows the exact pass writes per (head, query block) = its query-tile waves
inline int ekv_chunk_col_parts(int qpw, bool rope) { (void)rope; return qpw == 4 ? 4 : 2; }

// ---- LDS of the 16x16x32 chunk kernel (ekv_attn_chunk.inc): its launcher sizes the launch with it, the planner holds it to one CU ------
constexpr int kChunkKT = 64;     // positions per K/V super-tile
constexpr int kChunkPadH = 16;   // LDS row padding in halfs
// mode 0 / 1 / 2 = one pass / statistics pass / exact pass; tiles = 16-row query tiles per wave (1 or 2), nw = waves per workgroup
// (4, 8 or 16).  Slot entries of the key range | K tile (+ V tile, + the low plane of rotated keys) | the query block where it lives in
// LDS; the 16-wave build's in-kernel fold of the two key halves exchanges (m, l, o[D]) of nw / 2 x 64 lanes over the tile buffers.
constexpr bool ekv_chunk_q_in_lds(int mode, int tiles, bool rope, int nw) {
  return mode == 1 ? (rope && tiles >= 2) : (nw == 8 || (tiles >= 2 && rope));
}
inline size_t ekv_chunk_kernel_lds(int head_dim, int mode, int tiles, bool rope, int nw, int rows_per_split, bool fold) {
  const size_t row = (size_t)(head_dim + kChunkPadH) * 2, slots = ekv_align((size_t)rows_per_split * 4, 16);
  size_t lds = slots + (size_t)((rope ? 3 : 2) - (mode == 1 ? 1 : 0)) * kChunkKT * row +
               (ekv_chunk_q_in_lds(mode, tiles, rope, nw) ? (size_t)(rope ? 2 : 1) * 16 * tiles * (nw / 2) * row : 0);
  const size_t xch = slots + (size_t)(nw / 2) * 64 * ((size_t)(head_dim / 16) * 4 + 2) * 4;
  if (nw == 16 && fold && xch > lds) lds = xch;
  return lds;
}
// ... of the largest launch a step on this kernel makes: qpw as ekv_chunk_blocks answers it (4: the 8-wave workgroup with two tiles
// per wave, or the 16-wave one-pass build without RoPE-on-read)
inline size_t ekv_chunk_step_lds(int head_dim, int qpw, bool rope, bool two_pass, int rows_per_split, bool fold) {
  const int tiles = qpw == 4 ? 2 : qpw, nw = qpw == 4 ? 8 : 4;
  if (two_pass) {
    const size_t a = ekv_chunk_kernel_lds(head_dim, 1, tiles, rope, nw, rows_per_split, false);
    const size_t b = ekv_chunk_kernel_lds(head_dim, 2, tiles, rope, nw, rows_per_split, fold);
    return a > b ? a : b;
  }
  if (qpw == 4 && !rope) return ekv_chunk_kernel_lds(head_dim, 0, 1, false, 16, rows_per_split, fold);
  return ekv_chunk_kernel_lds(head_dim, 0, tiles, rope, nw, rows_per_split, fold);
}
