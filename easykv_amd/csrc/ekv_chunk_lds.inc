// K2s: strided-prefill chunk step with few query rows (rep * stride <= 8) — the WHOLE step of one (KV head, layer) in one
// workgroup with the head's probabilities kept in LDS: HBM traffic = K once + V once + score rows in/out (the algorithmic
// bytes of SURVEY.md §8d), no logits round trip, no staging of K/V through LDS.  BASELINE.json configs[1] (Llama2-7B,
// stride 8, budget 0.5: 8 rows x 2064 slots = 66 KB of fp32 logits per head) is the shape it is built for.
// Compiled once per EKV_D by ekv_chunk_lds_d*.hip.
//
// Replaces, per (layer, head) and chunk forward (same reference sites as ekv_attn_chunk.inc + ekv_score_select.inc):
//   attention of the chunk          easykv/llama_patch.py:198-222 (mistral_patch.py:144-169), append :193-196
//   GQA fold, accumulate            easykv/easykv.py:188-196, :443-457 (auto :604-618, ppl :834-848)
//   count advance, select           easykv/easykv.py:460-499
//   K/V + score-row compaction      easykv/easykv.py:56-82, :465-490   (slot-map compaction, rows never move)
//
// One workgroup = 4 waves, two workgroups per CU (LDS <= 80 KB each), 2 waves per SIMD with up to 256 registers each:
//   A  logits of every PHYSICAL row [0, E) of the head (address order, dead rows masked by one bit per row, as in the fused
//      decode kernel).  K rows are read fully coalesced (16 lanes x 16 B per row, non-temporal, 12 loads per lane in flight, no
//      barrier in the loop), transposed into the MFMA fragment layout through a wave-private 8-row staging tile in LDS, and
//      S = Q . K^T is one mfma_f32_16x16x32_f16 chain per tile with A = Q, B = K, so that a lane ends up with four consecutive
//      query rows of ONE key: raw logits -> LDS [physical row][query row], one conflict-free ds_write_b128 per lane and tile.
//      Software-pipelined: the staging + fragment reads of tile u + 1 are issued before the MFMA chain of tile u.  The row maxima
//      are taken on the way.  The chunk's own keys come from k_new (causal inside the chunk).
//   M  e = exp2((x - max) * log2 e) in place, L = sum e (all threads, float4 pieces, one block reduction).
//   S  the scorer, by thread-owned columns held in registers: pbar = mean over the rep heads of e / L, column sums
//      S += sum_i pbar, Q += sum_i pbar^2 (same order of operations as ekv_score_select.inc); roco's feasible set by an exact
//      threshold select over sampled pivots (lds_kth_threshold), the k victims by k wave-wide arg-min rounds + a ranking of the 4k
//      candidates; compaction of the score rows and of the slot map straight from registers.
//   B  O = sum_j e_j v_j over the same physical rows: V rows read fully coalesced (8 loads per lane in flight); D = 128: the 8
//      rows of a lane group become MFMA B operands by an 8 x 8 half transpose inside the lane, P in fp16 from the LDS array;
//      O / L -> fp16 (cross-wave sum through the key array, the logits stay intact).
// S and B are independent (B needs e and L only).  The two workgroups of a CU take them in OPPOSITE order (parity of the
// hardware wave slot, flipped every dispatch round): A M S B and A B M S — the B-first one takes exp inside phase B and only its
// output stage waits for M — so that one's statistics + scorer (latency chains in LDS, no HBM traffic) run under the other's V stream.  Measured history (C2, us per 32-layer step; docs/TUNING.md §3.6, §8): fragment-layout K loads straight from
// global memory 282 (K at 4.2 TB/s: 64-byte segments); v_dot2 + DPP reduce-scatter on row-coalesced registers 298; 8-wave
// workgroups at 128 registers 332; 6 waves 335; round 2's version (all phases in the same order in both workgroups, PV on
// v_pk_fma_f32, one tile at a time in phase A, library expf, block-wide victim rounds) 260; this version 222-228.
#include "ekv_common.h"
#include "ekv_kernels.h"
#if EKV_BF16   // (bf16 instances: the same kernel under a tagged name)
#define ekv_chunk_lds_kernel ekv_chunk_lds_kernel_bf16
#endif

#ifndef EKV_LDS_ORDER
#define EKV_LDS_ORDER 2   // 0: scorer then phase B, 1: phase B then scorer, 2: by the parity of the workgroup's wave slot
#endif
#define EKV_SS_NT 256
#define EKV_SS_DEVICE_ONLY
#include "ekv_score_select.inc"

namespace {

typedef float ekv_f4 __attribute__((ext_vector_type(4)));
struct EkvTrue { static constexpr bool value = true; };
struct EkvFalse { static constexpr bool value = false; };
#ifdef EKV_LDS_NO_PEEL
typedef EkvTrue EkvLastRefill;
#else
typedef EkvFalse EkvLastRefill;
#endif
typedef float ekv_f2 __attribute__((ext_vector_type(2)));

// 4 waves per workgroup, two workgroups per CU = 2 waves per SIMD with up to 256 registers each: 12 K loads (phase A) / 8 V
// loads + 32 accumulators (phase B) per lane in flight (a scratch reload inside a stream loop waits for every
// load issued before it: vmcnt retires in order).  8-wave workgroups at 128 registers were tried: they need the query rows split
// between wave groups in phase B (V fetched twice) and were slower in BOTH stream phases.
constexpr int kLNT = 64 * kLNW;            // threads per workgroup (kLNW, kLItems, kListCap and the LDS plan ekv_lds_plan: ekv_geometry.h)
constexpr unsigned kLdsResident = 512;      // workgroups resident at a time on an MI355X: 256 CUs x 2 (LDS)

// Exclusive threshold `thr` on UNIQUE 64-bit composites ((order-preserving key) << 32 | position) such that exactly k of the
// workgroup's composites lie below it — "the k smallest keys, ties to the lower position" — or 0 when the fast path does not
// apply (the caller then falls back to the generic LDS select).  cv[it] = composite of the thread's it-th column (position
// tid + it * 256; ~0 for columns >= W).
// A histogram over bins of equal key WIDTH piles most keys into a few bins as soon as one outlier stretches the range (hundreds of
// same-address LDS atomics, then an overflowing candidate list).  Here the bins are cut at 64 SAMPLED composites (every W/64-th
// position, ordered by one wave with 64 readlane compares): about W/64 members per bin whatever the distribution, ties included
// (composites are unique).  Five barriers: sample, pivots, histogram, bin of rank k - 1, its members ranked against each other —
// LDS-only ones (ekv_lds_barrier): __syncthreads would also drain the caller's global stores still in flight at every step.
__device__ unsigned long long lds_kth_threshold(Blk& b, const unsigned long long (&cv)[kLItems], int W, int k, uint32_t* hist,
                                                unsigned long long* list, int list_cap) {
  unsigned long long* piv = reinterpret_cast<unsigned long long*>(hist + 128);   // 64 pivots in the upper half of the 264 words
  const int step = W / 64;
  if (step < 2 || k < 1 || k > W) return 0;
  for (int i = b.tid; i < 128; i += kLNT) hist[i] = 0;          // [0..64] bins, [66] listed, [67] bin, [68] below, [70..71] result
#pragma unroll
  for (int it = 0; it < kLItems; ++it) {
    const int j = b.tid + it * kLNT;
    if (j < W && j % step == 0 && j / step < 64) piv[j / step] = cv[it];
  }
  ekv_lds_barrier();
  if (b.wave == 0) {               // order the 64 samples: rank by counting (unique values), lane -> piv[rank]
    const unsigned long long mine = piv[b.lane];
    int rank = 0;
    for (int x = 0; x < 64; ++x) {
      const unsigned long long other = ((unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)(mine >> 32), x) << 32) |
                                       (uint32_t)__builtin_amdgcn_readlane((int)(mine & 0xFFFFFFFFu), x);
      rank += other < mine ? 1 : 0;
    }
    piv[rank] = mine;              // (every lane has read its sample before any lane writes: readlane is wave-synchronous)
  }
  ekv_lds_barrier();
  int bin[kLItems];      // bin = number of pivots <= composite, 0 .. 64: branch-free binary searches, the columns' searches side by
#pragma unroll           // side (step-major), so that a step is kLItems independent LDS reads and not a chain of dependent round trips
  for (int it = 0; it < kLItems; ++it) bin[it] = 0;
#pragma unroll
  for (int sft = 32; sft >= 1; sft >>= 1) {
    unsigned long long pv[kLItems];
#pragma unroll
    for (int it = 0; it < kLItems; ++it) pv[it] = piv[bin[it] + sft - 1];
#pragma unroll
    for (int it = 0; it < kLItems; ++it) bin[it] += pv[it] <= cv[it] ? sft : 0;
  }
  {
    unsigned long long pv[kLItems];
#pragma unroll
    for (int it = 0; it < kLItems; ++it) pv[it] = piv[bin[it]];
#pragma unroll
    for (int it = 0; it < kLItems; ++it) {
      bin[it] += pv[it] <= cv[it] ? 1 : 0;
      if (b.tid + it * kLNT < W) atomicAdd(&hist[bin[it]], 1u);
    }
  }
  ekv_lds_barrier();
  if (b.wave == 0) {               // lane l owns bin l (lane 63 also bin 64); inclusive scan
    const uint32_t mine = hist[b.lane];
    uint32_t incl = mine;
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t up = (uint32_t)__shfl_up((int)incl, o, 64);
      if (b.lane >= o) incl += up;
    }
    const uint32_t excl = incl - mine, kk = (uint32_t)k;
    if (excl < kk && kk <= incl) {
      hist[67] = b.lane;
      hist[68] = excl;
    }
    if (b.lane == 63 && kk > incl) {
      hist[67] = 64;
      hist[68] = incl;
    }
  }
  ekv_lds_barrier();
  const int b_sel = (int)hist[67];
  const uint32_t below = hist[68], in_bin = hist[b_sel];
  if ((int)in_bin > list_cap || (int)in_bin > kLNT) {
    ekv_lds_barrier();
    return 0;
  }
#pragma unroll
  for (int it = 0; it < kLItems; ++it)
    if (bin[it] == b_sel && b.tid + it * kLNT < W) list[atomicAdd(&hist[66], 1u)] = cv[it];
  ekv_lds_barrier();
  if (b.tid < (int)in_bin) {
    const unsigned long long e = list[b.tid];
    uint32_t rank = 0;
    const int nb = (int)in_bin;
    for (int i = 0; i < nb; i += 4) {          // four broadcast reads per trip (clamped; the guards keep a duplicate from counting)
      const unsigned long long l0 = list[i], l1 = list[min(i + 1, nb - 1)], l2 = list[min(i + 2, nb - 1)], l3 = list[min(i + 3, nb - 1)];
      rank += (l0 < e ? 1u : 0u) + ((i + 1 < nb && l1 < e) ? 1u : 0u) + ((i + 2 < nb && l2 < e) ? 1u : 0u) + ((i + 3 < nb && l3 < e) ? 1u : 0u);
    }
    if (below + rank == (uint32_t)k - 1u) *reinterpret_cast<unsigned long long*>(hist + 70) = e + 1ull;
  }
  ekv_lds_barrier();
  // (no barrier after this read: the caller's next LDS writes — candidate and victim lists at hist[100..115], hist[128..255] — do not
  //  touch hist[70..71], and its next barrier comes before anything else reuses the histogram)
  return *reinterpret_cast<const unsigned long long*>(hist + 70);
}

// Warm start of the threshold select: `hint` = the key of the k-th smallest composite of the head's PREVIOUS chunk step (kept in
// ekv_bank.slot_state[head][3] when the bank has that array).  A chunk step adds `stride` probabilities to every column, the
// threshold moves by a percent or so: count the composites below a window of +- 2^18 ulps (+- 3 %) around the hint and list the window's
// members in the same pass; one LDS barrier later the exact threshold is known (two more for its ranking) — against the sample /
// pivot / histogram / bin / list sequence of lds_kth_threshold.  Returns 0 when the window misses (the caller then runs the full
// select).  hist[66] and hist[70..71] must be zero on entry (the statistics pass clears them).
__device__ unsigned long long lds_warm_threshold(Blk& b, const unsigned long long (&cv)[kLItems], int W, int k, uint32_t hint, uint32_t* hist,
                                                 unsigned long long* list, int list_cap) {
#ifndef EKV_LDS_WARM_WIN
#define EKV_LDS_WARM_WIN 18   // measured on configs[1] (us per step, 4 interleaved rounds): no hint 211, 2^14 204, 2^16 204, 2^18 204.4 vs 210.9 (-3 %), 2^20 207, 2^22 212 (the list overflows)
#endif
  constexpr uint32_t kWin = 1u << EKV_LDS_WARM_WIN;
  const uint32_t kSent = ekv_fkey(1e9f);
  const uint32_t lo = hint > kWin ? hint - kWin : 0u, hi = hint < kSent - kWin ? hint + kWin : kSent - 1u;
  int below = 0;
#pragma unroll
  for (int it = 0; it < kLItems; ++it) {
    const uint32_t key = (uint32_t)(cv[it] >> 32);
    const bool in = b.tid + it * kLNT < W;
    below += __popcll(__ballot(in && key < lo));
    if (in && key >= lo && key <= hi) {
      const uint32_t at = atomicAdd(&hist[66], 1u);
      if ((int)at < list_cap) list[at] = cv[it];
    }
  }
  if (b.lane == 0) hist[72 + b.wave] = (uint32_t)below;
  ekv_lds_barrier();
  int n_below = 0;
#pragma unroll
  for (int w = 0; w < kLNW; ++w) n_below += (int)hist[72 + w];
  const int in_win = (int)hist[66];
  if (!(n_below < k && k <= n_below + in_win && in_win <= list_cap && in_win <= kLNT)) {
    ekv_lds_barrier();      // (everybody has read the counters: lds_kth_threshold clears them next)
    return 0;
  }
  if (b.tid < in_win) {
    const unsigned long long e = list[b.tid];
    int rank = 0;
    for (int i = 0; i < in_win; ++i) rank += list[i] < e ? 1 : 0;
    if (n_below + rank == k - 1) *reinterpret_cast<unsigned long long*>(hist + 70) = e + 1ull;
  }
  ekv_lds_barrier();
  return *reinterpret_cast<const unsigned long long*>(hist + 70);
}

// Block-wide minimum of a 64-bit value: DPP butterflies inside a row of 16 lanes, three shuffles across the rows, then LDS.
// (ekv_wave_min_u64's twelve ds_bpermute round trips were ~1.5 k cycles per call; the victims are found by one such reduction
// per victim.)
template <int CTRL>
__device__ __forceinline__ unsigned long long lds_dpp_u64(unsigned long long x) {
  const int lo = __builtin_amdgcn_update_dpp(0, (int)(x & 0xFFFFFFFFu), CTRL, 0xf, 0xf, true);
  const int hi = __builtin_amdgcn_update_dpp(0, (int)(x >> 32), CTRL, 0xf, 0xf, true);
  return ((unsigned long long)(uint32_t)hi << 32) | (uint32_t)lo;
}
__device__ __forceinline__ unsigned long long lds_blk_min_u64(Blk& b, unsigned long long x) {
  unsigned long long y;
  y = lds_dpp_u64<0xB1>(x); x = y < x ? y : x;     // quad_perm [1,0,3,2]
  y = lds_dpp_u64<0x4E>(x); x = y < x ? y : x;     // quad_perm [2,3,0,1]
  y = lds_dpp_u64<0x141>(x); x = y < x ? y : x;    // row_half_mirror
  y = lds_dpp_u64<0x140>(x); x = y < x ? y : x;    // row_mirror
  y = __shfl_xor(x, 16, 64); x = y < x ? y : x;
  y = __shfl_xor(x, 32, 64); x = y < x ? y : x;
  unsigned long long* r = b.red + (b.phase & 1) * kLNW;
  if (b.lane == 0) r[b.wave] = x;
  ekv_lds_barrier();
  unsigned long long m = r[0];
#pragma unroll
  for (int i = 1; i < kLNW; ++i) m = r[i] < m ? r[i] : m;
  b.phase++;
  return m;
}

// Wave-wide minimum of a 64-bit value, no LDS: DPP butterflies inside the rows of 16 lanes, then the four row results by readlane.
__device__ __forceinline__ unsigned long long lds_wave_min_u64(unsigned long long x) {
  unsigned long long y;
  y = lds_dpp_u64<0xB1>(x); x = y < x ? y : x;     // quad_perm [1,0,3,2]
  y = lds_dpp_u64<0x4E>(x); x = y < x ? y : x;     // quad_perm [2,3,0,1]
  y = lds_dpp_u64<0x141>(x); x = y < x ? y : x;    // row_half_mirror
  y = lds_dpp_u64<0x140>(x); x = y < x ? y : x;    // row_mirror
  unsigned long long m = ~0ull;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const unsigned long long v = ((unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)(x >> 32), 16 * r) << 32) |
                                 (uint32_t)__builtin_amdgcn_readlane((int)(x & 0xFFFFFFFFu), 16 * r);
    m = v < m ? v : m;
  }
  return m;
}

template <int D, int NQ>
__global__ void __launch_bounds__(kLNT, 2) ekv_chunk_lds_kernel(const EkvAttnArgs a, const EkvScoreArgs sc) {
  constexpr int LPR = D / 8;          // lanes per row (phase B)
  constexpr int G = 64 / LPR;         // rows per wave-load (phase B)
  constexpr int QP = NQ / 4;          // float4 pieces per key in the logits array
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int h = blockIdx.y, ll = blockIdx.z, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int T = a.n_slots, n = a.q_len, rep = a.n_q_heads / a.n_kv_heads;
  const int rows = rep * n;                       // <= NQ; row = i * rep + r
  const int E = a.phys_extent, E16 = (E + 15) & ~15;
  const int W = T;                                // score rows cover the whole cache (score_off == 0 on chunk steps)
  const int t_new = T - n;
  const bool roco = sc.policy == EKV_POLICY_ROCO;
  const LdsPlan lp = ekv_lds_plan<D, NQ>(E16, W);
  float* s_e = reinterpret_cast<float*>(smem);                      // [key][NQ]
  uint32_t* s_key = reinterpret_cast<uint32_t*>(smem + lp.key_off);
  float* s_M = reinterpret_cast<float*>(smem + lp.stat_off);        // [16] row maxima
  float* s_invL = s_M + 16;                                         // [16] 1 / row sums
  float* s_rmax = s_invL + 16;                                      // [waves][8] partial maxima
  float* s_rsum = s_rmax + kLNW * 8;                                // [waves][8] partial sums
  uint32_t* s_dead = reinterpret_cast<uint32_t*>(smem + lp.dead_off);
  Blk b;
  b.tid = tid;
  b.lane = lane;
  b.wave = wave;
  b.red = reinterpret_cast<unsigned long long*>(smem + lp.red_off);
  b.phase = 0;
  uint32_t* s_hist = reinterpret_cast<uint32_t*>(smem + lp.hist_off);

  const size_t head_row = ((size_t)(a.layer_begin + ll) * a.n_kv_heads + h) * a.cap;
#ifdef EKV_LDS_PROFILE   // cycle stamps per workgroup (profiling builds only): [0] start, [1] A done, [2] statistics, [6] accumulate, [7] select, [3] scorer done, [4] B, [5] end
  unsigned long long* stamps = reinterpret_cast<unsigned long long*>(sc.tova_row) + ((size_t)ll * a.n_kv_heads + h) * 12;
#define EKV_LSTAMP(i) do { if (tid == 0) stamps[i] = __builtin_readcyclecounter(); } while (0)
#else
#define EKV_LSTAMP(i) do { } while (0)
#endif
  EKV_LSTAMP(0);
  const int32_t* slot_row = a.slot_of_pos + head_row;
  const __half* kbase = a.k + head_row * D;
  const __half* vbase = a.v + head_row * D;

  const int fl_idx = t_new + tid;                              // this thread's free-list entry (applied below)
  const int fl = slot_row[min(fl_idx, a.cap - 1)];

  // ======================================== A: logits of every physical row =============================================
  // K rows are read exactly as the fused decode kernel reads them: 16 lanes x 16 B = one 256-byte row, a wave-load covers G rows,
  // fully coalesced along head-dim, non-temporal, 12 loads per lane in flight.  q.k is an MFMA (16x16x32 f16, A = Q rows,
  // B = 8 keys): its B fragment wants lane (c, g) <- row c, 16 bytes at k-step kb, piece g, i.e. the TRANSPOSE of the
  // row-coalesced lane grid.  The transposition goes through a wave-private 8-row staging tile in LDS (2 KB per wave, XOR-swizzled
  // 16-byte pieces; no workgroup barrier: a wave only reads what it wrote).  Two rejected versions: fragment-layout loads
  // straight from global memory (64-byte segments of 16 rows per instruction: K streamed at 4.2 TB/s), and v_dot2 + a DPP
  // reduce-scatter on the row-coalesced registers (~100 dependent VALU per row at 2 waves per SIMD: 112 k cycles per head).
  constexpr int KB = D / 32;          // MFMA k-steps per row
  constexpr int PPR = D / 8;          // 16-byte pieces per row
  constexpr int LH = 8 / G;           // wave-loads per 8-row staging tile (D = 128: 2; D <= 64: 1 covers >= 8 rows)
  constexpr int TR = LH > 0 ? 8 : G;  // rows per staging tile
  constexpr int NLD = LH > 0 ? LH : 1;
  // K loads per lane in flight.  MORE IS NOT BETTER here: the chip-wide stream is bandwidth-bound either way, and every byte in flight
  // is queueing delay for the latency-bound phases of the OTHER workgroup of the CU (its scorer's loads and stores, its phase
  // hand-overs).  Measured (us per configs[1] step / per stride-4 step, same box, three interleaved rounds): 24 K + 24 V loads
  // 222.9 / 210.7, 12 + 16: 217.4 / 207.4, 8 + 16: 219.5 / 202.7, 8 + 8: 215.3 / 203.7, 12 + 8: 217.5 / 200.4; 4 K loads: slower again.
#ifndef EKV_LDS_KLOADS
#define EKV_LDS_KLOADS 12
#endif
  constexpr int NBA = EKV_LDS_KLOADS / NLD;       // tiles in flight
  const int sub = lane % LPR, grp = lane / LPR;
  const int c = lane & 15, g = lane >> 4;
  ekv_h8 aq[KB];                      // A operand: query row c
  {
    const bool ok = c < rows;
    const size_t qoff = (size_t)ll * a.n_q_heads * n * D + (size_t)(h * rep + (ok ? c % rep : 0)) * a.q_hs + (size_t)(ok ? c / rep : 0) * a.q_ts;      // (ekv_step.q_*_stride)
#pragma unroll
    for (int kb = 0; kb < KB; ++kb) {
      aq[kb] = __builtin_bit_cast(ekv_h8, reinterpret_cast<const uint4*>(a.q + qoff + kb * 32)[g]);
      if (!ok) aq[kb] = ekv_h8{0, 0, 0, 0, 0, 0, 0, 0};
    }
  }
  const int n_tiles = (E16 + TR - 1) / TR;
  const float inv_div = 1.f / a.sm_div;
  uint4 kr[NBA][NLD];
  const char* kb8 = reinterpret_cast<const char*>(kbase);
  const unsigned lane_off_a = (unsigned)sub * 16u;
  auto load_k = [&](const int buf, int t) {
    const int j0 = min(t, n_tiles - 1) * TR + grp;
#pragma unroll
    for (int u = 0; u < NLD; ++u) {
      const unsigned off = (unsigned)min(j0 + u * G, E - 1) * (unsigned)(D * 2) + lane_off_a;
      kr[buf][u] = __builtin_bit_cast(uint4, __builtin_nontemporal_load(reinterpret_cast<const ekv_u4*>(kb8 + off)));
    }
  };
  // The first tiles are requested before anything else: their addresses depend on nothing but the block index, so the dead-row
  // bits below are built under their round trip.
#pragma unroll
  for (int u = 0; u < NBA; ++u) load_k(u, wave + kLNW * u);

  // ---- dead-row bits: padding past the extent; free rows and the rows the chunk is being written to = slot-map entries
  //      [T - n, cap) ----------------------------------------------------------------------------------------------------
  {
    const int n_words = E16 / 32 + 1;
    for (int i = tid; i < n_words; i += kLNT) s_dead[i] = i * 32 >= E ? ~0u : (i * 32 + 32 > E ? ~0u << (E & 31) : 0u);
    // HW_REG_HW_ID.WAVE_ID = wave 0's slot on its SIMD, flipped every "round" of the launch (workgroups are dispatched in linear
    // order, kLdsResident at a time): the scorer-last order is the slower one (its scorer runs under the neighbour's V stream), so a
    // slot that always took it finishes after the other slot of its CU and leaves the CU half empty at the end (measured: +1 %)
    if (tid == 0) s_hist[263] = (__builtin_amdgcn_s_getreg(63492) & 0xFu) ^ ((unsigned)(h + a.n_kv_heads * ll) / kLdsResident);
    ekv_lds_barrier();     // (LDS-only barriers: the K loads stay in flight across them)
    if (fl_idx < a.cap && fl < E) atomicOr(&s_dead[fl >> 5], 1u << (fl & 31));
    for (int i = fl_idx + kLNT; i < a.cap; i += kLNT) {        // free lists longer than the workgroup: rare
      const int row = slot_row[i];
      if (row < E) atomicOr(&s_dead[row >> 5], 1u << (row & 31));
    }
    ekv_lds_barrier();
  }
  // staging tile of this wave: TR rows x D halfs, piece p of row r at (p ^ (r & (PPR - 1) & 7)) — aliases the key array of the
  // fallback select, which is only used after this phase
  char* stg = reinterpret_cast<char*>(s_key) + (size_t)wave * (TR * D * 2);
  // S = Q . K^T for the TR keys of a tile: A = Q rows, B = keys; lane (c, g) gets S[query row 4g + e][key c], e = 0..3.
  // Three steps per tile — stage (row registers -> staging tile), fetch (staging tile -> B fragments), finish (MFMA chain, / sqrt(D),
  // masks, logits -> LDS) — software-pipelined: the stage + fetch of tile u + 1 are issued BEFORE the finish of tile u, so their LDS
  // round trips run under the MFMA chain and the VALU of tile u (one tile at a time was a serial chain of ~500 cycles per tile:
  // ds_write -> ds_read -> 4 dependent MFMAs -> VALU -> ds_write; 32 k cycles per wave for a head that streams in 30 k).  ONE
  // staging tile is enough: a wave's LDS operations execute in order, so the stage of tile u + 1 lands after the fetch of tile u.
  const int rr = c & (TR - 1);                       // lanes c >= TR read a copy (their columns are not stored)
  float rmax[4] = {EKV_NEG_INF, EKV_NEG_INF, EKV_NEG_INF, EKV_NEG_INF};   // running maxima of query rows 4g .. 4g + 3 over this lane's keys
  auto stage = [&](const uint4 (&kt)[NLD]) __attribute__((always_inline)) {
#pragma unroll
    for (int u = 0; u < NLD; ++u) {
      const int r = grp + u * G;                     // row of the tile this lane's piece belongs to
      if (r < TR) *reinterpret_cast<uint4*>(stg + r * (D * 2) + ((sub ^ (r & 7 & (PPR - 1))) * 16)) = kt[u];
    }
  };
  auto fetch = [&](ekv_h8 (&bk)[KB]) __attribute__((always_inline)) {
#pragma unroll
    for (int kb = 0; kb < KB; ++kb)
      bk[kb] = *reinterpret_cast<const ekv_h8*>(stg + rr * (D * 2) + (((kb * 4 + g) ^ (rr & 7 & (PPR - 1))) * 16));
  };
  auto finish = [&](const ekv_h8 (&bk)[KB], int key0, unsigned dead_bits, int chunk_key0) __attribute__((always_inline)) {
    ekv_f4 sacc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kb = 0; kb < KB; ++kb) sacc = EKV_MFMA_16x16x32(aq[kb], bk[kb], sacc, 0, 0, 0);
    const bool dead = (dead_bits >> rr) & 1u;
    float x[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      // the reference divides by sqrt(D) (llama_patch.py:198).  q0 = s * (1/d), then one residual correction: the correctly
      // rounded quotient for every normal operand (what v_div_scale / v_div_fmas / v_div_fixup add is the handling of
      // denormals, infinities and zero divisors) in 3 instructions instead of 11
      const float q0 = sacc[e] * inv_div;
      x[e] = fmaf(fmaf(-a.sm_div, q0, sacc[e]), inv_div, q0);
      if (dead || (chunk_key0 >= 0 && chunk_key0 + rr > (4 * g + e) / rep)) x[e] = EKV_NEG_INF;   // causal inside the chunk: key i' <= query i
    }
    if (c < TR && g < QP) *reinterpret_cast<float4*>(s_e + (size_t)(key0 + c) * NQ + 4 * g) = make_float4(x[0], x[1], x[2], x[3]);
#pragma unroll
    for (int e = 0; e < 4; ++e) rmax[e] = fmaxf(rmax[e], x[e]);     // (lanes c >= TR hold copies: harmless in a maximum)
  };
  ekv_h8 bk[2][KB];
  stage(kr[0]);
  fetch(bk[0]);
  // A round = NBA tiles per wave.  Every round but the last refills each slot right after staging it — UNCONDITIONALLY (clamped): a
  // load inside a branch makes hipcc's s_waitcnt accounting assume it may not have been issued, and every later wait of the round
  // then also waits for the loads just requested (the prefetch depth decayed to 0 across a round).  The LAST round is a separate
  // copy WITHOUT the refill: loads still in flight at the end of the phase own registers the next phase wants, so the compiler
  // drains them there — and with the other workgroup of the CU streaming, that drain queues behind ITS requests (10-20 k cycles).
  auto tile_round = [&](const int t0, auto refill) __attribute__((always_inline)) {
#pragma unroll
    for (int u = 0; u < NBA; ++u) {
      const int t = t0 + kLNW * u;
      const int tw = min(t, n_tiles - 1) * TR;     // (read ahead of the next tile's LDS traffic: the finish would otherwise wait for all of it)
      const unsigned db = (s_dead[tw >> 5] >> (tw & 31)) & ((1u << TR) - 1u);   // a tile never straddles a word
      stage(kr[(u + 1) % NBA]);          // tile t + kLNW (u = NBA - 1: slot 0 was refilled at the top of this round)
      fetch(bk[(u + 1) & 1]);
      if constexpr (decltype(refill)::value) load_k(u, t + kLNW * NBA);
      if (t < n_tiles) finish(bk[u & 1], t * TR, db, -1);      // wave-uniform
    }
  };
  {
    int t0 = wave;
    for (; t0 + kLNW * NBA < n_tiles; t0 += kLNW * NBA) tile_round(t0, EkvTrue{});
    tile_round(t0, EkvLastRefill{});
  }
  auto score_tile = [&](const uint4 (&kt)[NLD], int key0, unsigned dead_bits, int chunk_key0) __attribute__((always_inline)) {
    stage(kt);
    fetch(bk[0]);
    finish(bk[0], key0, dead_bits, chunk_key0);
  };
  // the chunk's own keys (from k_new), causal inside the chunk: 16 logits columns E16 .. E16 + 15, TR at a time
  if (wave == kLNW - 1) {
#pragma unroll
    for (int t = 0; t < 16 / TR; ++t) {
      uint4 kn[NLD];
      unsigned db = 0;
#pragma unroll
      for (int u = 0; u < NLD; ++u) {
        const int i = t * TR + grp + u * G;
        // (an ext-vector load + bit cast: assigning a HIP uint4 STRUCT from memory is a memcpy through the private segment — the
        //  three dead scratch_store_dwordx4 of the round-2 build)
        kn[u] = __builtin_bit_cast(uint4, reinterpret_cast<const ekv_u4*>(a.k_new + (size_t)ll * a.n_kv_heads * n * D + (size_t)h * a.kv_hs + (size_t)min(i, n - 1) * a.kv_ts)[sub]);
      }
#pragma unroll
      for (int r = 0; r < TR; ++r) db |= (t * TR + r >= n ? 1u : 0u) << r;
      score_tile(kn, E16 + t * TR, db, t * TR);
    }
  }
  // ---- append: the chunk's K/V rows go into the recycled slots (nobody reads them in this launch) ----------------------
  {
    constexpr int PPR = D / 8;
    for (int piece = tid; piece < n * PPR; piece += kLNT) {
      const int i = piece / PPR, sub = piece % PPR;
      const size_t off = (head_row + slot_row[t_new + i]) * D;
      const size_t noff = (size_t)ll * a.n_kv_heads * n * D + (size_t)h * a.kv_hs + (size_t)i * a.kv_ts;
      reinterpret_cast<uint4*>(a.k_w + off)[sub] = reinterpret_cast<const uint4*>(a.k_new + noff)[sub];
      reinterpret_cast<uint4*>(a.v_w + off)[sub] = reinterpret_cast<const uint4*>(a.v_new + noff)[sub];
    }
  }
  // row maxima of this wave (taken on the way, no pass over the array): lanes of one g by DPP, lane c = 0 publishes rows 4g .. 4g + 3
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    rmax[e] = fmaxf(rmax[e], ekv_dpp<0xB1>(rmax[e]));
    rmax[e] = fmaxf(rmax[e], ekv_dpp<0x4E>(rmax[e]));
    rmax[e] = fmaxf(rmax[e], ekv_dpp<0x141>(rmax[e]));
    rmax[e] = fmaxf(rmax[e], ekv_dpp<0x140>(rmax[e]));
  }
  if (c == 0 && g < QP) *reinterpret_cast<float4*>(s_rmax + wave * 8 + 4 * g) = make_float4(rmax[0], rmax[1], rmax[2], rmax[3]);
  ekv_lds_barrier();   // all logits in LDS (LDS-only barrier: nothing here depends on the loads still in flight)
  EKV_LSTAMP(1);

  // ---- owned columns (positions tid + it * 256): slot-map cells and score rows; requested before the statistics
  //      pass (whose barriers are LDS-only and do not wait for them); issued later, under the other workgroup's V stream, they queue
  //      behind its requests (measured: +25 k cycles on the accumulation) ----------------------------------------------------
  int cell[kLItems];
  float rS[kLItems], rQ[kLItems], rC[kLItems];
#pragma unroll
  for (int it = 0; it < kLItems; ++it) {
    const int j = min(tid + it * kLNT, W - 1);     // unconditional (clamped) loads
    cell[it] = slot_row[j];
    rS[it] = sc.score_sum[head_row + j];
    rQ[it] = roco ? sc.score_sq[head_row + j] : 0.f;
    rC[it] = roco ? sc.score_cnt[head_row + j] : 0.f;
  }
  // ======================================== M: softmax statistics, scorer ================================================
  // float4 pieces of the [key][NQ] array: piece p = key * QP + qp holds query rows 4 qp .. 4 qp + 3 of one key.  A thread's pieces
  // (tid + 256 i) all have the same qp, so it carries 4 running maxima / sums; lanes of equal qp are merged by shuffles, waves
  // through LDS (every thread reads all 8 wave partials: one barrier per reduction).
  auto stats = [&]() __attribute__((always_inline)) {
    constexpr int NP = 12 * QP;                      // pieces per thread: up to 12 * 256 = 3072 keys
    const int n_piece = (E16 + 16) * QP;
    const int qp = tid & (QP - 1);
    float4* e4 = reinterpret_cast<float4*>(s_e);
    float4 mx = make_float4(EKV_NEG_INF, EKV_NEG_INF, EKV_NEG_INF, EKV_NEG_INF);
    // lanes of equal qp: butterflies inside the 16-lane rows by DPP (quad_perm [2,3,0,1] = xor 2 is qp-preserving for QP <= 2,
    // xor 1 only for QP == 1), then two cross-row shuffles
#define EKV_LRED4(v, OP)                                                                        \
    do {                                                                                       \
      if (QP == 1) { v.x = OP(v.x, ekv_dpp<0xB1>(v.x)); v.y = OP(v.y, ekv_dpp<0xB1>(v.y)); v.z = OP(v.z, ekv_dpp<0xB1>(v.z)); v.w = OP(v.w, ekv_dpp<0xB1>(v.w)); } \
      v.x = OP(v.x, ekv_dpp<0x4E>(v.x)); v.y = OP(v.y, ekv_dpp<0x4E>(v.y)); v.z = OP(v.z, ekv_dpp<0x4E>(v.z)); v.w = OP(v.w, ekv_dpp<0x4E>(v.w)); \
      v.x = OP(v.x, __shfl_xor(v.x, 4, 64)); v.y = OP(v.y, __shfl_xor(v.y, 4, 64)); v.z = OP(v.z, __shfl_xor(v.z, 4, 64)); v.w = OP(v.w, __shfl_xor(v.w, 4, 64)); \
      v.x = OP(v.x, __shfl_xor(v.x, 8, 64)); v.y = OP(v.y, __shfl_xor(v.y, 8, 64)); v.z = OP(v.z, __shfl_xor(v.z, 8, 64)); v.w = OP(v.w, __shfl_xor(v.w, 8, 64)); \
      v.x = OP(v.x, __shfl_xor(v.x, 16, 64)); v.y = OP(v.y, __shfl_xor(v.y, 16, 64)); v.z = OP(v.z, __shfl_xor(v.z, 16, 64)); v.w = OP(v.w, __shfl_xor(v.w, 16, 64)); \
      v.x = OP(v.x, __shfl_xor(v.x, 32, 64)); v.y = OP(v.y, __shfl_xor(v.y, 32, 64)); v.z = OP(v.z, __shfl_xor(v.z, 32, 64)); v.w = OP(v.w, __shfl_xor(v.w, 32, 64)); \
    } while (0)
#define EKV_LADD(a_, b_) ((a_) + (b_))
    // the row maxima were taken in phase A: fold the waves' partials
#pragma unroll
    for (int w = 0; w < kLNW; ++w) {
      const float4 o4 = *reinterpret_cast<const float4*>(s_rmax + w * 8 + 4 * qp);
      mx.x = fmaxf(mx.x, o4.x);
      mx.y = fmaxf(mx.y, o4.y);
      mx.z = fmaxf(mx.z, o4.z);
      mx.w = fmaxf(mx.w, o4.w);
    }
    // e = exp(x - max) as exp2((x - max) * log2(e)): v_exp_f32 (1 ulp) instead of the library expf's ~14 instructions — 16 k of these
    // per head; the difference (~1e-7 relative for the probabilities that matter) is far inside the eviction stability margin the
    // tests use (2e-5) and the 1e-3 output tolerance
    constexpr float kLog2e = 1.4426950408889634f;
    float4 sm = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      const int p = tid + kLNT * i;
      if (kLNT * i < n_piece) {       // workgroup-uniform: rounds past the end of the array are skipped altogether
        float4 x = make_float4(EKV_NEG_INF, EKV_NEG_INF, EKV_NEG_INF, EKV_NEG_INF);
        if (p < n_piece) x = e4[p];
        x.x = __builtin_amdgcn_exp2f((x.x - mx.x) * kLog2e);
        x.y = __builtin_amdgcn_exp2f((x.y - mx.y) * kLog2e);
        x.z = __builtin_amdgcn_exp2f((x.z - mx.z) * kLog2e);
        x.w = __builtin_amdgcn_exp2f((x.w - mx.w) * kLog2e);
        sm.x += x.x;
        sm.y += x.y;
        sm.z += x.z;
        sm.w += x.w;
        if (p < n_piece) e4[p] = x;
      }
    }
    EKV_LRED4(sm, EKV_LADD);
    if (lane < QP) *reinterpret_cast<float4*>(s_rsum + wave * 8 + 4 * lane) = sm;
    ekv_lds_barrier();
    if (tid < NQ) {
      float l = 0.f;
#pragma unroll
      for (int w = 0; w < kLNW; ++w) l += s_rsum[w * 8 + tid];
      s_invL[tid] = 1.f / l;     // p = e * (1 / L): see ekv_score_select.inc on why not a division per element
      s_M[tid] = 0.f;
    }
    if (tid >= 64 && tid < 72) s_hist[tid] = 0;      // scratch of the warm-started select ([66] listed, [70..71] result): published by this barrier
    ekv_lds_barrier();
    EKV_LSTAMP(2);
  };

  // ======================================== scorer (reads e and 1 / L; independent of phase B) ==============================
  auto scorer = [&]() __attribute__((always_inline)) {
    if (sc.accumulate) {
      // pbar_i = mean over the rep heads of query i (rows i * rep .. i * rep + rep - 1, summed in row order), then the column sums
      // over the queries.  Branch-free: 0 / 1 masks per row (group start, group end, last row) — the row bounds are wave-uniform
      // and hipcc otherwise turns every `q < rows` / `r == rep` into a scalar branch (thousands of lines of code for this block).
      // x * 1, x * 0 + y and y + 0 are exact, and rep is a power of two (1 / rep exact), so the values equal the reference's
      // `.mean()` then `.sum()` (easykv/easykv.py:188-196, :443-457).
      float invl[NQ], m_keep[NQ], m_end[NQ], m_last[NQ];
      const float inv_rep = 1.f / (float)rep;
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
        invl[q] = q < rows ? s_invL[q] : 0.f;
        m_keep[q] = (q % rep) != 0 ? 1.f : 0.f;                      // 0 at the first row of a query: the group sum restarts
        m_end[q] = (q < rows && (q + 1) % rep == 0) ? 1.f : 0.f;     // last row of a query: pbar complete
        m_last[q] = q == rows - 1 ? 1.f : 0.f;
      }
#pragma unroll
      for (int it = 0; it < kLItems; ++it) {
        const int j = min(tid + it * kLNT, W - 1);
        const int col = j < t_new ? cell[it] : E16 + (j - t_new);
        float v[NQ];
#pragma unroll
        for (int qq = 0; qq < QP; ++qq) {
          const float4 e = *reinterpret_cast<const float4*>(s_e + (size_t)col * NQ + 4 * qq);
          v[4 * qq] = e.x * invl[4 * qq];
          v[4 * qq + 1] = e.y * invl[4 * qq + 1];
          v[4 * qq + 2] = e.z * invl[4 * qq + 2];
          v[4 * qq + 3] = e.w * invl[4 * qq + 3];
        }
        float cs = 0.f, cq = 0.f, last = 0.f, acc = 0.f;
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
          acc = acc * m_keep[q] + v[q];
          const float pb = acc * inv_rep;
          cs += pb * m_end[q];
          cq += (pb * pb) * m_end[q];
          last += pb * m_last[q];
        }
        if (sc.policy == EKV_POLICY_TOVA) {
          rS[it] = last;
        } else {
          rS[it] += cs;
          rQ[it] += cq;
        }
      }
    }
    EKV_LSTAMP(6);

    const int k = sc.n_evict;
    if (k <= 0) {
      if (sc.accumulate) {
#pragma unroll
        for (int it = 0; it < kLItems; ++it) {
          const int j = tid + it * kLNT;
          if (j < W) {
            sc.score_sum[head_row + j] = rS[it];
            if (roco) sc.score_sq[head_row + j] = rQ[it];
          }
        }
      }
    } else {
      // ---- selection (easykv/easykv.py:462-490): roco = the k smallest means inside the feasible set F = the k1 smallest std
      //      (ties to the lower position, NaN largest); h2o_head / tova = the k smallest scores inside the window ---------------
      unsigned feas = 0;                  // bit it: column it of this thread may be evicted
      float skey[kLItems];                // what the victims are the k smallest of
      if (roco) {
        unsigned long long cv[kLItems];
#pragma unroll
        for (int it = 0; it < kLItems; ++it) {
          const int j = tid + it * kLNT;
          const float cc = rC[it] + sc.count_add;
          rC[it] = cc;
          const float mean = rS[it] / cc;
          float sd = sqrtf(rQ[it] / cc - mean * mean);
          if (j >= W - sc.roco_tail || j < sc.win_lo) sd = 1e9f;
          skey[it] = mean;
          cv[it] = j < W ? (((unsigned long long)ekv_fkey(sd) << 32) | (uint32_t)j) : ~0ull;
        }
        uint32_t* hint_p = sc.slot_state != nullptr ? reinterpret_cast<uint32_t*>(sc.slot_state) + 4 * ((size_t)(a.layer_begin + ll) * a.n_kv_heads + h) + 3 : nullptr;
        const uint32_t hint = hint_p != nullptr ? *hint_p : 0u;
        unsigned long long thr = 0;
        if (hint != 0u) thr = lds_warm_threshold(b, cv, W, sc.roco_k1, hint, s_hist, reinterpret_cast<unsigned long long*>(s_hist + 264), kListCap);
        if (thr == 0) thr = lds_kth_threshold(b, cv, W, sc.roco_k1, s_hist, reinterpret_cast<unsigned long long*>(s_hist + 264), kListCap);
        if (hint_p != nullptr && tid == 0) {      // hint for the head's next chunk step (0 = none: a sentinel key is no useful pivot)
          const uint32_t kt = (uint32_t)((thr - 1ull) >> 32);
          *hint_p = (thr != 0 && kt != 0u && kt < ekv_fkey(1e9f)) ? kt : 0u;
        }
        if (thr != 0) {
#pragma unroll
          for (int it = 0; it < kLItems; ++it) feas |= (cv[it] < thr ? 1u : 0u) << it;
        } else {     // tiny rows / a bin too crowded to list: the generic exact select on the keys in LDS
#pragma unroll
          for (int it = 0; it < kLItems; ++it) {
            const int j = tid + it * kLNT;
            if (j < W) s_key[j] = (uint32_t)(cv[it] >> 32);
          }
          __syncthreads();
          [[clang::always_inline]] blk_mark_k_smallest(b, s_key, W, sc.roco_k1, s_hist, ekv_fkey(1e9f), kListCap);   // (a real call would put `b` in the private segment)
#pragma unroll
          for (int it = 0; it < kLItems; ++it) {
            const int j = tid + it * kLNT;
            feas |= ((j < W && s_key[j]) ? 1u : 0u) << it;
          }
          __syncthreads();
        }
      } else {
#pragma unroll
        for (int it = 0; it < kLItems; ++it) {
          const int j = tid + it * kLNT;
          skey[it] = rS[it];
          feas |= ((j >= sc.win_lo && j < W - sc.win_tail) ? 1u : 0u) << it;
        }
      }
      EKV_LSTAMP(7);
      // k <= 16 victims: k rounds of one block-wide arg-min each (one LDS-only barrier per round).  A thread proposes the best of
      // its own columns and recomputes it only when that column has just been taken.
      int32_t* s_vict = reinterpret_cast<int32_t*>(s_hist + 100);     // k victim positions (histogram scratch is idle now)
      // Every wave finds ITS k smallest by k wave-wide arg-min rounds (DPP + readlane, no LDS, no barrier); the k smallest of the
      // workgroup are among those 4k candidates and are ranked by counting (composites are unique).  (Round 2: k block-wide rounds,
      // one barrier and two ds_bpermute round trips each.)
      unsigned long long* cand = reinterpret_cast<unsigned long long*>(s_hist + 128);     // [4][16] (the pivots are dead)
      unsigned long long mv[kLItems];     // composites (order-preserving key, position) of the feasible columns, ~0 otherwise / once taken
#pragma unroll
      for (int it = 0; it < kLItems; ++it)
        mv[it] = ((feas >> it) & 1u) ? (((unsigned long long)ekv_fkey(skey[it]) << 32) | (uint32_t)(tid + it * kLNT)) : ~0ull;
      auto own_best = [&]() __attribute__((always_inline)) {
        unsigned long long best = mv[0];
#pragma unroll
        for (int it = 1; it < kLItems; ++it) best = mv[it] < best ? mv[it] : best;
        return best;
      };
      unsigned long long mine = own_best();
      for (int r = 0; r < k; ++r) {
        const unsigned long long best = lds_wave_min_u64(mine);
        if (best == mine && best != ~0ull) {       // composites are unique: only the owner matches
#pragma unroll
          for (int it = 0; it < kLItems; ++it) mv[it] = mv[it] == best ? ~0ull : mv[it];
          mine = own_best();
        }
        if (lane == 0) cand[wave * 16 + r] = best;
      }
      ekv_lds_barrier();
      if (tid < kLNW * 16) {
        const int w = tid >> 4, r = tid & 15;
        const unsigned long long x = r < k ? cand[tid] : ~0ull;
        int rank = 0;
#pragma unroll
        for (int ww = 0; ww < kLNW; ++ww)
          for (int rr2 = 0; rr2 < k; ++rr2) rank += cand[ww * 16 + rr2] < x ? 1 : 0;
        // ~0 = "this wave ran out of feasible columns" (duplicates): they rank after every real candidate; the k-th slot is -1 only
        // when fewer than k real candidates exist at all
        if (x != ~0ull && rank < k) s_vict[rank] = (int)(x & 0xFFFFFFFFu);
        if (x == ~0ull && r < k && w == 0) {
          int real = 0;
          for (int ww = 0; ww < kLNW; ++ww)
            for (int rr2 = 0; rr2 < k; ++rr2) real += cand[ww * 16 + rr2] != ~0ull ? 1 : 0;
          if (r >= real) s_vict[r] = -1;
        }
      }
      EKV_LSTAMP(11);
      ekv_lds_barrier();
    }
    EKV_LSTAMP(3);
  };
  // ---- write back: compacted score rows, evict ids (ascending), compacted slot map (cells are still in registers) ------
  // A lambda of its own since round 4: the workgroup that runs the scorer BEFORE its V stream issues these stores AFTER the stream
  // (EKV_LDS_WB = 1: 210.4 vs 211.9 us per configs[1] step; after the output stage: 210.7).  What the write-back costs, measured by
  // leaving parts of it out (same box, us per step, 212 with everything): no stores at all 188; the same store instructions aimed at a
  // 1 KB window per array (no DRAM traffic) 197; the same bytes as 16-byte stores 207 — i.e. ~15 of its 24 us are the 34 MB of DRAM
  // writes themselves (written bytes cost about twice what read bytes do in the middle of a read stream), ~5 the instruction count.
  auto write_back = [&]() __attribute__((always_inline)) {
    const int k = sc.n_evict;
    if (k <= 0) return;
    {
      const int32_t* s_vict = reinterpret_cast<const int32_t*>(s_hist + 100);
      int vict[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) vict[r] = r < k ? s_vict[r] : 0x7FFFFFFF;
#pragma unroll
      for (int it = 0; it < kLItems; ++it) {
        const int j = tid + it * kLNT;
        if (j < W) {
          int before = 0;
          bool is_v = false;
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            if (r < k) {       // uniform
              before += vict[r] < j ? 1 : 0;
              is_v |= vict[r] == j;
            }
          }
          if (!is_v) {
            const int d = j - before;
            sc.score_sum[head_row + d] = rS[it];
            if (roco) {
              sc.score_sq[head_row + d] = rQ[it];
              sc.score_cnt[head_row + d] = rC[it];
            }
            sc.slot_of_pos[head_row + d] = cell[it];
          } else {
            if (sc.evict_ids != nullptr) sc.evict_ids[((size_t)ll * sc.n_kv_heads + h) * k + before] = j;
            sc.slot_of_pos[head_row + (W - k) + before] = cell[it];
          }
        }
      }
      for (int i = tid; i < k; i += kLNT) {
        sc.score_sum[head_row + W - k + i] = 0.f;
        if (roco) {
          sc.score_sq[head_row + W - k + i] = 0.f;
          sc.score_cnt[head_row + W - k + i] = (float)i * sc.count_tail_step;
        }
      }
    }
  };
  // ======================================== B: O = sum_j e_j v_j =========================================================
  ekv_f4 acc[8];       // D = 128: phase B's accumulators (MFMA form)
  auto b_stream = [&](auto raw) __attribute__((always_inline)) {
    constexpr bool RAW = decltype(raw)::value;
    // V rows are read like K (16 lanes x 16 B per row, non-temporal), lane group g of a wave-batch holding the 8 CONSECUTIVE rows
    // 8g .. 8g + 7 of a 32-row block.  That is already the k-slice structure of mfma_f32_16x16x32_f16's B operand (lane (n, g) <-
    // B[8g .. 8g + 7][n]) up to an 8 x 8 transpose of halfs INSIDE the lane: 32 v_perm_b32 turn the 8 row registers (8 d's of one
    // key each) into 8 operands (8 keys of one d each), operand i = columns d = 8 n + i.  A = P (query rows x 32 keys, fp16 — one
    // fp16 per probability is the reference's own arithmetic, llama_patch.py:207-213) comes from the fp32 array in LDS, 8
    // ds_read_b32 per lane and block.  8 MFMAs per 32 rows replace 256 v_pk_fma_f32 + 64 v_cvt per lane (round 2: the phase was
    // VALU-bound, 41 k cycles per wave alone on its SIMD, 80 k with the other workgroup of the CU in the same phase) and the
    // MFMA sums over the lane groups, so there is no in-wave shuffle reduction either.
    const int pq = c < NQ ? c : 0;             // lane (c, g) feeds query row c of the A operand (rows >= NQ: zero)
#ifndef EKV_LDS_VBATCHES
#define EKV_LDS_VBATCHES 1
#endif
    constexpr int KUB = 8, NB = EKV_LDS_VBATCHES, RB = 32;    // rows per lane group and batch, batches in flight (8 loads per lane: see EKV_LDS_KLOADS), rows per batch
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i] = ekv_f4{0.f, 0.f, 0.f, 0.f};
    // RAW: the array still holds the raw logits (the statistics pass has not run): e = exp2((x - max) * log2 e) is taken here, by the
    // same expression as the statistics pass (bit-identical P), from the row maximum phase A left
    float mxq = 0.f;
    if constexpr (RAW) {
      mxq = EKV_NEG_INF;
#pragma unroll
      for (int w = 0; w < kLNW; ++w) mxq = fmaxf(mxq, s_rmax[w * 8 + pq]);
    }
    const uint8_t* dead8p = reinterpret_cast<const uint8_t*>(s_dead);
    const char* vb8 = reinterpret_cast<const char*>(vbase);
    const int key_max = E16 + 15;
    auto pv_block = [&](const uint4 (&v)[KUB], int key0) __attribute__((always_inline)) {
      ekv_h8 pa;
      const float* ep = s_e + (size_t)min(key0, key_max - 7) * NQ + pq;   // (only the chunk's block can start past the array: its V rows are zero)
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        float e = ep[k * NQ];
        if constexpr (RAW) e = __builtin_amdgcn_exp2f((e - mxq) * 1.4426950408889634f);
        pa[k] = (ekv_e)(c < NQ ? e : 0.f);
      }
      uint32_t tb[8][4];
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        const uint32_t ra[4] = {v[2 * p].x, v[2 * p].y, v[2 * p].z, v[2 * p].w};
        const uint32_t rb[4] = {v[2 * p + 1].x, v[2 * p + 1].y, v[2 * p + 1].z, v[2 * p + 1].w};
#pragma unroll
        for (int m = 0; m < 4; ++m) {
          tb[2 * m][p] = __builtin_amdgcn_perm(rb[m], ra[m], 0x05040100u);        // (key 2p + 1, key 2p) of d = 2m
          tb[2 * m + 1][p] = __builtin_amdgcn_perm(rb[m], ra[m], 0x07060302u);    // ... of d = 2m + 1
        }
      }
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const ekv_u4 t4 = {tb[i][0], tb[i][1], tb[i][2], tb[i][3]};
        acc[i] = EKV_MFMA_16x16x32(pa, __builtin_bit_cast(ekv_h8, t4), acc[i], 0, 0, 0);
      }
    };
    const int n_batches = (E16 + RB - 1) / RB;
    uint4 vr[NB][KUB];
    auto load_batch = [&](const int buf, int bt) __attribute__((always_inline)) {
      const int j0 = min(bt, n_batches - 1) * RB + grp * KUB;
#pragma unroll
      for (int u = 0; u < KUB; ++u) {
        const unsigned off = (unsigned)min(j0 + u, E - 1) * (unsigned)(D * 2) + lane_off_a;
        vr[buf][u] = __builtin_bit_cast(uint4, __builtin_nontemporal_load(reinterpret_cast<const ekv_u4*>(vb8 + off)));
      }
    };
#pragma unroll
    for (int u = 0; u < NB; ++u) load_batch(u, wave + kLNW * u);
    auto batch_round = [&](const int b0, auto refill) __attribute__((always_inline)) {      // (last round without refills: see phase A)
#pragma unroll
      for (int u = 0; u < NB; ++u) {
        const int bt = b0 + kLNW * u;
        if (bt < n_batches) {       // wave-uniform
          const int j0 = bt * RB + grp * KUB;
          const unsigned d8 = dead8p[j0 >> 3];       // (words up to E16 / 32 are initialised: rows >= E are dead)
          if (d8 != 0u) {           // rare: a dead row may hold anything (0 * inf = NaN): its e is 0, its V is replaced by 0
#pragma unroll
            for (int r = 0; r < KUB; ++r)
              if ((d8 >> r) & 1u) vr[u][r] = uint4{0, 0, 0, 0};
          }
          pv_block(vr[u], j0);
        }
        if constexpr (decltype(refill)::value) load_batch(u, bt + kLNW * NB);     // unconditional (clamped inside)
      }
    };
    {
      int b0 = wave;
      for (; b0 + kLNW * NB < n_batches; b0 += kLNW * NB) batch_round(b0, EkvTrue{});
      batch_round(b0, EkvLastRefill{});
    }
    if (wave == kLNW - 1) {   // the chunk's own rows (from v_new): keys E16 .. E16 + 15
      uint4 vn[KUB];
#pragma unroll
      for (int u = 0; u < KUB; ++u) {
        const int i = grp * KUB + u;
        vn[u] = __builtin_bit_cast(uint4, reinterpret_cast<const ekv_u4*>(a.v_new + (size_t)ll * a.n_kv_heads * n * D + (size_t)h * a.kv_hs + (size_t)min(i, n - 1) * a.kv_ts)[sub]);
        if (i >= n) vn[u] = uint4{0, 0, 0, 0};
      }
      pv_block(vn, E16 + grp * KUB);
    }
  };
  auto b_out = [&]() __attribute__((always_inline)) {
    EKV_LSTAMP(4);
    // accumulator i of lane (c, g): O[query row 4g + e][d = 8c + i], e = 0..3.  Cross-wave sum as a fixed tree, (w0 + w2) + (w1 + w3),
    // through two [q][D] fp32 tiles in the key array of the fallback select (idle here: the scorer runs strictly before or after this
    // phase) — the logits array stays intact, so the scorer may also run AFTER this phase.
    float* scr = reinterpret_cast<float*>(s_key);   // [2][NQ][D]
    auto tile_rw = [&](const bool add) __attribute__((always_inline)) {
      if (g < QP) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          ekv_f4* dst = reinterpret_cast<ekv_f4*>(scr + ((size_t)(wave & 1) * NQ + 4 * g + e) * D + c * 8);   // (ext-vector type: a HIP float4 copied from memory goes through the private segment)
          ekv_f4 lo = {acc[0][e], acc[1][e], acc[2][e], acc[3][e]}, hi = {acc[4][e], acc[5][e], acc[6][e], acc[7][e]};
          if (add) {
            lo += dst[0];
            hi += dst[1];
          }
          dst[0] = lo;
          dst[1] = hi;
        }
      }
    };
    if (wave >= 2) tile_rw(false);
    ekv_lds_barrier();
    if (wave < 2) tile_rw(true);
    ekv_lds_barrier();
    for (int idx = tid; idx < rows * D; idx += kLNT) {
      const int q = idx / D, d = idx % D;
      sc.out[(size_t)ll * a.n_q_heads * n * D + (size_t)(h * rep + q % rep) * a.o_hs + (size_t)(q / rep) * a.o_ts + d] =
          ekv_to_e((scr[(size_t)q * D + d] + scr[((size_t)NQ + q) * D + d]) * s_invL[q]);
    }
  };
  auto phase_b_valu = [&]() __attribute__((always_inline)) {      // D = 64 / 32
  {
    ekv_f2 o[NQ][4];
  #pragma unroll
    for (int q = 0; q < NQ; ++q)
  #pragma unroll
      for (int i = 0; i < 4; ++i) o[q][i] = ekv_f2{0.f, 0.f};
    {
      constexpr int kUB = 4;            // rows per lane group and batch
      constexpr int NB = 4;             // batches in flight (16 loads per lane)
      constexpr int RB = G * kUB;       // rows per wave and batch
      const uint8_t* dead8p = reinterpret_cast<const uint8_t*>(s_dead);
      const char* vb8 = reinterpret_cast<const char*>(vbase);
      // one V row at a time: its 8 halfs are widened once and reused by all query rows (v_pk_fma_f32: two accumulators per
      // instruction); the e of the row for all query rows = NQ consecutive floats
      auto pv_row = [&](const uint4& vrow, int col) {
        const ekv_h8 hv = __builtin_bit_cast(ekv_h8, vrow);
        ekv_f2 f[4];
  #pragma unroll
        for (int i = 0; i < 4; ++i) f[i] = ekv_f2{(float)hv[2 * i], (float)hv[2 * i + 1]};
  #pragma unroll
        for (int qq = 0; qq < QP; ++qq) {
          const float4 e = *reinterpret_cast<const float4*>(s_e + (size_t)col * NQ + 4 * qq);
          const float ev[4] = {e.x, e.y, e.z, e.w};
  #pragma unroll
          for (int r = 0; r < 4; ++r) {
            const ekv_f2 pe = ekv_f2{ev[r], ev[r]};
  #pragma unroll
            for (int i = 0; i < 4; ++i) o[4 * qq + r][i] = __builtin_elementwise_fma(pe, f[i], o[4 * qq + r][i]);
          }
        }
      };
      // batches of RB rows: wave, wave + NW, ...; NB batches in flight
      const int n_batches = (E16 + RB - 1) / RB;
      uint4 vr[NB][kUB];
      auto load_batch = [&](const int buf, int bt) {
        const int j0 = min(bt, n_batches - 1) * RB + grp * kUB;
  #pragma unroll
        for (int u = 0; u < kUB; ++u) {
          const unsigned off = (unsigned)min(j0 + u, E - 1) * (unsigned)(D * 2) + lane_off_a;
          vr[buf][u] = __builtin_bit_cast(uint4, __builtin_nontemporal_load(reinterpret_cast<const ekv_u4*>(vb8 + off)));
        }
      };
  #pragma unroll
      for (int u = 0; u < NB; ++u) load_batch(u, wave + kLNW * u);
      for (int b0 = wave; b0 < n_batches; b0 += kLNW * NB) {
  #pragma unroll
        for (int u = 0; u < NB; ++u) {
          const int bt = b0 + kLNW * u;
          if (bt < n_batches) {       // wave-uniform
            const int j0 = bt * RB + grp * kUB;
            const unsigned d4 = j0 < E16 ? (dead8p[j0 >> 3] >> (j0 & 4)) & 0xFu : 0xFu;
            if (d4 != 0u) {           // rare: a dead row may hold anything (0 * inf = NaN): its e is 0, its V is replaced by 0
  #pragma unroll
              for (int r = 0; r < kUB; ++r)
                if ((d4 >> r) & 1u) vr[u][r] = uint4{0, 0, 0, 0};
            }
  #pragma unroll
            for (int r = 0; r < kUB; ++r) pv_row(vr[u][r], min(j0 + r, E16 - 1));
          }
          load_batch(u, bt + kLNW * NB);     // unconditional (clamped inside), see phase A
        }
      }
      if (wave == kLNW - 1) {   // the chunk's own rows (from v_new): keys E16 .. E16 + 15
  #pragma unroll
        for (int r = 0; r < 16 / G; ++r) {
          const int i = r * G + grp;
          uint4 vn = reinterpret_cast<const uint4*>(a.v_new + (size_t)ll * a.n_kv_heads * n * D + (size_t)h * a.kv_hs + (size_t)min(i, n - 1) * a.kv_ts)[sub];
          if (i >= n) vn = uint4{0, 0, 0, 0};
          pv_row(vn, E16 + i);
        }
      }
      // in-wave: the G lane groups hold different rows of the same 8-wide slice
  #pragma unroll
      for (int off = LPR; off < 64; off <<= 1)
  #pragma unroll
        for (int q = 0; q < NQ; ++q)
  #pragma unroll
          for (int i = 0; i < 4; ++i) {
            o[q][i].x += __shfl_xor(o[q][i].x, off, 64);
            o[q][i].y += __shfl_xor(o[q][i].y, off, 64);
          }
      ekv_lds_barrier();   // every wave has finished reading e: the logits buffer becomes the cross-wave scratch
      EKV_LSTAMP(4);
      float* scr = s_e;  // [wave][q][D]
      if (grp == 0) {
  #pragma unroll
        for (int q = 0; q < NQ; ++q) {
          float* dst = scr + ((size_t)wave * NQ + q) * D + sub * 8;
          *reinterpret_cast<float4*>(dst) = make_float4(o[q][0].x, o[q][0].y, o[q][1].x, o[q][1].y);
          *reinterpret_cast<float4*>(dst + 4) = make_float4(o[q][2].x, o[q][2].y, o[q][3].x, o[q][3].y);
        }
      }
      ekv_lds_barrier();
      for (int idx = tid; idx < rows * D; idx += kLNT) {
        const int q = idx / D, d = idx % D;
        float acc = 0.f;
  #pragma unroll
        for (int w = 0; w < kLNW; ++w) acc += scr[((size_t)w * NQ + q) * D + d];
        sc.out[(size_t)ll * a.n_q_heads * n * D + (size_t)(h * rep + q % rep) * a.o_hs + (size_t)(q / rep) * a.o_ts + d] = ekv_to_e(acc * s_invL[q]);
      }
    }
  }
  };
  // Phase B needs e and 1 / L only, not the scorer, and the scorer touches no K / V: with TWO workgroups per CU, one runs its
  // scorer (latency chains in LDS, no HBM traffic) while the other streams V, and then the other way round — provided they take
  // the two phases in OPPOSITE order.  The order bit is the parity of wave 0's hardware wave slot: the two workgroups resident on
  // a CU hold different slots of a SIMD, and a workgroup that starts later takes the slot its predecessor freed, i.e. the
  // parity the still-running neighbour does not have.  (Both workgroups in the same order = both scorers at the same time =
  // the CU's share of HBM idle for a third of the step: 260 us per 32-layer step at configs[1] in round 2.)
  bool b_first = false;
  if constexpr (D == 128) {
#if EKV_LDS_ORDER == 2
    b_first = (s_hist[263] & 1u) != 0u;
#else
    b_first = EKV_LDS_ORDER != 0;
#endif
  }
  // ONE copy of the statistics pass and of the scorer between two copies of phase B (it is small): a two-trip loop over one copy of
  // each keeps both phases' registers live at once and spills; two copies of the scorer stop its helpers from being inlined.
  // The B-first workgroup streams V BEFORE the statistics pass (phase B then takes exp itself, from the row maxima of phase A), so
  // that its V stream starts the moment both workgroups leave phase A — the neighbour's statistics + scorer run under it — and no
  // window is left in which both workgroups of the lock-stepped first pair sit in the statistics pass with the HBM share idle.
  if constexpr (D == 128) {
    if (b_first) b_stream(EkvTrue{});
    ekv_lds_barrier();       // (every wave has read the raw logits it needs: the statistics pass overwrites them with e)
    stats();
    if (b_first) b_out();
    ekv_lds_barrier();
    scorer();
#ifndef EKV_LDS_WB
#define EKV_LDS_WB 1   // where the scorer-first workgroup writes back: 0 right after the scorer, 1 after the V stream, 2 after the output stage
#endif
    if (b_first || EKV_LDS_WB == 0) write_back();
    ekv_lds_barrier();
    if (!b_first) {
      b_stream(EkvFalse{});
      if (EKV_LDS_WB == 1) write_back();
      b_out();
      if (EKV_LDS_WB == 2) write_back();
    }
  } else {
    stats();
    scorer();
    write_back();
    ekv_lds_barrier();
    phase_b_valu();
  }
  EKV_LSTAMP(5);
#ifdef EKV_LDS_PROFILE
  if (tid == 0) {
    stamps[8] = __builtin_amdgcn_s_getreg(63492);   // HW_REG_HW_ID
    stamps[9] = __builtin_amdgcn_s_getreg(63508);   // HW_REG_XCC_ID
    stamps[10] = b_first ? 1 : 0;
  }
#endif
}

template <int NQ>
hipError_t launch_lds(const EkvAttnArgs& a, const EkvScoreArgs& sc, int layer_count, hipStream_t s) {
  const int e16 = (a.phys_extent + 15) & ~15;
  const size_t lds = ekv_lds_plan<EKV_D, NQ>(e16, a.n_slots).total;
  if (lds > 48 * 1024)
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&ekv_chunk_lds_kernel<EKV_D, NQ>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL((ekv_chunk_lds_kernel<EKV_D, NQ>), dim3(1, a.n_kv_heads, layer_count), dim3(kLNT), lds, s, a, sc);
  return hipGetLastError();
}

}  // namespace

hipError_t EKV_FN_D_ELEM(ekv_launch_chunk_lds, EKV_D, EKV_ELEM)(const EkvAttnArgs& a, const EkvScoreArgs& sc, int layer_count, hipStream_t s) {
  const int rows = (a.n_q_heads / a.n_kv_heads) * a.q_len;
  if (rows > 8 || a.n_slots > kLItems * kLNT) return hipErrorInvalidValue;
  return rows <= 4 ? launch_lds<4>(a, sc, layer_count, s) : launch_lds<8>(a, sc, layer_count, s);
}
