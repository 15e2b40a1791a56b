// The streaming loop of the decode attention (shared by the split and the fused kernels).
//
// Mapping (D = 128): a K/V row is 256 B; 16 lanes x 16 B read one row fully coalesced along the
// head-dim axis, a wave64 load instruction covers 4 rows, each lane keeps kU = 8 K and 8 V loads in
// flight.  QK^T is v_dot2c_f32_f16 + a fused v_add_f32_dpp butterfly over the lanes of a row; softmax is
// lane-local online (exp2), so there is no cross-row traffic inside the loop.  One workgroup serves the
// REP query heads of one KV head (GQA: the K/V rows are read once).
#pragma once
#include "ekv_common.h"
#include "ekv_kernels.h"

// EkvDecodeGeom, kU and the LDS bytes of the one-launch kernel (ekv_fused_lds): ekv_geometry.h

// Streams positions [t0, t1) of KV head h.  SLOT_LDS: s_slot holds slot_of_pos[t0..t1) in LDS; otherwise s_slot is
// the head's row of the global slot map (t0 must be a multiple of 8) and the 8 indices of a lane group are fetched
// one iteration ahead.  Logits (q.k / sm_div) go to `logit_out` (+ `logit_stride` per query head): workspace or LDS.
//
// PHYS (fused kernel, t0 = 0, t1 = T): the rows are streamed in PHYSICAL order, 0 .. a.phys_extent-1, not through the slot
// map.  Eviction recycles rows in place, so after a few thousand steps of a score-driven policy the birth order of the
// live rows is a random permutation of their addresses, while attention does not care about the order: streaming by
// address keeps the HBM access pattern sequential whatever the eviction history was and takes the slot-map loads out of the
// loop.  (Measured on MI355X at T = 2049, D = 128: gathering whole 256-byte rows in random order costs nothing measurable,
// +-3 % run-to-run noise either way; the 188 -> 223 us drift of the first version over 1000+ steps was the roco select
// falling through to its bisection fallback, see ekv_decode_tail.h.)
// `s_dead` (LDS, one bit per row) marks free rows, the row the new token is being written to and the padding past the
// extent; logits are stored at the PHYSICAL row index (the scorer tail reads them back through the slot map).
// `mask_ready` (PHYS): finishes the dead-row bits (LDS barriers inside, so every wave calls it exactly once).  It runs after
// the loads of the wave's FIRST iteration have been issued — the K/V addresses do not depend on it — so the round trip of the
// free list hides behind the first K/V round trip instead of preceding it.
struct EkvNoop {
  __device__ __forceinline__ void operator()() const {}
};
// KU = rows in flight per lane group (K and V each): 8 (122 VGPRs in the fused kernel = four workgroups per CU).  16 is
// supported for plain keys in logical order and was tried in the split kernel (ekv_attn_decode.inc): no gain.
#ifndef EKV_ROPE_MOCK
#define EKV_ROPE_MOCK 0      // experiment builds of the RoPE-on-read decode stream: 1 = no table loads, 2 = no partner exchange
#endif
//
// FP8 rows (EPL = 16, deduced from `o`; plain keys, head_dim 64 / 128): a.k / a.v are the code planes, one byte per element, and
// a.k_scale / a.v_scale the fp32 row scales at the same physical index.  A lane's piece is 16 codes against 16 query elements; the
// codes are widened in registers (ekv_common.h), logit = (q . codes) * k_scale[row] / sm_div, and v_scale[row] is folded into p
// before the axpy.  The scales of an iteration's KU rows are read as 16-byte vectors when the rows are consecutive (PHYS) and per row
// through the slot map otherwise.  The appended row is quantised here (row maximum over the lane group, codes + scale stored) and
// takes part in the step AS QUANTISED, so the bank's contents alone determine the step.
//
// MXFP4 rows (EPL = 32; plain keys, head_dim 128): a.k / a.v are the code planes, two e2m1 codes per byte, and a.k_exp / a.v_exp the
// E8M0 bytes, four per row at the same physical index.  A row is a 4-lane group and a lane's piece is exactly ONE block: 32 codes
// against 32 query elements, so the block's 2^e multiplies the lane's partial dot product BEFORE the lane-group sum, and on the V
// side goes into the conversion of the lane's codes to fp32.  The exponent words of an iteration's KU rows are read as 16-byte
// vectors when the rows are consecutive (PHYS) and per row through the slot map otherwise.  The appended row is quantised here, one
// block per lane, and takes part in the step as quantised.
//
// MXFP6 rows (EPL = 32 like MXFP4, told apart by the format tag FMT = 6; plain keys, head_dim 128): the geometry, the exponent planes
// and everything around the piece are MXFP4's.  The piece is the block's 24 bytes at byte 24 * sub of a 96-byte row (8-byte aligned:
// three 8-byte loads, six registers per row in flight); K: the 32 codes widened to packed 16-bit pairs, V: to fp32 under the block's
// scale (ekv_common.h).
//
// FP8-key / MXFP4-value rows (EPL = 16 like FP8, told apart by the format tag FMT = 84; plain keys, head_dim 128): the K side IS the FP8
// rows' — codes, row scales, dot product, group sum, the appended row's K quantisation — so logits and (m, l) partials are bit for bit
// those of an FP8 step on the same K codes.  The V plane is MXFP4's (64-byte rows, a.v_exp: four E8M0 bytes per row) read on the FP8
// geometry: a lane's piece is 8 bytes, 16 e2m1 codes = half a block, at byte 8 * sub of the row, and lane `sub` takes exponent byte
// sub >> 1.  The exponent words are read as MXFP4 reads them.  The appended V row: block maximum over the lane pair, 16 codes per lane,
// the even lane stores the exponent byte.
//
// 16-bit-key / MXFP4-value rows (EPL = 8 like 16-bit rows, told apart by the format tag FMT = 164; plain keys, head_dim 128): the K side
// IS the 16-bit rows' — the 16-byte non-temporal load, ekv_dot8, the group sum over 16 lanes, / sm_div, the appended K row stored as it
// comes — so logits and (m, l) partials are bit for bit those of a 16-bit step on the same K rows.  The V plane is MXFP4's (64-byte rows,
// a.v_exp: four E8M0 bytes per row) read on the 16-bit geometry: a lane's piece is 4 bytes, 8 e2m1 codes = a quarter of a block — its
// own 8 output elements — at byte 4 * sub of the row, and lane `sub` takes exponent byte sub >> 2.  The exponent words are read as MXFP4
// reads them.  The appended V row: block maximum over the lane quad, 8 codes per lane, lane sub % 4 == 0 stores the exponent byte, and
// the row is attended as quantised.  No resident rows and no phase order K (ekv_attn_decode.inc).
//
// Load policy of the 16-bit K/V rows.  A row is read exactly once per step and the bank (> 1 GB at the flagship shape) never fits L2 or
// the 256 MiB Infinity Cache: non-temporal loads (measured on MI355X: 5.5 -> 6.1 TB/s on the pure stream).  But step i + 1 reads the
// rows of step i except one per head, so a fixed SHARE of the bank can stay in the Infinity Cache from step to step.  RES (the
// instances named in ekv_attn_decode.inc, kResident; PHYS only): the wave iterations over the physical rows [0, res_rows) — a multiple
// of RW, planned per launch (ekv_decode_resident_rows, ekv_plan.h) — issue default-policy loads, all others non-temporal ones.  The
// policy is an instruction modifier, so an iteration's requests exist twice, under a wave-uniform branch (base is per wave); the row ->
// (wave, lane group, iteration) mapping, the request order, the clamping and everything behind the loads are shared and unchanged.
template <bool RESIDENT>
__device__ __forceinline__ uint4 ekv_load_row_piece(const char* row, int sub) {
  const ekv_u4* p = reinterpret_cast<const ekv_u4*>(row) + sub;
  if constexpr (RESIDENT) return __builtin_bit_cast(uint4, *p);
  else return __builtin_bit_cast(uint4, __builtin_nontemporal_load(p));
}
template <bool B>
struct EkvBool {
  static constexpr bool value = B;
};

template <int D, int REP, bool ROPE, bool SLOT_LDS, int NW = 4, bool PHYS = false, int KU = kU, typename MaskReady = EkvNoop, int EPL = 8, int FMT = 0, bool RES = false>
__device__ __forceinline__ void ekv_decode_stream(const EkvAttnArgs& a, const int32_t* s_slot, float* logit_out,
                                                  int logit_stride, int t0, int t1_in, int ll, int h, size_t head_row,
                                                  float (&m)[REP], float (&l)[REP], float (&o)[REP][EPL],
                                                  const uint8_t* s_dead = nullptr, MaskReady mask_ready = MaskReady(),
                                                  int n_rep_real = 0, int q_head0 = -1, int res_rows = 0
                                                  EKV_SINK_ONLY(, const float* sink_row = nullptr)      // (the sinks of this bank layer's query heads)
                                                  EKV_WIN_ONLY(, const EkvWinArgs win = EkvWinArgs{})) {      // (sliding windows: below)
  static_assert(!RES || (PHYS && EPL == 8 && D == 128), "resident rows: 16-bit rows of head_dim 128 (whole lane groups) in physical order");
  using Gm = EkvDecodeGeom<D, NW, KU, EPL>;
  constexpr int LPR = Gm::LPR, RW = Gm::RW, LIVE = Gm::LIVE;
  constexpr bool KV8 = EPL == 16, KV4 = EPL == 32;      // (KV4: the MX geometry, one block per lane — MXFP4 and MXFP6 rows)
  constexpr bool KV6 = KV4 && FMT == 6;
  constexpr bool KV84 = KV8 && FMT == 84;      // FP8 keys (everything KV8 says about K holds), MXFP4 values
  constexpr bool KV164 = EPL == 8 && FMT == 164;      // 16-bit keys (the K side is the 16-bit code itself), MXFP4 values
  constexpr bool V4 = KV84 || KV164;      // the V plane is MXFP4's: 64-byte rows under a.v_exp, LPR / 4 lanes per block
  constexpr int VSH = KV164 ? 2 : 1;      // ... lane `sub` holds a piece of block sub >> VSH
  static_assert(FMT == 0 || KV6 || KV84 || KV164,
                "format tag: 6 = MXFP6 rows (EPL = 32), 84 = FP8 keys with MXFP4 values (EPL = 16), 164 = 16-bit keys with MXFP4 values (EPL = 8)");
  static_assert(!KV84 || (D == 128 && LPR == 8), "FP8-key / MXFP4-value rows: head_dim 128 (a lane pair = one 32-element V block)");
  static_assert(!KV164 || (D == 128 && LPR == 16 && !ROPE && !RES), "16-bit-key / MXFP4-value rows: plain keys, head_dim 128 (a lane quad = one 32-element V block), no resident rows");
  static_assert(EPL == 8 || (KV8 && !ROPE && LIVE == LPR) || KV4, "FP8 rows: plain keys, head_dim 64 / 128");
  static_assert(!KV4 || (!ROPE && D == 128 && LPR == 4), "MXFP4 rows: plain keys, head_dim 128 (a lane = one 32-element block)");
  constexpr int ESZ = KV8 ? 1 : 2;      // bytes per stored K/V element
  constexpr int ROWB = KV6 ? 3 * D / 4 : (KV4 ? D / 2 : D * ESZ);      // bytes per stored K/V row
  constexpr int VROWB = V4 ? D / 2 : ROWB;     // ... of a V row where the planes differ
  constexpr bool PADDED = LIVE != LPR;      // head_dim 96: lanes sub >= LIVE of a lane group are idle (zero pieces, no loads / stores)
  constexpr int kNW = NW;
  static_assert(!(PHYS && (ROPE || SLOT_LDS)), "physical-order streaming: plain keys, global slot map");
  static_assert((KU == 4 || KU == 8 || KU == 16) && (!PHYS || KU <= 8), "4, 8 or 16 rows per lane group; the dead-row mask is one byte per 8 rows");
  // head_dim 256 (LPR = 32: two rows per wave-load, the group sums cross the DPP row boundary): 16-bit rows with plain keys only
  static_assert(LPR <= 16 || (EPL == 8 && FMT == 0 && !ROPE && !RES), "lane groups of 32: 16-bit rows, plain keys");
  static_assert(LIVE <= LPR && LPR * Gm::G == 64, "one 16-byte piece per lane, whole rows per wave-load");
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int sub = lane % LPR, grp = lane / LPR;
  const int t_new = a.n_slots - 1;  // the appended position
#if EKV_WINDOW
  // Sliding windows (ekv_common.h).  The KU rows of a lane group's iteration are scored by all of its lanes, so lane `sub` reads the token
  // position of ONE of them, row sub % KU, behind the iteration's K/V requests (physical order: KU consecutive words per group; through
  // the slot map: the row index is in a register already), tests it against the query's position, and one ballot per wave hands every
  // group the mask bits of its rows.  A masked row's logit is -inf where it is formed: the online softmax gives it p = 0, its V row (a
  // live row: finite) adds nothing, and the logit export writes the -inf, so the tails, which tell dead rows from live ones by the
  // dead-row bits or the slot map and never by the logit, see a live column of probability 0.  The appended row is the query's own
  // position and never masked; the lane that stores it stamps its token position (the row does not move until it is evicted).
  static_assert(LPR >= KU && (KU & (KU - 1)) == 0 && EPL == 8 && FMT == 0 && !ROPE && !RES, "window instances: 16-bit rows, plain keys, no resident rows");
  const int win_w = win.windows[a.layer_begin + ll];
#endif
  int t1 = t1_in;
  const bool live_lane = !PADDED || sub < LIVE;
  // GQA factors that are not a power of two (or, in the split kernel, groups of <= 8 query heads of a wider factor): REP is the
  // padded count, `nrep` the query heads this workgroup really serves, from head `q_head0`; the padding heads r >= nrep repeat the
  // last real one (their logits / partials / outputs are never written out)
  const int nrep = n_rep_real > 0 ? n_rep_real : REP;
  const int hq0 = q_head0 >= 0 ? q_head0 : h * REP;

  uint4 qv[REP], qv1[REP];      // (qv1: FP8 rows, query elements 8..15 of the lane's 16)
  uint4 qx[KV4 ? REP : 1][4];      // (MXFP4 rows: the lane's 32 query elements)
  float qf[REP][8];  // ROPE: rotated query q' (fp32)
#pragma unroll
  for (int r = 0; r < REP; ++r) {
    const __half* qp = a.q + ((size_t)ll * a.n_q_heads + hq0 + min(r, nrep - 1)) * D;
    qv[r] = live_lane ? reinterpret_cast<const uint4*>(qp)[sub * (EPL / 8)] : uint4{0, 0, 0, 0};
    qv1[r] = KV8 ? reinterpret_cast<const uint4*>(qp)[sub * 2 + 1] : uint4{0, 0, 0, 0};
    if constexpr (KV4) {
#pragma unroll
      for (int i = 0; i < 4; ++i) qx[r][i] = reinterpret_cast<const uint4*>(qp)[sub * 4 + i];
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) qf[r][i] = 0.f;
    if (ROPE && live_lane) {
      // q' = q*cos[T-1] + rotate_half(q)*sin[T-1]   (llama_patch.py:311, :326)
      const int half_d = D / 2;
      const float* c = a.rope_cos + (size_t)t_new * D;
      const float* s = a.rope_sin + (size_t)t_new * D;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int d = sub * 8 + i;
        const int dp = d < half_d ? d + half_d : d - half_d;
        const float x = __half2float(qp[d]), y = __half2float(qp[dp]);
        qf[r][i] = x * c[d] + (d < half_d ? -y : y) * s[d];
      }
    }
  }

  // RoPE-on-read: keys are cached un-rotated and rotated by their SLOT index j at read time (llama_patch.py:312, :327):
  // k'[d] = k[d]*cos[j][d] + rotate_half(k)[d]*sin[j][d]; the partner k[d +- D/2] sits in lane sub ^ LPR/2 of the row's lane
  // group.  The row is rotated ONCE (fp32) and then dotted with each of the REP rotated queries.
  //
  // Where cos / sin come from (round 6).  A lane group walks KU CONSECUTIVE positions per iteration.  The tables are a rotation that is
  // linear in the position — row j = (cos(j*theta_f), sin(j*theta_f)), include/easykv_hip.h — so only the FIRST row of an iteration
  // is read from the table (the seed: exact table values) and the following KU - 1 rows advance the lane's 8 (cos, sin) pairs by the
  // angle-addition recurrence with the step constants (cos theta_f, sin theta_f) = table row 1, held in registers: 4 flops per pair
  // and step, a drift of a few fp32 roundings (< 1e-6 after 7 steps) before the next seed.  Before, every row loaded 64 B of fp32
  // table per lane — 512 B of table per 256-B key row through the vector-memory path, and 16 table registers per row IN FLIGHT next
  // to the K / V registers, which is what held the Llama-shape build at 4 rows in flight (25 of the 33 us over the plain stream:
  // profiles/r05 mocks).  The sine is kept pre-multiplied by the half's sign (-1 for d < D/2): (c, s~) obeys the same recurrence with
  // the step constant s~1, and the rotation is one fma + one multiply per element.  -DEKV_ROPE_EXACT=1 reads every row from the table;
  // so does the GQA x 8 build, whose eight fp32 queries leave no room for the 16 step registers (8 spilled VGPRs: 143 vs 135 us at
  // Hq = 64 / H = 8, measured).  Measured, Llama2-7B shape, budget 2048, same box: 219.3 us (round 5) / 225.5 (this code, every row from
  // the table) -> 198.6 us with the recurrence; plain keys 185.6; Mistral shape 95.0 -> 88.3.
#ifndef EKV_ROPE_EXACT
#define EKV_ROPE_EXACT 0
#endif
  constexpr bool kRopeExact = EKV_ROPE_EXACT || REP == 8;
  const float sgn = (sub < LIVE / 2) ? -1.f : 1.f;
  const int tab_off = (sub % (LIVE / 2)) * 8;      // cat(freqs, freqs): both halves of the lane group read the FIRST half of a row
  auto rope_seed = [&](int j, ekv_f2 (&cc)[4], ekv_f2 (&ss)[4]) {
#if EKV_ROPE_MOCK == 1      // (mock: no table loads — opaque constants, same arithmetic)
    float one = 1.f, zero = 0.25f;
    asm volatile("" : "+v"(one), "+v"(zero));
#pragma unroll
    for (int i = 0; i < 4; ++i) cc[i] = ekv_f2{one, one}, ss[i] = ekv_f2{zero, zero};
    (void)j;
#else
    const float4* c4 = reinterpret_cast<const float4*>(a.rope_cos + (size_t)j * D + tab_off);
    const float4* s4 = reinterpret_cast<const float4*>(a.rope_sin + (size_t)j * D + tab_off);
    const float4 c0 = c4[0], c1 = c4[1], s0 = s4[0], s1 = s4[1];
    cc[0] = ekv_f2{c0.x, c0.y}, cc[1] = ekv_f2{c0.z, c0.w}, cc[2] = ekv_f2{c1.x, c1.y}, cc[3] = ekv_f2{c1.z, c1.w};
    ss[0] = ekv_f2{s0.x, s0.y} * sgn, ss[1] = ekv_f2{s0.z, s0.w} * sgn, ss[2] = ekv_f2{s1.x, s1.y} * sgn, ss[3] = ekv_f2{s1.z, s1.w} * sgn;
#endif
  };
  ekv_f2 stp_c[4], stp_s[4];      // (cos theta_f, sgn * sin theta_f) of this lane's 8 frequencies
  if (ROPE && !kRopeExact) rope_seed(min(1, a.n_slots - 1), stp_c, stp_s);
  auto rope_advance = [&](ekv_f2 (&cc)[4], ekv_f2 (&ss)[4]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const ekv_f2 cn = __builtin_elementwise_fma(cc[i], stp_c[i], -(ss[i] * stp_s[i]));
      ss[i] = __builtin_elementwise_fma(ss[i], stp_c[i], cc[i] * stp_s[i]);
      cc[i] = cn;
    }
  };
  auto rope_rotate = [&](const uint4& kv, const ekv_f2 (&cc)[4], const ekv_f2 (&ss)[4], float (&kp)[8]) {
    uint4 other;
#if EKV_ROPE_MOCK == 2      // (mock: no partner exchange)
    other = kv;
#else
    if (PADDED) {      // the partner piece d +- D/2 is LIVE/2 lanes away, not an xor pattern: ds_bpermute
      const int src = (lane & ~(LPR - 1)) | (sub < LIVE / 2 ? sub + LIVE / 2 : (sub < LIVE ? sub - LIVE / 2 : sub));
      other.x = __shfl(kv.x, src, 64);
      other.y = __shfl(kv.y, src, 64);
      other.z = __shfl(kv.z, src, 64);
      other.w = __shfl(kv.w, src, 64);
    } else {
      other.x = __shfl_xor(kv.x, LPR / 2, 64);
      other.y = __shfl_xor(kv.y, LPR / 2, 64);
      other.z = __shfl_xor(kv.z, LPR / 2, 64);
      other.w = __shfl_xor(kv.w, LPR / 2, 64);
    }
#endif
    const ekv_h8 kh = __builtin_bit_cast(ekv_h8, kv), oh = __builtin_bit_cast(ekv_h8, other);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const ekv_f2 k2 = {(float)kh[2 * i], (float)kh[2 * i + 1]}, o2 = {(float)oh[2 * i], (float)oh[2 * i + 1]};
      const ekv_f2 r2 = __builtin_elementwise_fma(k2, cc[i], o2 * ss[i]);
      kp[2 * i] = r2[0];
      kp[2 * i + 1] = r2[1];
    }
  };

  const __half* k_new_row = a.k_new + ((size_t)ll * a.n_kv_heads + h) * D;
  const __half* v_new_row = a.v_new + ((size_t)ll * a.n_kv_heads + h) * D;
  const int slot_base = SLOT_LDS ? t0 : 0;   // index origin of s_slot
#pragma unroll
  for (int r = 0; r < REP; ++r) {
    m[r] = EKV_NEG_INF;
    l[r] = 0.f;
#pragma unroll
    for (int i = 0; i < EPL; ++i) o[r][i] = 0.f;
  }

  // The appended row is peeled off the loop: its K/V come from k_new / v_new and one lane group appends and scores it AFTER
  // the loop (below) — doing that first cost wave 0 three dependent round trips (slot index, k_new, v_new -> store) before
  // its first K/V load, while the other waves were already streaming.  The loop covers [t0, t_new): with T = budget + 1 =
  // 2049 that is exactly 16 full iterations instead of 17.
  const bool has_new = t_new >= t0 && t_new < t1;
  if (has_new) t1 = t_new;
  auto appended_row = [&]() {
    if (!(has_new && wave == 0 && grp == 0)) return;
    const int slot_new = s_slot[t_new - slot_base];
    uint4 kn = uint4{0, 0, 0, 0}, vn = uint4{0, 0, 0, 0};
    const size_t off = (head_row + slot_new) * D;          // append: the new row goes into the recycled slot
    float ksn = 1.f, vsn = 1.f;      // FP8 rows: the new row's scales
    ekv_u6 kn6 = {0, 0, 0, 0, 0, 0}, vn6 = {0, 0, 0, 0, 0, 0};      // MXFP6 rows: the new row's blocks
    if constexpr (KV6) {
      // quantise the new row (rule: include/easykv_hip.h): each lane's 32 elements are one block — 24 bytes of codes + one exponent byte
      uint32_t ke, ve;
      kn6 = ekv_fp6_quant_block(reinterpret_cast<const uint4*>(k_new_row) + sub * 4, ke);
      vn6 = ekv_fp6_quant_block(reinterpret_cast<const uint4*>(v_new_row) + sub * 4, ve);
      ksn = ekv_fp4_exp_scale(ke), vsn = ekv_fp4_exp_scale(ve);
      ekv_fp6_store_block(reinterpret_cast<char*>(a.k_w) + (head_row + slot_new) * ROWB, sub, kn6);
      ekv_fp6_store_block(reinterpret_cast<char*>(a.v_w) + (head_row + slot_new) * ROWB, sub, vn6);
      a.k_exp[(head_row + slot_new) * 4 + sub] = (uint8_t)ke;
      a.v_exp[(head_row + slot_new) * 4 + sub] = (uint8_t)ve;
    } else if constexpr (KV8) {
      // quantise the new row (rule: include/easykv_hip.h): row maximum over the lane group, then 16 codes per lane + one scale
      float kf[16], vf[16];
      const uint4* kq = reinterpret_cast<const uint4*>(k_new_row) + sub * 2;
      const uint4* vq = reinterpret_cast<const uint4*>(v_new_row) + sub * 2;
      float ka = fmaxf(ekv_widen8_amax(kq[0], kf), ekv_widen8_amax(kq[1], kf + 8));
      float va = fmaxf(ekv_widen8_amax(vq[0], vf), ekv_widen8_amax(vq[1], vf + 8));
      ksn = ekv_fp8_row_scale(ekv_group_max<LPR>(ka));
      uint32_t ve = 127u;      // KV84: the exponent byte of the lane pair's V block (the MXFP4 rule over the pair's maximum)
      if constexpr (KV84) ve = ekv_fp4_block_exp(fmaxf(va, ekv_dpp<0xB1>(va))), vsn = ekv_fp4_exp_scale(ve);
      else vsn = ekv_fp8_row_scale(ekv_group_max<LPR>(va));
      kn = uint4{ekv_fp8_quant4(kf[0], kf[1], kf[2], kf[3], ksn), ekv_fp8_quant4(kf[4], kf[5], kf[6], kf[7], ksn),
                 ekv_fp8_quant4(kf[8], kf[9], kf[10], kf[11], ksn), ekv_fp8_quant4(kf[12], kf[13], kf[14], kf[15], ksn)};
      if constexpr (KV84)
        vn = uint4{ekv_fp4_quant8(vf, vsn), ekv_fp4_quant8(vf + 8, vsn), 0, 0};      // (the lane's 16 codes: half a block)
      else
        vn = uint4{ekv_fp8_quant4(vf[0], vf[1], vf[2], vf[3], vsn), ekv_fp8_quant4(vf[4], vf[5], vf[6], vf[7], vsn),
                   ekv_fp8_quant4(vf[8], vf[9], vf[10], vf[11], vsn), ekv_fp8_quant4(vf[12], vf[13], vf[14], vf[15], vsn)};
      reinterpret_cast<uint4*>(reinterpret_cast<uint8_t*>(a.k_w) + off)[sub] = kn;
      if constexpr (KV84) {
        reinterpret_cast<uint2*>(reinterpret_cast<uint8_t*>(a.v_w) + off / 2)[sub] = uint2{vn.x, vn.y};
        if (!(sub & 1)) a.v_exp[(head_row + slot_new) * 4 + (sub >> 1)] = (uint8_t)ve;
      } else {
        reinterpret_cast<uint4*>(reinterpret_cast<uint8_t*>(a.v_w) + off)[sub] = vn;
      }
      if (sub == 0) {
        a.k_scale[head_row + slot_new] = ksn;
        if constexpr (!KV84) a.v_scale[head_row + slot_new] = vsn;
      }
    } else if constexpr (KV4) {
      // quantise the new row (rule: include/easykv_hip.h): each lane's 32 elements are one block — 16 bytes of codes + one exponent byte
      uint32_t ke, ve;
      kn = ekv_fp4_quant_block(reinterpret_cast<const uint4*>(k_new_row) + sub * 4, ke);
      vn = ekv_fp4_quant_block(reinterpret_cast<const uint4*>(v_new_row) + sub * 4, ve);
      ksn = ekv_fp4_exp_scale(ke), vsn = ekv_fp4_exp_scale(ve);
      reinterpret_cast<uint4*>(reinterpret_cast<uint8_t*>(a.k_w) + off / 2)[sub] = kn;
      reinterpret_cast<uint4*>(reinterpret_cast<uint8_t*>(a.v_w) + off / 2)[sub] = vn;
      a.k_exp[(head_row + slot_new) * 4 + sub] = (uint8_t)ke;
      a.v_exp[(head_row + slot_new) * 4 + sub] = (uint8_t)ve;
    } else if constexpr (KV164) {
      // K: stored as the 16-bit step stores it.  V: quantised by the MXFP4 rule (include/easykv_hip.h) — the block maximum over the lane
      // quad (two DPP quad_perms), 8 codes per lane (4 bytes at byte 4 * sub of the 64-byte row), one exponent byte per quad
      kn = reinterpret_cast<const uint4*>(k_new_row)[sub];
      reinterpret_cast<uint4*>(a.k_w + off)[sub] = kn;
      float vf[8];
      float va = ekv_widen8_amax(reinterpret_cast<const uint4*>(v_new_row)[sub], vf);
      va = fmaxf(va, ekv_dpp<0xB1>(va));
      va = fmaxf(va, ekv_dpp<0x4E>(va));
      const uint32_t ve = ekv_fp4_block_exp(va);
      vsn = ekv_fp4_exp_scale(ve);
      vn.x = ekv_fp4_quant8(vf, vsn);
      reinterpret_cast<uint32_t*>(reinterpret_cast<uint8_t*>(a.v_w) + off / 2)[sub] = vn.x;
      if (!(sub & 3)) a.v_exp[(head_row + slot_new) * 4 + (sub >> 2)] = (uint8_t)ve;
    } else if (live_lane) {
      kn = reinterpret_cast<const uint4*>(k_new_row)[sub];
      vn = reinterpret_cast<const uint4*>(v_new_row)[sub];
      reinterpret_cast<uint4*>(a.k_w + off)[sub] = kn;
      reinterpret_cast<uint4*>(a.v_w + off)[sub] = vn;
    }
#if EKV_WINDOW
    if (sub == 0) win.tok_pos[head_row + slot_new] = win.q_pos0;
#endif
    float kpn[8];
    if (ROPE) {
      ekv_f2 cn[4], sn[4];
      rope_seed(t_new, cn, sn);
      rope_rotate(kn, cn, sn, kpn);
    }
#pragma unroll
    for (int r = 0; r < REP; ++r) {
      float acc;
      if (ROPE) {
        acc = 0.f;
#pragma unroll
        for (int i = 0; i < 8; ++i) acc = fmaf(kpn[i], qf[r][i], acc);
      } else if constexpr (KV8) {
        acc = ekv_dot16_fp8(qv[r], qv1[r], kn, 0.f);
      } else if constexpr (KV6) {
        acc = ekv_dot32_fp6(qx[r], kn6, 0.f) * ksn;      // (this lane's block scale, before the group sum)
      } else if constexpr (KV4) {
        acc = ekv_dot32_fp4(qx[r], kn, 0.f) * ksn;      // (this lane's block scale, before the group sum)
      } else {
        acc = ekv_dot8(qv[r], kn, 0.f);
      }
      acc = KV8 ? ekv_group_sum<LPR>(acc) * ksn / a.sm_div : EKV_LOGIT(ekv_group_sum<LPR>(acc), a);
      if (logit_out != nullptr && sub == 0 && r < nrep) logit_out[(size_t)r * logit_stride + (PHYS ? slot_new : t_new)] = acc;
      // one more row for this lane group's online softmax
      const float mn = fmaxf(m[r], acc);
      const float alpha = m[r] == EKV_NEG_INF ? 0.f : exp2f((m[r] - mn) * EKV_LOG2E);
      const float p = exp2f((acc - mn) * EKV_LOG2E);
      l[r] = l[r] * alpha + p;
#pragma unroll
      for (int i = 0; i < EPL; ++i) o[r][i] *= alpha;
      if constexpr (KV84) ekv_axpy16_fp4(p, vsn, uint2{vn.x, vn.y}, o[r]);
      else if constexpr (KV8) ekv_axpy16_fp8(p * vsn, vn, o[r]);
      else if constexpr (KV6) ekv_axpy32_fp6(p, vsn, vn6, o[r]);
      else if constexpr (KV4) ekv_axpy32_fp4(p, vsn, vn, o[r]);
      else if constexpr (KV164) ekv_axpy8_fp4(p, vsn, vn.x, o[r]);
      else ekv_axpy8(p, vn, o[r]);
      m[r] = mn;
#if EKV_SINK
      // the sink of query head r: a virtual key with value 0, counted here and nowhere else in the launch — this lane group of the one
      // workgroup whose key range holds the appended row
      ekv_sink_fold(sink_row[hq0 + min(r, nrep - 1)], m[r], l[r], o[r]);
#endif
    }
  };
  if (!PHYS && t1 <= t0) {   // the split held only the appended row
    appended_row();
    return;
  }

  if (PHYS) t1 = a.phys_extent;   // loop bound: physical rows [0, E); which of them count is s_dead's business
  const int last_slot = PHYS ? 0 : s_slot[t1 - 1 - slot_base];
  const int idx_cap = (a.cap - KU) & ~(KU - 1);   // prefetches past t1 stay inside the head's map row (values unused); a multiple of KU like j0
  uint4 iv[KU / 4];                        // !SLOT_LDS: slot indices of rows j0..j0+KU-1 of the next iteration
#pragma unroll
  for (int i = 0; i < KU / 4; ++i) iv[i] = uint4{0, 0, 0, 0};
  if (!PHYS && !SLOT_LDS && t0 + wave * RW < t1) {
    const uint4* ip = reinterpret_cast<const uint4*>(s_slot + min(t0 + wave * RW + grp * KU, idx_cap));
#pragma unroll
    for (int i = 0; i < KU / 4; ++i) iv[i] = ip[i];
  }
  auto iteration = [&](const int base, auto&& after_issue) {
    uint4 kr[KU], vr[KU];
    ekv_u6 kr6[KV6 ? KU : 1], vr6[KV6 ? KU : 1];      // MXFP6 rows: the lane's block of each row (kr / vr stay unused)
    float ksc[KV8 || KV4 ? KU : 1], vsc[KV8 || KV4 || KV164 ? KU : 1];     // FP8 rows: the scales of the KU rows; MXFP4 rows: of this lane's block of each
    const int j0 = base + grp * KU;
    if constexpr (KV8 && PHYS) {
      // consecutive physical rows: KU / 4 16-byte loads per plane (fused step: cap % 4 == 0, so head_row + j0 is 16-byte aligned); a
      // group whose rows would run past the head's scale row reads them one by one (clamped; those rows are dead anyway)
      if (j0 + KU <= a.cap) {
        const float4* k4 = reinterpret_cast<const float4*>(a.k_scale + head_row + j0);
        const float4* v4 = reinterpret_cast<const float4*>(a.v_scale + head_row + j0);
#pragma unroll
        for (int i = 0; i < KU / 4; ++i) {
          const float4 kk = k4[i], vv = KV84 ? float4{1.f, 1.f, 1.f, 1.f} : v4[i];      // (KV84: a.v_scale is a.v_exp — below)
          ksc[4 * i] = kk.x, ksc[4 * i + 1] = kk.y, ksc[4 * i + 2] = kk.z, ksc[4 * i + 3] = kk.w;
          vsc[4 * i] = vv.x, vsc[4 * i + 1] = vv.y, vsc[4 * i + 2] = vv.z, vsc[4 * i + 3] = vv.w;
        }
      } else {
#pragma unroll
        for (int u = 0; u < KU; ++u) {
          ksc[u] = a.k_scale[head_row + min(j0 + u, a.cap - 1)];
          vsc[u] = KV84 ? 1.f : a.v_scale[head_row + min(j0 + u, a.cap - 1)];
        }
      }
    }
    if constexpr (V4 && PHYS) {
      // the V exponent words of the KU consecutive rows, as the MXFP4 stream reads them (same bound); lane `sub` holds half of block
      // sub >> 1 (16-bit keys: a quarter of block sub >> 2)
      uint32_t vw[KU];
      if (j0 + KU <= a.cap) {
        const uint4* v4 = reinterpret_cast<const uint4*>(a.v_exp + (head_row + j0) * 4);
#pragma unroll
        for (int i = 0; i < KU / 4; ++i) {
          const uint4 vv = v4[i];
          vw[4 * i] = vv.x, vw[4 * i + 1] = vv.y, vw[4 * i + 2] = vv.z, vw[4 * i + 3] = vv.w;
        }
      } else {
#pragma unroll
        for (int u = 0; u < KU; ++u) vw[u] = reinterpret_cast<const uint32_t*>(a.v_exp)[head_row + min(j0 + u, a.cap - 1)];
      }
#pragma unroll
      for (int u = 0; u < KU; ++u) vsc[u] = ekv_fp4_exp_scale((vw[u] >> (8 * (sub >> VSH))) & 0xFFu);
    }
    if constexpr (KV4 && PHYS) {
      // consecutive physical rows: their exponent words (4 bytes per row) as KU / 4 16-byte loads per plane, under the bound of the FP8
      // scales above; lane `sub` of a row's group keeps byte `sub`, its own block's
      uint32_t kw[KU], vw[KU];
      if (j0 + KU <= a.cap) {
        const uint4* k4 = reinterpret_cast<const uint4*>(a.k_exp + (head_row + j0) * 4);
        const uint4* v4 = reinterpret_cast<const uint4*>(a.v_exp + (head_row + j0) * 4);
#pragma unroll
        for (int i = 0; i < KU / 4; ++i) {
          const uint4 kk = k4[i], vv = v4[i];
          kw[4 * i] = kk.x, kw[4 * i + 1] = kk.y, kw[4 * i + 2] = kk.z, kw[4 * i + 3] = kk.w;
          vw[4 * i] = vv.x, vw[4 * i + 1] = vv.y, vw[4 * i + 2] = vv.z, vw[4 * i + 3] = vv.w;
        }
      } else {
#pragma unroll
        for (int u = 0; u < KU; ++u) {
          kw[u] = reinterpret_cast<const uint32_t*>(a.k_exp)[head_row + min(j0 + u, a.cap - 1)];
          vw[u] = reinterpret_cast<const uint32_t*>(a.v_exp)[head_row + min(j0 + u, a.cap - 1)];
        }
      }
#pragma unroll
      for (int u = 0; u < KU; ++u) {
        ksc[u] = ekv_fp4_exp_scale((kw[u] >> (8 * sub)) & 0xFFu);
        vsc[u] = ekv_fp4_exp_scale((vw[u] >> (8 * sub)) & 0xFFu);
      }
    }
    EKV_WIN_ONLY(int win_tp = 0;)
    int cur[KU];
#pragma unroll
    for (int i = 0; i < KU / 4; ++i) {
      cur[4 * i] = (int)iv[i].x;
      cur[4 * i + 1] = (int)iv[i].y;
      cur[4 * i + 2] = (int)iv[i].z;
      cur[4 * i + 3] = (int)iv[i].w;
    }
    if (!PHYS && !SLOT_LDS && base + kNW * RW < t1) {     // next iteration's indices (the map row has >= t_pad entries)
      const uint4* ip = reinterpret_cast<const uint4*>(s_slot + min(j0 + kNW * RW, idx_cap));
#pragma unroll
      for (int i = 0; i < KU / 4; ++i) iv[i] = ip[i];
    }
    if constexpr (RES) {
      // the iteration's K/V requests under one load policy, twice (see the head of this function).  The row index is opaque inside each
      // copy, so that every address is formed next to its load as in the single-policy code: hoisted above the branch, the 2 * KU
      // addresses are live at once and cost the occupancy the kernel is built for
      auto request = [&](auto resident) {
        int jr = j0;
        asm volatile("" : "+v"(jr));
#pragma unroll
        for (int u = 0; u < KU; ++u) {
          const int row = jr + u < t1 ? jr + u : t1 - 1;
          kr[u] = ekv_load_row_piece<decltype(resident)::value>(reinterpret_cast<const char*>(a.k) + (head_row + row) * ROWB, sub);
          vr[u] = ekv_load_row_piece<decltype(resident)::value>(reinterpret_cast<const char*>(a.v) + (head_row + row) * ROWB, sub);
        }
      };
      if (base < res_rows) request(EkvBool<true>());
      else request(EkvBool<false>());
    } else {
    EKV_WIN_ONLY(int win_row = 0;)      // (the physical row whose token position this lane reads)
#pragma unroll
    for (int u = 0; u < KU; ++u) {
      const int j = j0 + u;
      const int jj = j < t1 ? j : t1 - 1;
      const int row = PHYS ? jj : (SLOT_LDS ? s_slot[jj - t0] : (j < t1 ? cur[u] : last_slot));
      EKV_WIN_ONLY(win_row = (sub & (KU - 1)) == u ? row : win_row;)
      const char* kp = reinterpret_cast<const char*>(a.k) + (head_row + row) * ROWB;
      const char* vp = reinterpret_cast<const char*>(a.v) + (head_row + row) * VROWB;
      if constexpr (KV8 && !PHYS) {      // rows through the slot map: one scale per row (the lanes of a group read the same word)
        ksc[u] = a.k_scale[head_row + row];
        if constexpr (KV84) vsc[u] = ekv_fp4_exp_scale(a.v_exp[(head_row + row) * 4 + (sub >> 1)]);
        else vsc[u] = a.v_scale[head_row + row];
      }
      if constexpr (KV4 && !PHYS) {      // rows through the slot map: this lane's exponent byte of each row
        ksc[u] = ekv_fp4_exp_scale(a.k_exp[(head_row + row) * 4 + sub]);
        vsc[u] = ekv_fp4_exp_scale(a.v_exp[(head_row + row) * 4 + sub]);
      }
      // a row is read once per step: non-temporal loads (the load policy: the head of this function)
      if constexpr (KV6) {
        kr6[u] = ekv_fp6_load_block(kp, sub);
        vr6[u] = ekv_fp6_load_block(vp, sub);
      } else if constexpr (KV84) {      // 16 K codes, and the 8 bytes (16 codes) of the V row at byte 8 * sub
        kr[u] = __builtin_bit_cast(uint4, __builtin_nontemporal_load(reinterpret_cast<const ekv_u4*>(kp) + sub));
        const ekv_u2 w = __builtin_nontemporal_load(reinterpret_cast<const ekv_u2*>(vp) + sub);
        vr[u] = uint4{w[0], w[1], 0, 0};
      } else if constexpr (KV164) {      // the 16-bit K piece as always, and the 4 bytes (8 codes) of the V row at byte 4 * sub
        if constexpr (!PHYS) vsc[u] = ekv_fp4_exp_scale(a.v_exp[(head_row + row) * 4 + (sub >> 2)]);      // (through the slot map: one byte per row)
        kr[u] = __builtin_bit_cast(uint4, __builtin_nontemporal_load(reinterpret_cast<const ekv_u4*>(kp) + sub));
        vr[u] = uint4{__builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(vp) + sub), 0, 0, 0};
      } else if (live_lane) {
        kr[u] = __builtin_bit_cast(uint4, __builtin_nontemporal_load(reinterpret_cast<const ekv_u4*>(kp) + sub));
        vr[u] = __builtin_bit_cast(uint4, __builtin_nontemporal_load(reinterpret_cast<const ekv_u4*>(vp) + sub));
      } else {
        kr[u] = vr[u] = uint4{0, 0, 0, 0};
      }
    }
    EKV_WIN_ONLY(win_tp = win.tok_pos[head_row + win_row];)      // (a row inside the head's map row, live or not: always readable)
    }
    ekv_f2 rc[4], rs[4];      // ROPE: (cos, signed sin) of row j0 for this lane's 8 frequencies — the seed, read with the K / V rows
    if (ROPE) rope_seed(min(j0, t1 - 1), rc, rs);
    after_issue();
    // PHYS: bit u of dead8 = row j0+u is free / being appended / past the extent (j0 is a multiple of 8: one mask byte)
    const unsigned dead8 = PHYS ? (KU == 4 ? ((unsigned)s_dead[j0 >> 3] >> (j0 & 4)) & 0xFu : (unsigned)s_dead[j0 >> 3]) : 0u;
    if (PHYS && dead8 != 0u) {   // rare: a dead row may hold anything (0 * inf = NaN in the PV accumulation)
#pragma unroll
      for (int u = 0; u < KU; ++u)
        if ((dead8 >> u) & 1u) {
          vr[u] = uint4{0, 0, 0, 0};
          if constexpr (KV6) vr6[u] = ekv_u6{0, 0, 0, 0, 0, 0};
          if constexpr (KV8) vsc[u] = KV84 ? 1.f : 0.f;      // (KV84: zero codes under scale 1, as MXFP4)
          if constexpr (KV4 || KV164) vsc[u] = 1.f;      // (zero codes under a finite scale)
        }
    }
#if EKV_WINDOW
    // bit u of win8 = row j0 + u is window-masked (bits of dead or out-of-range rows mean nothing: those are -inf already)
    const unsigned win8 = (unsigned)(__ballot(ekv_win_masked(win.q_pos0, win_tp, win_w)) >> (grp * LPR)) & ((1u << KU) - 1u);
#endif
    float sall[ROPE ? REP : 1][KU];   // ROPE: every row is rotated once, then dotted with all REP queries
    if (ROPE) {
#pragma unroll
      for (int u = 0; u < KU; ++u) {
        float kp[8];
        rope_rotate(kr[u], rc, rs, kp);
        if (u + 1 < KU) {      // (cos, sin) of the next position
          if (kRopeExact) rope_seed(min(j0 + u + 1, t1 - 1), rc, rs);
          else rope_advance(rc, rs);
        }
#pragma unroll
        for (int r = 0; r < REP; ++r) {
          float acc = 0.f;
#pragma unroll
          for (int i = 0; i < 8; ++i) acc = fmaf(kp[i], qf[r][i], acc);
          acc = ekv_group_sum<LPR>(acc);
          sall[r][u] = (j0 + u < t1) ? acc / a.sm_div : EKV_NEG_INF;
        }
      }
    }
#pragma unroll
    for (int r = 0; r < REP; ++r) {
      float s[KU];
#pragma unroll
      for (int u = 0; u < KU; ++u) {
        if (ROPE) {
          s[u] = sall[r][u];
        } else {
          float acc;
          if constexpr (KV6) acc = ekv_dot32_fp6(qx[r], kr6[u], 0.f) * ksc[u];
          else if constexpr (KV4) acc = ekv_dot32_fp4(qx[r], kr[u], 0.f) * ksc[u];      // (the lane's block scale, before the group sum)
          else acc = KV8 ? ekv_dot16_fp8(qv[r], qv1[r], kr[u], 0.f) : ekv_dot8(qv[r], kr[u], 0.f);
          acc = ekv_group_sum<LPR>(acc);
          if constexpr (KV8) acc *= ksc[u];
          s[u] = ((PHYS ? !((dead8 >> u) & 1u) : (j0 + u < t1)) EKV_WIN_ONLY(&& !((win8 >> u) & 1u))) ? EKV_LOGIT(acc, a) : EKV_NEG_INF;
        }
      }
      // export the raw logits: lane `sub` of the group owns row j0+sub -> 8 consecutive floats per group
      // (D = 32 has only 4 lanes per row: each lane then owns rows sub and sub + 4)
      constexpr int NST = (KU + LPR - 1) / LPR;
#pragma unroll
      for (int st = 0; st < NST; ++st) {
        const int mu = sub + st * LPR;
        float mine = s[0];
#pragma unroll
        for (int u = 1; u < KU; ++u) mine = (mu == u) ? s[u] : mine;
        if (logit_out != nullptr && mu < KU && r < nrep && (PHYS ? !((dead8 >> mu) & 1u) : (j0 + mu < t1)))
          logit_out[(size_t)r * logit_stride + j0 + mu] = mine;
      }
      float mx = s[0];
#pragma unroll
      for (int u = 1; u < KU; ++u) mx = fmaxf(mx, s[u]);
      const float mn = fmaxf(m[r], mx);
      if (mn == EKV_NEG_INF) continue;  // whole group out of range
      const float alpha = exp2f((m[r] - mn) * EKV_LOG2E);
      l[r] *= alpha;
#pragma unroll
      for (int i = 0; i < EPL; ++i) o[r][i] *= alpha;
#pragma unroll
      for (int u = 0; u < KU; ++u) {
        const float p = exp2f((s[u] - mn) * EKV_LOG2E);
        l[r] += p;
        if constexpr (KV84) ekv_axpy16_fp4(p, vsc[u], uint2{vr[u].x, vr[u].y}, o[r]);
        else if constexpr (KV8) ekv_axpy16_fp8(p * vsc[u], vr[u], o[r]);
        else if constexpr (KV6) ekv_axpy32_fp6(p, vsc[u], vr6[u], o[r]);
        else if constexpr (KV4) ekv_axpy32_fp4(p, vsc[u], vr[u], o[r]);
        else if constexpr (KV164) ekv_axpy8_fp4(p, vsc[u], vr[u].x, o[r]);
        else ekv_axpy8(p, vr[u], o[r]);
      }
      m[r] = mn;
    }
  };
  int base = t0 + wave * RW;
  if (PHYS) {
    if (t1 > (kNW - 1) * RW) {   // every wave has a first iteration: peel it around the mask completion
      iteration(base, mask_ready);
      base += kNW * RW;
    } else {
      mask_ready();
    }
  }
  for (; base < t1; base += kNW * RW) iteration(base, EkvNoop());
  appended_row();
}

// Combine the G lane groups of a wave (flash-decoding merge over lanes LPR, 2*LPR, ... apart); afterwards every lane
// holds the wave's (m, l, o) for its 8-wide slice of head_dim.
template <int D, int REP, int EPL = 8>
__device__ __forceinline__ void ekv_decode_wave_combine(float (&m)[REP], float (&l)[REP], float (&o)[REP][EPL]) {
  using Gm = EkvDecodeGeom<D, 4, kU, EPL>;
#pragma unroll
  for (int off = Gm::LPR; off < 64; off <<= 1) {
#pragma unroll
    for (int r = 0; r < REP; ++r) {
      const float mo = __shfl_xor(m[r], off, 64), lo = __shfl_xor(l[r], off, 64);
      const float mn = fmaxf(m[r], mo);
      const float wa = (m[r] == EKV_NEG_INF) ? 0.f : exp2f((m[r] - mn) * EKV_LOG2E);
      const float wb = (mo == EKV_NEG_INF) ? 0.f : exp2f((mo - mn) * EKV_LOG2E);
      l[r] = l[r] * wa + lo * wb;
#pragma unroll
      for (int i = 0; i < EPL; ++i) o[r][i] = o[r][i] * wa + __shfl_xor(o[r][i], off, 64) * wb;
      m[r] = mn;
    }
  }
}

// Wave partials -> LDS (call after ekv_decode_wave_combine, then __syncthreads(), then ekv_decode_reduce).
template <int D, int REP, int NW = 4, int EPL = 8>
__device__ __forceinline__ void ekv_decode_stash(float* s_part, const float (&m)[REP], const float (&l)[REP],
                                                 const float (&o)[REP][EPL]) {
  using Gm = EkvDecodeGeom<D, NW, kU, EPL>;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int sub = lane % Gm::LPR, grp = lane / Gm::LPR;
  if (grp != 0 || sub >= Gm::LIVE) return;
#pragma unroll
  for (int r = 0; r < REP; ++r) {
    float* p = s_part + ((size_t)wave * REP + r) * Gm::PS;
    if (sub == 0) {
      p[0] = m[r];
      p[1] = l[r];
    }
#pragma unroll
    for (int i = 0; i < EPL; ++i) p[2 + sub * EPL + i] = o[r][i];
  }
}

// Combined (max, sum, o[d]) of query head r over the workgroup's wave partials.
template <int D, int REP, int NW = 4>
__device__ __forceinline__ void ekv_decode_reduce(const float* s_part, int r, int d, float& mm, float& ls, float& os) {
  using Gm = EkvDecodeGeom<D, NW>;
  mm = EKV_NEG_INF;
#pragma unroll
  for (int i = 0; i < Gm::NP; ++i) mm = fmaxf(mm, s_part[((size_t)i * REP + r) * Gm::PS]);
  ls = 0.f;
  os = 0.f;
#pragma unroll
  for (int i = 0; i < Gm::NP; ++i) {
    const float* p = s_part + ((size_t)i * REP + r) * Gm::PS;
    const float w = (p[0] == EKV_NEG_INF) ? 0.f : exp2f((p[0] - mm) * EKV_LOG2E);
    ls += p[1] * w;
    os += p[2 + d] * w;
  }
}

// One plane (K or V) of the physical-order stream on its own, for the phase order that runs the scorer tail between the K rows and
// the V rows (ekv_attn_decode.inc, "order K").  Same row -> (wave, lane group, iteration) mapping as ekv_decode_stream with KU = 8:
// lane group `grp` of wave `wave` takes rows base + grp * 8 .. + 7 of every block of NW * 32 rows, 16 lanes x 16 B per row.  With
// one plane there are 8 loads per lane and iteration, so the NEXT iteration's rows are requested before the current ones are
// consumed (two register sets, the loop unrolled by two): 16 x 16 B in flight per lane, as in the fused loop.  Rows past t1 are
// clamped to t1 - 1 (requested and dropped; the dead-row bits decide what counts), so every request is unconditional and the
// waits the compiler places count requests, not paths.  `first` runs once per wave, behind the first requests (mask_ready).
// RES / res_rows: the load policy per block of RW rows, as in ekv_decode_stream; a block wholly past t1 (a request ahead of the loop's
// end: every row clamped to t1 - 1) takes the policy of that row's block.
template <int D, int NW, bool RES = false, typename First, typename Consume>
__device__ __forceinline__ void ekv_decode_plane_loop(const __half* plane, size_t head_row, int t1, First&& first, Consume&& consume, int res_rows = 0) {
  using Gm = EkvDecodeGeom<D, NW, 8, 8>;
  static_assert(Gm::LIVE == Gm::LPR, "whole lane groups");
  constexpr int RW = Gm::RW, STEP = NW * RW;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int sub = lane % Gm::LPR, grp = lane / Gm::LPR;
  auto request_as = [&](auto resident, uint4 (&r)[8], int base) {
    int j0 = base + grp * 8;
    if constexpr (RES) asm volatile("" : "+v"(j0));      // (opaque per copy: addresses formed next to their loads, see ekv_decode_stream)
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int row = j0 + u < t1 ? j0 + u : t1 - 1;
      const char* p = reinterpret_cast<const char*>(plane) + (head_row + row) * (D * 2);
      r[u] = ekv_load_row_piece<decltype(resident)::value>(p, sub);
    }
  };
  auto request = [&](uint4 (&r)[8], int base) {
    if constexpr (RES) {
      if (min(base, t1 - 1) < res_rows) request_as(EkvBool<true>(), r, base);
      else request_as(EkvBool<false>(), r, base);
    } else {
      request_as(EkvBool<false>(), r, base);
    }
  };
  uint4 ra[8], rb[8];
  int base = wave * RW;
  request(ra, base);
  first();
  while (base < t1) {
    request(rb, base + STEP);
    consume(ra, base + grp * 8);
    base += STEP;
    if (base >= t1) break;
    request(ra, base + STEP);
    consume(rb, base + grp * 8);
    base += STEP;
  }
}
