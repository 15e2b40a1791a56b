// Long-row scorer: the generic scorer (ekv_score_select.inc) for score rows of ANY width up to the bank's cap, in two launches.
//
// The generic scorer runs one workgroup per (head, layer) and keeps its selection keys in that CU's LDS, 4 B per column, which ends at
// about 38 400 columns.  Here nothing that scales with the width W lives in LDS:
//   ekv_long_sweep_kernel    grid (column tile, KV head, layer), 256 threads, four consecutive columns per thread.  Stage 2 of the generic
//                            scorer — load S (roco: Q, C), add this forward's folded probabilities (exponentials of the exported logits,
//                            or the column-sum partials of a two-pass chunk step), tova's last row — spread over the chip, plus the
//                            stage-1 selection key of every column.  Writes S' / Q' / C' to the `big_rows` scratch (the layout of the
//                            generic scorer's wide-row build) and the keys to a fourth scratch row per head.
//   ekv_long_select_kernel   grid (KV head, layer), 1024 threads.  Stages 3-6 of the generic scorer with the key array in that scratch
//                            (L2-resident; the workgroup's own barriers order its accesses, as they do for S / Q / C in the wide-row
//                            build): feasible set, mean keys, the k smallest, destinations by scan, compacted write-back, evict ids,
//                            slot-map compaction.  LDS: reduction scratch, the 264-word histogram, the candidate list.
//   ekv_long_fold_kernel     the fold of the key-range partials into the 16-bit output, for the steps whose generic scorer folds it
//                            itself (the planner puts it in front).  Element type at run time: one build serves fp16 and bf16 banks.
//
// Arithmetic contract (what makes every bit equal to the generic scorer's wherever both run).  Per column: queries i in order,
// pb = (sum over the rep query heads r, in order, of expf(x - M) * (1 / L)) / rep — divided only when rep > 1 —, colsum += pb,
// colsq += pb * pb; column-sum partials summed in part order 0, 1, 2, ...; -ffp-contract=off.  The row statistics (M, 1 / L) and the
// folded output come from ekv_fold_partials_auto with the batch width of the generic scorer's build the plain call would have run
// (FOLD16: its 512-thread build takes the partials 16 at a time, the other two 8 at a time; beyond 8 partials the two round differently).
// Selection: the k smallest (key, index) pairs, ties to the lowest index, NaN largest — ekv_blk_select.h, shared with the generic scorer.
// Every index is a 32-bit int below cap; offsets into the bank and the workspace are size_t.
#include "ekv_common.h"
#include "ekv_kernels.h"

#ifndef EKV_LONG_NT
#define EKV_LONG_NT 1024
#endif

namespace {

constexpr int kNT = EKV_LONG_NT;   // threads of the select workgroup (what ekv_blk_select.h strides by)
constexpr int kNWV = kNT / 64;
constexpr int kSW = kLongSweepNT;  // threads of a sweep workgroup
static_assert(kNT == kLongSelectNT, "the manifest line and ekv_geometry.h must name the same select workgroup");

#include "ekv_blk_select.h"

// Four consecutive floats of a row from column j4: one 16-byte load where the row start is 16-byte aligned (VEC; columns past W stay
// inside the row's t_pad pitch), else four clamped scalar loads.  Columns >= W are loaded and never used.
template <bool VEC>
__device__ __forceinline__ float4 long_load4(const float* row, int j4, int W) {
  if (VEC) return *reinterpret_cast<const float4*>(row + j4);
  return make_float4(row[min(j4, W - 1)], row[min(j4 + 1, W - 1)], row[min(j4 + 2, W - 1)], row[min(j4 + 3, W - 1)]);
}

// This forward's column sums of the four columns from j4: sum and sum of squares of pbar, and the last query's pbar (tova).
template <bool VEC>
__device__ __forceinline__ void long_columns(const EkvScoreArgs& a, int h, int ll, size_t hq0, int n, int rep, int off, int W, int j4,
                                             const float* sRowM, const float* sRowL, float (&cs)[4], float (&cq)[4], float (&last)[4]) {
  if (a.colsum != nullptr) {
    // two-pass chunk step: n_col_parts partial rows per head, summed in part order
    const float* cp = a.colsum + ((size_t)ll * a.n_kv_heads + h) * a.n_col_parts * 2 * a.t_pad + off;
    for (int p0 = 0; p0 < a.n_col_parts; p0 += 4) {
      float4 x[4], y[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int part = min(p0 + u, a.n_col_parts - 1);
        x[u] = long_load4<VEC>(cp + (size_t)(2 * part) * a.t_pad, j4, W);
        y[u] = long_load4<VEC>(cp + (size_t)(2 * part + 1) * a.t_pad, j4, W);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (p0 + u < a.n_col_parts) {
          cs[0] += x[u].x, cs[1] += x[u].y, cs[2] += x[u].z, cs[3] += x[u].w;
          cq[0] += y[u].x, cq[1] += y[u].y, cq[2] += y[u].z, cq[3] += y[u].w;
        }
      }
    }
    return;
  }
  // exported logits: the rows of a column in the order (query i, query head r), eight 16-byte loads in flight
  const float* base = a.logits + hq0 * n * a.t_pad + off;
  const int total = n * rep;
  float v[4] = {0.f, 0.f, 0.f, 0.f};
  int r = 0;
  for (int f0 = 0; f0 < total; f0 += 8) {
    float4 x[8];
    float mm[8], lr[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int f = min(f0 + u, total - 1), i = f / rep, row = (f - i * rep) * n + i;   // row = r * n + i
      x[u] = long_load4<VEC>(base + (size_t)row * a.t_pad, j4, W);
      mm[u] = sRowM[row];
      lr[u] = sRowL[row];
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      if (f0 + u < total) {
        v[0] += expf(x[u].x - mm[u]) * lr[u];
        v[1] += expf(x[u].y - mm[u]) * lr[u];
        v[2] += expf(x[u].z - mm[u]) * lr[u];
        v[3] += expf(x[u].w - mm[u]) * lr[u];
        if (++r == rep) {      // the GQA mean of query i is complete
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            const float pb = rep == 1 ? v[c] : v[c] / (float)rep;
            cs[c] += pb;
            cq[c] += pb * pb;
            last[c] = pb;
            v[c] = 0.f;
          }
          r = 0;
        }
      }
    }
  }
}

// FOLD16: see the header (the batch width of ekv_fold_partials_auto)
template <bool FOLD16>
__global__ void __launch_bounds__(kSW) ekv_long_sweep_kernel(const EkvScoreArgs a, uint32_t* const key_rows) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tile = blockIdx.x, h = blockIdx.y, ll = blockIdx.z, tid = threadIdx.x;
  const int gl = a.layer_begin + ll;
  const int n = a.q_len, rep = a.n_q_heads / a.n_kv_heads;
  const int off = a.score_off, W = a.n_slots - off, rows = rep * n;
  const int lrows = a.colsum != nullptr ? 0 : rows;
  float* sRowM = reinterpret_cast<float*>(smem);
  float* sRowL = sRowM + lrows;
  const size_t hq0 = (size_t)ll * a.n_q_heads + (size_t)h * rep;
  const size_t head_row = ((size_t)gl * a.n_kv_heads + h) * a.cap;

  // ---- row statistics of the logits rows: left by the chunk kernel's own fold, or folded from the key-range partials (per tile again:
  //      rows x n_partials loads)
  if (a.accumulate && lrows > 0) {
    const int PS = a.head_dim + 2;
    for (int row = tid; row < rows; row += kSW) {
      float mm, ls;
      if (a.row_stats != nullptr) {
        mm = a.row_stats[(hq0 * n + row) * 2];
        ls = a.row_stats[(hq0 * n + row) * 2 + 1];
      } else {
        (void)ekv_fold_partials_auto<(FOLD16 ? 16 : 8)>(a.partials + ((hq0 * n + row) * a.n_split) * PS, a.n_split, PS, 0, mm, ls);
      }
      sRowM[row] = mm;
      sRowL[row] = 1.f / ls;   // reciprocal of the row's sum of exponentials
    }
  }
  __syncthreads();

  const int j4 = tile * kLongTile + tid * 4;
  if (j4 >= W) return;
  const bool roco = a.policy == EKV_POLICY_ROCO;
  float s_in[4], q_in[4] = {0.f, 0.f, 0.f, 0.f}, c_in[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int c = 0; c < 4; ++c) {      // (score rows are cap floats apart: not 16-byte aligned in general)
    const int j = min(j4 + c, W - 1);
    s_in[c] = a.score_sum[head_row + j];
    if (roco) {
      q_in[c] = a.score_sq[head_row + j];
      c_in[c] = a.score_cnt[head_row + j];
    }
  }
  float cs[4] = {0.f, 0.f, 0.f, 0.f}, cq[4] = {0.f, 0.f, 0.f, 0.f}, last[4] = {0.f, 0.f, 0.f, 0.f};
  if (a.accumulate) {
    if ((off & 3) == 0) long_columns<true>(a, h, ll, hq0, n, rep, off, W, j4, sRowM, sRowL, cs, cq, last);
    else long_columns<false>(a, h, ll, hq0, n, rep, off, W, j4, sRowM, sRowL, cs, cq, last);
  }

  const size_t scratch_row = (size_t)ll * a.n_kv_heads + h;
  float* sS = a.big_rows + scratch_row * 3 * (size_t)a.big_stride;
  float* sQ = sS + a.big_stride;
  float* sC = sQ + a.big_stride;
  uint32_t* sKey = key_rows + scratch_row * (size_t)a.big_stride;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int j = j4 + c;
    if (j < W) {
      float s = s_in[c], q = q_in[c], cc = c_in[c];
      if (a.accumulate) {
        if (a.policy == EKV_POLICY_TOVA) {
          s = a.tova_head_mean ? a.tova_row[(size_t)ll * a.t_pad + off + j] : last[c];
        } else {
          s += cs[c];
          q += cq[c];
        }
      }
      // the stage-1 selection key (stage 3 of the generic scorer, first sweep)
      uint32_t key;
      if (roco) {
        cc = cc + a.count_add;
        const float mean = s / cc;
        float sd = sqrtf(q / cc - mean * mean);
        if (j >= W - a.roco_tail || j < a.win_lo) sd = 1e9f;
        key = ekv_fkey(sd);
      } else {   // h2o_head / tova: accumulated score inside the candidate window
        key = (j >= a.win_lo && j < W - a.win_tail) ? ekv_fkey(s) : 0xFFFFFFFFu;
      }
      sS[j] = s;
      sQ[j] = q;
      sC[j] = cc;
      sKey[j] = key;
    }
  }
}

__global__ void __launch_bounds__(kNT) ekv_long_select_kernel(const EkvScoreArgs a, uint32_t* const key_rows) {
  __shared__ __attribute__((aligned(16))) char smem[ekv_long_select_lds()];
  const int h = blockIdx.x, ll = blockIdx.y;
  const int gl = a.layer_begin + ll;
  const int off = a.score_off, W = a.n_slots - off;
  const size_t scratch_row = (size_t)ll * a.n_kv_heads + h;
  float* sS = a.big_rows + scratch_row * 3 * (size_t)a.big_stride;
  float* sQ = sS + a.big_stride;
  float* sC = sQ + a.big_stride;
  uint32_t* sKey = key_rows + scratch_row * (size_t)a.big_stride;
  Blk b;
  b.tid = threadIdx.x;
  b.lane = b.tid & 63;
  b.wave = b.tid >> 6;
  b.red = reinterpret_cast<unsigned long long*>(smem);
  b.phase = 0;
  uint32_t* sHist = reinterpret_cast<uint32_t*>(b.red) + 2 * kNWV * 8;   // 264 words, then the select's candidate list (kNT uint64)
  const size_t head_row = ((size_t)gl * a.n_kv_heads + h) * a.cap;
  const bool roco = a.policy == EKV_POLICY_ROCO;

  const int k = a.n_evict;
  if (k <= 0) {      // nothing to evict: the accumulated rows go back as they are (the counts were not advanced in the bank)
    if (a.accumulate) {
      for (int j = b.tid; j < W; j += kNT) {
        a.score_sum[head_row + j] = sS[j];
        if (roco) a.score_sq[head_row + j] = sQ[j];
      }
    }
    return;
  }

  // ---- 3. selection: k == 1 of h2o_head / tova yields `victim` directly; else flags in sKey (1 = evict) ----------------------------
  int victim = -1;
  if (roco) {
    blk_mark_k_smallest(b, sKey, W, a.roco_k1, sHist, ekv_fkey(1e9f));  // feasible set (1e9 sentinels and NaN above every real std)
    for (int j = b.tid; j < W; j += kNT) sKey[j] = sKey[j] ? ekv_fkey(sS[j] / sC[j]) : 0xFFFFFFFFu;
    __syncthreads();
    blk_mark_k_smallest(b, sKey, W, k, sHist);
  } else if (k == 1) {
    unsigned long long best = ~0ull;
    for (int j = a.win_lo + b.tid; j < W - a.win_tail; j += kNT) {
      const unsigned long long x = ((unsigned long long)sKey[j] << 32) | (uint32_t)j;
      best = x < best ? x : best;
    }
    victim = (int)(blk_min_u64(b, best) & 0xFFFFFFFFu);
  } else {
    blk_mark_k_smallest(b, sKey, W, k, sHist);
  }

  if (victim >= 0) {
    // ---- 4a. single victim: everything behind it moves up by one, no scan needed ------------------------
    for (int d = b.tid; d < W; d += kNT) {
      const int j = d + (d >= victim ? 1 : 0);
      const bool tail = d == W - 1;
      a.score_sum[head_row + d] = tail ? 0.f : sS[j];
      if (roco) {
        a.score_sq[head_row + d] = tail ? 0.f : sQ[j];
        a.score_cnt[head_row + d] = tail ? 0.f : sC[j];
      }
    }
    if (a.evict_ids != nullptr && b.tid == 0) a.evict_ids[(size_t)ll * a.n_kv_heads + h] = off + victim;
    // slot map: positions >= victim shift; the victim's row becomes the free tail (recycled by the next append)
    const int n_move = W - victim;          // entries victim .. W-1
    int32_t* sSlot = reinterpret_cast<int32_t*>(sKey);
    __syncthreads();
    for (int i = b.tid; i < n_move; i += kNT) sSlot[i] = a.slot_of_pos[head_row + off + victim + i];
    __syncthreads();
    for (int i = b.tid; i < n_move; i += kNT)
      a.slot_of_pos[head_row + off + victim + i] = (i == n_move - 1) ? sSlot[0] : sSlot[i + 1];
    return;
  }

  // ---- 4b. destinations: kept j -> #kept before j ; evicted j -> -(1 + #evicted before j) ----------
  {
    const int items = (W + kNT - 1) / kNT;
    const int c0 = min(W, b.tid * items), c1 = min(W, c0 + items);
    int kept = 0;
    for (int j = c0; j < c1; ++j) kept += sKey[j] ? 0 : 1;
    int incl = kept;
    for (int o = 1; o < 64; o <<= 1) {
      const int y = __shfl_up(incl, o, 64);
      if (b.lane >= o) incl += y;
    }
    int* r = reinterpret_cast<int*>(b.red) + (b.phase & 1) * kNWV * 2;
    if (b.lane == 63) r[b.wave] = incl;
    __syncthreads();
    int base = incl - kept;
    for (int i = 0; i < b.wave; ++i) base += r[i];
    b.phase++;
    for (int j = c0; j < c1; ++j) {
      if (sKey[j]) {
        sKey[j] = (uint32_t)(-(1 + (j - base)));
      } else {
        sKey[j] = (uint32_t)base;
        base++;
      }
    }
    __syncthreads();
  }

  // ---- 5. write back compacted score rows, evict ids -------------------------------------------------
  for (int j = b.tid; j < W; j += kNT) {
    const int d = (int)sKey[j];
    if (d >= 0) {
      a.score_sum[head_row + d] = sS[j];
      if (roco) {
        a.score_sq[head_row + d] = sQ[j];
        a.score_cnt[head_row + d] = sC[j];
      }
    }
  }
  for (int i = b.tid; i < k; i += kNT) {
    a.score_sum[head_row + W - k + i] = 0.f;
    if (roco) {
      a.score_sq[head_row + W - k + i] = 0.f;
      a.score_cnt[head_row + W - k + i] = (float)i * a.count_tail_step;
    }
  }
  if (a.evict_ids != nullptr) {
    for (int j = b.tid; j < W; j += kNT) {
      const int d = (int)sKey[j];
      if (d < 0) a.evict_ids[((size_t)ll * a.n_kv_heads + h) * k + (-1 - d)] = off + j;
    }
  }

  // ---- 6. slot-map compaction: kept rows keep their order, victims' rows become the free tail (staged in the S scratch row) -----
  __syncthreads();
  int32_t* sSlot = reinterpret_cast<int32_t*>(sS);
  for (int j = b.tid; j < W; j += kNT) sSlot[j] = a.slot_of_pos[head_row + off + j];
  __syncthreads();
  for (int j = b.tid; j < W; j += kNT) {
    const int d = (int)sKey[j];
    const int dst = d >= 0 ? d : (W - k) + (-1 - d);
    a.slot_of_pos[head_row + off + dst] = sSlot[j];
  }
}

// Partials of the key-range splits -> 16-bit attention output (rows = q_len * n_q_heads per layer): what the generic scorer does in
// its stage 0 when the output was not folded before it.  bf16: the element type of `out`.
template <bool FOLD16>
__global__ void __launch_bounds__(128) ekv_long_fold_kernel(const EkvScoreArgs sc, const int bf16) {
  const int D = sc.head_dim, PS = D + 2;
  const size_t row = (size_t)blockIdx.y * sc.n_q_heads * sc.q_len + blockIdx.x;
  const float* p0 = sc.partials + row * sc.n_split * PS;
  // (ekv_step.out_*_stride: blockIdx.x = head * q_len + token)
  __half* orow = sc.out + (size_t)blockIdx.y * sc.n_q_heads * sc.q_len * D + (size_t)(blockIdx.x / sc.q_len) * sc.o_hs + (size_t)(blockIdx.x % sc.q_len) * sc.o_ts;
  for (int d = threadIdx.x; d < D; d += 128) {
    const float o = ekv_fold_partials_auto<(FOLD16 ? 16 : 8)>(p0, sc.n_split, PS, d);
    orow[d] = bf16 ? __builtin_bit_cast(__half, (__bf16)o) : __float2half(o);
  }
}

// does the generic scorer build of the plain call fold in batches of 16 (its 512-thread build)?
bool long_fold16(const EkvScoreArgs& a, bool plain_big, int layer_count) {
  const int64_t W = (int64_t)a.n_slots - a.score_off;
  const int64_t rows = a.colsum != nullptr ? 0 : (int64_t)(a.n_q_heads / a.n_kv_heads) * a.q_len;
  return ekv_score_select_threads((int64_t)a.n_kv_heads * layer_count, W, rows, plain_big) == 512;
}

template <bool FOLD16>
hipError_t launch_long(const EkvScoreArgs& a, uint32_t* key_rows, int tiles, size_t lds, int layer_count, hipStream_t s) {
  if (lds > 48 * 1024)
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&ekv_long_sweep_kernel<FOLD16>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL(ekv_long_sweep_kernel<FOLD16>, dim3(tiles, a.n_kv_heads, layer_count), dim3(kSW), lds, s, a, key_rows);
  if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  hipLaunchKernelGGL(ekv_long_select_kernel, dim3(a.n_kv_heads, layer_count), dim3(kNT), 0, s, a, key_rows);
  return hipGetLastError();
}

}  // namespace

hipError_t ekv_launch_score_long(const EkvScoreArgs& a, uint32_t* key_rows, bool plain_big, int layer_count, hipStream_t s) {
  const bool scored = a.policy == EKV_POLICY_H2O_HEAD || a.policy == EKV_POLICY_ROCO || a.policy == EKV_POLICY_TOVA;
  const int64_t W = (int64_t)a.n_slots - a.score_off;
  if (!scored || a.big_rows == nullptr || key_rows == nullptr || W < 1 || W > a.big_stride || a.n_slots > a.cap) return hipErrorInvalidValue;
  if (layer_count < 1 || layer_count > 65535 || a.n_kv_heads > 65535) return hipErrorInvalidValue;      // (grid y / z)
  const size_t lds = ekv_long_sweep_lds(a.colsum != nullptr ? 0 : (int64_t)(a.n_q_heads / a.n_kv_heads) * a.q_len);
  if (lds > 160 * 1024) return hipErrorInvalidValue;
  const int tiles = (int)ekv_long_tiles(W);
  return long_fold16(a, plain_big, layer_count) ? launch_long<true>(a, key_rows, tiles, lds, layer_count, s)
                                                : launch_long<false>(a, key_rows, tiles, lds, layer_count, s);
}

hipError_t ekv_launch_long_fold(const EkvScoreArgs& a, bool plain_big, int layer_count, hipStream_t s, bool bf16) {
  if (layer_count < 1 || layer_count > 65535) return hipErrorInvalidValue;
  const dim3 grid(a.n_q_heads * a.q_len, layer_count);
  if (long_fold16(a, plain_big, layer_count)) hipLaunchKernelGGL(ekv_long_fold_kernel<true>, grid, dim3(128), 0, s, a, bf16 ? 1 : 0);
  else hipLaunchKernelGGL(ekv_long_fold_kernel<false>, grid, dim3(128), 0, s, a, bf16 ? 1 : 0);
  return hipGetLastError();
}
