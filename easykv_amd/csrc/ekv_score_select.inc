// K3 + K4: per (layer, KV head) — exact softmax of the exported logits, GQA fold, score accumulation,
// victim selection, and order-preserving compaction of the score rows and of the slot map.
//
// Replaces, per layer (SURVEY.md probe 7 shows per-layer == all-layers-at-once):
//   GQA fold              easykv/easykv.py:188-196, :271-276
//   accumulate            easykv/easykv.py:287-300 (decode), :443-457 (prefill), :693-707 (auto)
//   count advance         easykv/easykv.py:304, :460, :708
//   select                easykv/easykv.py:310-337 (decode), :462-490 (prefill), :711-740 (auto)
//   K/V compaction        easykv/easykv.py:56-82, :105-112   -> 4-byte slot-map compaction, rows never move
//   score-row compaction  easykv/easykv.py:315-333, :465-490
// It also folds the key-range split partials of the attention kernel into the fp16 output.
//
// Selection is exact and deterministic: "k smallest" is an MSB-first radix select (8 bits per pass) on
// order-preserving uint32 keys held in LDS (no sort); ties go to the lowest index, NaN ranks largest.
// The score arithmetic mirrors the reference op for op in fp32 (IEEE div/sqrt; the library is built
// with -ffp-contract=off so q/c - (s/c)^2 is not fused).  One exception: the softmax normalisation p = exp(x - M) / L is
// computed as exp(x - M) * (1 / L) with the reciprocal taken once per row.  expf itself is v_exp_f32(x * log2e) (+ range
// fix-ups), ~1e-6 relative on these arguments and not the CPU library's exp either way, so a correctly rounded division
// behind it bought nothing — and with it the sweep spent 10 of its ~22 VALU instructions per element on v_div_*.
#include "ekv_common.h"
#include "ekv_kernels.h"

namespace {

constexpr int kNT = EKV_SS_NT;   // compiled for 256 and 512 threads per workgroup (ekv_score_select_nt*.hip)
constexpr int kNWV = kNT / 64;

#include "ekv_blk_select.h"   // Blk, blk_* reductions, blk_mark_k_smallest (shared with ekv_score_long.inc)

// EKV_POOL = 1 (the EKV_SCORE_SELECT_POOL lines of the manifest): the pooled build of the scorer (include/easykv_hip.h, "pooled selection").
// The kernel takes (radius, op) as its LAST argument; EKV_POOL_ONLY(...) spells what exists only in that build and vanishes everywhere
// else, so every other instance — and the chunk kernel's tail, which includes this body — keeps its tokens.
#ifndef EKV_POOL
#define EKV_POOL 0
#endif
#if EKV_POOL
#define EKV_POOL_ONLY(...) __VA_ARGS__
#else
#define EKV_POOL_ONLY(...)
#endif
// EKV_ADA = 1 (the EKV_SCORE_SELECT_ADA lines of the manifest): the adaptive build of the scorer (include/easykv_hip.h, "adaptive head
// budgets"), one build run twice around the allot kernel (ekv_score_allot.inc).  The kernel takes an EkvAdaArgs as its LAST argument;
// its pooling words stand where the pooled build has `pool`, and the stencil below is shared.  ada.phase 0 = rank: the accumulated score
// rows go back to the bank, the head's W ranking keys and the class of each (forced / free / neither, by two block selects) go to the
// workspace.  ada.phase 1 = select (launched with accumulate = 0: the rows are read back, the keys re-formed): k is the head's own, read
// from ada.k_out.  EKV_ADA_ONLY(...) vanishes in every other build.
#ifndef EKV_ADA
#define EKV_ADA 0
#endif
#if EKV_ADA
#define EKV_ADA_ONLY(...) __VA_ARGS__
#define EKV_SS_IDS_PITCH ada.evict_max      // evict_ids is [layer][head][evict_max]: entries beyond a head's k are left unwritten
#else
#define EKV_ADA_ONLY(...)
#define EKV_SS_IDS_PITCH k
#endif

// Wide logits sweep of the scorer (see the call site): thread -> 4 consecutive columns, 8 rows (IB queries x REP heads) of
// 16-byte loads in flight.  REP is a compile-time constant so that the per-batch arrays stay in registers.
template <int REP>
__device__ __forceinline__ void wide_sweep(const EkvScoreArgs& a, int tid, size_t hq0, size_t head_row, int ll, int n, int off, int W,
                                           const float* sRowM, const float* sRowL, float* sS, float* sQ, float* sC) {
  constexpr int IB = 8 / REP;
  int j4 = tid * 4;
  if (j4 >= W) return;
  const float* base = a.logits + hq0 * n * a.t_pad + off;
  // one batch = 8 rows x 4 columns of logits; unconditional (clamped) loads
  auto load_batch = [&](float4 (&x)[8], int jj, int i0) {
#pragma unroll
    for (int u = 0; u < 8; ++u) {      // u = ib * REP + r ; clamped query index, masked in the consumer
      const int r = u % REP, i = min(i0 + u / REP, n - 1);
      x[u] = *reinterpret_cast<const float4*>(base + jj + (size_t)(r * n + i) * a.t_pad);
    }
  };
  // Software pipeline over the flattened sequence (column group, row batch): the loads of the NEXT batch are in flight while
  // the current one goes through expf / div.  Without it every batch is one exposed L2/HBM round trip (the sweep was 40 % of
  // the scorer at stride 8 and 85 % at stride 64).
  float4 xa[8], xb[8];
  load_batch(xa, j4, 0);
  while (true) {
    float cs[4] = {0.f, 0.f, 0.f, 0.f}, cq[4] = {0.f, 0.f, 0.f, 0.f}, lastv[4] = {0.f, 0.f, 0.f, 0.f};
    // the score rows of these four columns, issued ahead of their use (clamped, masked below)
    float s_in[4], q_in[4] = {0.f, 0.f, 0.f, 0.f}, c_in[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int j = min(j4 + c, W - 1);
      s_in[c] = a.score_sum[head_row + j];
      if (a.policy == EKV_POLICY_ROCO) {
        q_in[c] = a.score_sq[head_row + j];
        c_in[c] = a.score_cnt[head_row + j];
      }
    }
    for (int i0 = 0; i0 < n; i0 += IB) {
      const bool last_batch = i0 + IB >= n;
      const int nj = last_batch ? (j4 + kNT * 4 < W ? j4 + kNT * 4 : j4) : j4;   // past the end: a harmless re-read
      load_batch(xb, nj, last_batch ? 0 : i0 + IB);
#pragma unroll
      for (int ib = 0; ib < IB; ++ib) {
        const int i = min(i0 + ib, n - 1);
        float v[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int r = 0; r < REP; ++r) {
          const float mm = sRowM[r * n + i], lr = sRowL[r * n + i];
          const float4 xv = xa[ib * REP + r];
          v[0] += expf(xv.x - mm) * lr;
          v[1] += expf(xv.y - mm) * lr;
          v[2] += expf(xv.z - mm) * lr;
          v[3] += expf(xv.w - mm) * lr;
        }
        if (i0 + ib < n) {
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            const float pb = REP == 1 ? v[c] : v[c] / (float)REP;
            cs[c] += pb;
            cq[c] += pb * pb;
            lastv[c] = pb;
          }
        }
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) xa[u] = xb[u];
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int j = j4 + c;
      if (j < W) {
        float s = s_in[c];
        float q = q_in[c], cc = c_in[c];
        if (a.policy == EKV_POLICY_TOVA) {
          s = a.tova_head_mean ? a.tova_row[(size_t)ll * a.t_pad + off + j] : lastv[c];
        } else {
          s += cs[c];
          q += cq[c];
        }
        sS[j] = s;
        sQ[j] = q;
        sC[j] = cc;
      }
    }
    j4 += kNT * 4;
    if (j4 >= W) break;
  }
}

// The scorer of one (KV head h, layer ll of the launch) by the kNT threads of a workgroup; `smem` = its dynamic LDS
// (ekv_score_lds_bytes, ekv_geometry.h).  Body of ekv_score_select_kernel, and the tail of the chunk attention kernel when a head is not
// split (ekv_attn_chunk.inc, FUSE): the scorer of one head then overlaps the K/V stream of the workgroups still streaming.
// BIG: rows wider than one CU's LDS (W > ~10 000: 16 B of LDS per column).  The working copies of the score rows live in global
// scratch (a.big_rows; L2-resident, the workgroup's own barriers order its accesses) and LDS holds the selection keys only, 4 B per
// column: W up to ~39 000.  Same code, same arithmetic, same summation order — only where sS / sQ / sC point differs; the template
// keeps the LDS address space provable (ds_read instead of flat loads) in the build every other shape uses.
template <bool BIG = false>
__device__ void ekv_score_select_body(const EkvScoreArgs& a, const int h, const int ll, char* smem EKV_POOL_ONLY(, const EkvPoolArgs& pool) EKV_ADA_ONLY(, const EkvAdaArgs& ada)) {
  const int gl = a.layer_begin + ll;
  const int T = a.n_slots, n = a.q_len, D = a.head_dim;
  const int rep = a.n_q_heads / a.n_kv_heads;
  const bool scored = a.policy == EKV_POLICY_H2O_HEAD || a.policy == EKV_POLICY_ROCO || a.policy == EKV_POLICY_TOVA;
  const int off = scored ? a.score_off : 0;
  const int W = T - off;
  const int rows = rep * n;
  // per-row softmax statistics in LDS: only when this forward's probabilities are rebuilt from exported logits.  With the column
  // sums of the two-pass chunk kernels nothing per row is needed — a scored dense prefix (keep_attention, easykv/easykv.py:173-186)
  // arrives as ONE step of thousands of rows
  const int lrows = a.colsum != nullptr ? 0 : rows;

  float* const big = BIG ? a.big_rows + ((size_t)ll * a.n_kv_heads + h) * 3 * (size_t)a.big_stride : nullptr;
  float* sS = BIG ? big : reinterpret_cast<float*>(smem);
  float* sQ = BIG ? big + a.big_stride : sS + W;
  float* sC = BIG ? big + 2 * (size_t)a.big_stride : sQ + W;
  uint32_t* sKey = BIG ? reinterpret_cast<uint32_t*>(smem) : reinterpret_cast<uint32_t*>(sC + W);
  float* sRowM = reinterpret_cast<float*>(sKey + W);
  float* sRowL = sRowM + lrows;
  Blk b;
  b.tid = threadIdx.x;
  b.lane = b.tid & 63;
  b.wave = b.tid >> 6;
  b.red = reinterpret_cast<unsigned long long*>(smem + ekv_align((size_t)((BIG ? 1 : 4) * W + 2 * lrows) * 4, 16));
  b.phase = 0;
  uint32_t* sHist = reinterpret_cast<uint32_t*>(b.red) + 2 * kNWV * 8;   // 264 words, then the select's candidate list (kNT uint64)

  const size_t head_row = ((size_t)gl * a.n_kv_heads + h) * a.cap;
  const size_t hq0 = (size_t)ll * a.n_q_heads + (size_t)h * rep;
#ifdef EKV_TAIL_PROFILE
  unsigned long long* stamps = reinterpret_cast<unsigned long long*>(a.tova_row) + ((size_t)ll * a.n_kv_heads + h) * 8;
#define EKV_SS_STAMP(i) do { __syncthreads(); if (threadIdx.x == 0) stamps[i] = __builtin_readcyclecounter(); } while (0)
#else
#define EKV_SS_STAMP(i) do { } while (0)
#endif
  EKV_SS_STAMP(0);

  // ---- 0. fold the key-range splits into the attention output; the fold also yields every query row's softmax
  //         statistics (max, sum exp), which the scorer needs to turn the exported logits into probabilities --------
  const int PS = D + 2;
  if (a.row_stats != nullptr && scored) {   // the chunk kernel folded its own output and left the row statistics here
    for (int row = b.tid; row < rows; row += kNT) {
      sRowM[row] = a.row_stats[(hq0 * n + row) * 2];
      sRowL[row] = 1.f / a.row_stats[(hq0 * n + row) * 2 + 1];   // reciprocal of the row's sum of exponentials
    }
  }
  const bool nothing_to_fold = a.row_stats != nullptr || (a.skip_fold && (a.colsum != nullptr || !a.accumulate));
  for (int idx = b.tid; idx < (nothing_to_fold ? 0 : rows * D); idx += kNT) {
    const int row = idx / D, d = idx % D;  // row = r*n + i
    // output already folded (ekv_fold_kernel, or the chunk kernel itself): row statistics only, and only if they are used
    if (a.skip_fold && (d != 0 || a.colsum != nullptr || !a.accumulate)) continue;
    float mm, ls;
    const float o = ekv_fold_partials_auto<(EKV_SS_NT == 512 ? 16 : 8)>(a.partials + ((hq0 * n + row) * a.n_split) * PS, a.n_split, PS, d, mm, ls);
    if (!a.skip_fold)      // row = r * n + i (ekv_step.out_*_stride)
      a.out[(size_t)ll * a.n_q_heads * n * D + (size_t)(h * rep + row / n) * a.o_hs + (size_t)(row % n) * a.o_ts + d] = ekv_to_e(o);
    if (d == 0 && scored && a.colsum == nullptr) sRowM[row] = mm, sRowL[row] = 1.f / ls;
  }

  EKV_SS_STAMP(1);
  if (scored) {
    __syncthreads();
    EKV_SS_STAMP(2);
    // ---- 2. load the score rows, add this forward's folded probabilities ---------------------
    const float inv_rep_div = (float)rep;
    // Wide path for the logits sweep (rows x W floats per head — as many bytes as K+V at 64..128 rows): every thread owns
    // FOUR consecutive columns and keeps eight 16-byte row loads in flight (the scalar path below keeps 8 x 4 bytes).
    // One batch = IB queries x rep heads = 8 rows, so the GQA mean over the rep heads of a query is complete in a batch.
    const bool wide = a.accumulate && a.colsum == nullptr && (off & 3) == 0 && (rep == 1 || rep == 2 || rep == 4 || rep == 8) &&
                      rows >= 8;
    if (wide) {
      switch (rep) {
        case 1: wide_sweep<1>(a, b.tid, hq0, head_row, ll, n, off, W, sRowM, sRowL, sS, sQ, sC); break;
        case 2: wide_sweep<2>(a, b.tid, hq0, head_row, ll, n, off, W, sRowM, sRowL, sS, sQ, sC); break;
        case 4: wide_sweep<4>(a, b.tid, hq0, head_row, ll, n, off, W, sRowM, sRowL, sS, sQ, sC); break;
        default: wide_sweep<8>(a, b.tid, hq0, head_row, ll, n, off, W, sRowM, sRowL, sS, sQ, sC); break;
      }
    }
    // Two-pass chunk steps: the column sums arrive as n_col_parts partial rows per head.  Four consecutive columns per thread, the
    // 16-byte loads of four partial rows (sum and square) in flight together: the scalar loop below walks the parts one dependent
    // round trip after the other (8 parts x 5 columns per thread at the C4 shape: 100 of the scorer's 150 us).  Same summation
    // order (part 0, 1, 2, ...) as the scalar loop, which still handles the last W % 4 columns.
    const bool colfast = a.accumulate && a.colsum != nullptr && (off & 3) == 0 && a.policy != EKV_POLICY_TOVA;
    const int Wq = wide ? W : (colfast ? (W & ~3) : 0);
    if (colfast && !wide) {
      const bool roco_rows = a.policy == EKV_POLICY_ROCO;
      const float* cp0 = a.colsum + ((size_t)ll * a.n_kv_heads + h) * a.n_col_parts * 2 * a.t_pad + off;
      for (int j = b.tid * 4; j < Wq; j += kNT * 4) {
        float sv[4], qv[4] = {0.f, 0.f, 0.f, 0.f}, cv[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int u = 0; u < 4; ++u) {      // (score rows are cap floats apart: not 16-byte aligned in general)
          sv[u] = a.score_sum[head_row + j + u];
          if (roco_rows) qv[u] = a.score_sq[head_row + j + u], cv[u] = a.score_cnt[head_row + j + u];
        }
        float4 cs = make_float4(0.f, 0.f, 0.f, 0.f), cq = cs;
        for (int p0 = 0; p0 < a.n_col_parts; p0 += 4) {
          float4 x[4], y[4];
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const int part = min(p0 + u, a.n_col_parts - 1);
            x[u] = *reinterpret_cast<const float4*>(cp0 + (size_t)(2 * part) * a.t_pad + j);
            y[u] = *reinterpret_cast<const float4*>(cp0 + (size_t)(2 * part + 1) * a.t_pad + j);
          }
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            if (p0 + u < a.n_col_parts) {
              cs.x += x[u].x, cs.y += x[u].y, cs.z += x[u].z, cs.w += x[u].w;
              cq.x += y[u].x, cq.y += y[u].y, cq.z += y[u].z, cq.w += y[u].w;
            }
          }
        }
        sS[j] = sv[0] + cs.x, sS[j + 1] = sv[1] + cs.y, sS[j + 2] = sv[2] + cs.z, sS[j + 3] = sv[3] + cs.w;
        sQ[j] = qv[0] + cq.x, sQ[j + 1] = qv[1] + cq.y, sQ[j + 2] = qv[2] + cq.z, sQ[j + 3] = qv[3] + cq.w;
        sC[j] = cv[0], sC[j + 1] = cv[1], sC[j + 2] = cv[2], sC[j + 3] = cv[3];
      }
    }
    for (int j = Wq + b.tid; j < W; j += kNT) {
      float s = a.score_sum[head_row + j];
      float q = 0.f, c = 0.f;
      if (a.policy == EKV_POLICY_ROCO) {
        q = a.score_sq[head_row + j];
        c = a.score_cnt[head_row + j];
      }
      if (a.accumulate) {
        float colsum = 0.f, colsq = 0.f, last = 0.f;
        const float* col = a.logits + hq0 * n * a.t_pad + off + j;
        if (a.colsum != nullptr) {
          // two-pass chunk kernel: the column sums were accumulated next to the MFMA tiles, one partial per
          // (query block, query-tile wave); fixed summation order
          const float* cp = a.colsum + ((size_t)ll * a.n_kv_heads + h) * a.n_col_parts * 2 * a.t_pad + off + j;
          for (int part = 0; part < a.n_col_parts; ++part) {
            colsum += cp[(size_t)(2 * part) * a.t_pad];
            colsq += cp[(size_t)(2 * part + 1) * a.t_pad];
          }
        } else if (rep == 1) {
          // 8 independent loads in flight per thread (the rows of a column are t_pad floats apart)
          for (int i0 = 0; i0 < n; i0 += 8) {
            float x[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) x[u] = col[(size_t)min(i0 + u, n - 1) * a.t_pad];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
              if (i0 + u < n) {
                const float pb = expf(x[u] - sRowM[i0 + u]) * sRowL[i0 + u];
                colsum += pb;
                colsq += pb * pb;
                last = pb;
              }
            }
          }
        } else {
          for (int i = 0; i < n; ++i) {
            float pb = 0.f;
            float x[8];
#pragma unroll
            for (int r = 0; r < 8; ++r) x[r] = col[(size_t)(min(r, rep - 1) * n + i) * a.t_pad];
#pragma unroll
            for (int r = 0; r < 8; ++r)
              if (r < rep) pb += expf(x[r] - sRowM[r * n + i]) * sRowL[r * n + i];
            for (int r = 8; r < rep; ++r) pb += expf(col[(size_t)(r * n + i) * a.t_pad] - sRowM[r * n + i]) * sRowL[r * n + i];
            pb = pb / inv_rep_div;
            colsum += pb;
            colsq += pb * pb;
            last = pb;
          }
        }
        if (a.policy == EKV_POLICY_TOVA) {
          s = a.tova_head_mean ? a.tova_row[(size_t)ll * a.t_pad + off + j] : last;
        } else {
          s += colsum;
          q += colsq;
        }
      }
      sS[j] = s;
      sQ[j] = q;
      sC[j] = c;
    }
    __syncthreads();
  }

  EKV_SS_STAMP(3);
#if EKV_ADA
  const EkvPoolArgs pool{ada.radius, ada.op};
  const size_t ada_row = ((size_t)ll * a.n_kv_heads + h) * ada.stride;
  if (ada.phase == 0 && a.accumulate)      // (a step that does not accumulate ranks the rows as the bank holds them: nothing to write)
    for (int j = b.tid; j < W; j += kNT) a.score_sum[head_row + j] = sS[j];
  // rank: evict_max >= 1 carries it past the early return below, as far as the keys.  select: the head's own share; with k_h = 0 the
  // early return below is taken with accumulate = 0 and writes nothing, which is right only because the rank phase has already put the
  // accumulated rows into the bank and a head that evicts nothing has nothing to compact.
  const int k = ada.phase == 0 ? ada.evict_max : ada.k_out[ll * a.n_kv_heads + h];
#else
  const int k = a.n_evict;
#endif
  if (k <= 0) {
    if (scored && a.accumulate) {
      for (int j = b.tid; j < W; j += kNT) {
        a.score_sum[head_row + j] = sS[j];
        if (a.policy == EKV_POLICY_ROCO) a.score_sq[head_row + j] = sQ[j];
      }
    }
    return;
  }

  // ---- 3. selection: k == 1 yields `victim` directly; k > 1 leaves flags in sKey (1 = evict) -------------
  int victim = -1;
  if (a.policy == EKV_POLICY_RANGE) {
    if (k == 1) {
      victim = a.range_start;
    } else {
      for (int j = b.tid; j < W; j += kNT) sKey[j] = (j >= a.range_start && j < a.range_start + k) ? 1u : 0u;
      __syncthreads();
    }
  } else if (a.policy == EKV_POLICY_ROCO) {
    for (int j = b.tid; j < W; j += kNT) {
      const float c = sC[j] + a.count_add;
      sC[j] = c;
      const float mean = sS[j] / c;
      float sd = sqrtf(sQ[j] / c - mean * mean);
      if (j >= W - a.roco_tail || j < a.win_lo) sd = 1e9f;
      sKey[j] = ekv_fkey(sd);
    }
    __syncthreads();
    // (no candidate walk for k == 1 either: in steady state the lowest-mean tokens are exactly the ones outside the feasible
    // set, see ekv_decode_tail.h; the feasible set is marked exactly, then the k smallest means are taken from it)
    if (victim < 0) {
      blk_mark_k_smallest(b, sKey, W, a.roco_k1, sHist, ekv_fkey(1e9f));  // feasible set (1e9 sentinels and NaN above every real std)
      for (int j = b.tid; j < W; j += kNT) sKey[j] = sKey[j] ? ekv_fkey(sS[j] / sC[j]) : 0xFFFFFFFFu;
      __syncthreads();
      blk_mark_k_smallest(b, sKey, W, k, sHist);
    }
  } else {  // h2o_head / tova: k smallest accumulated scores inside the candidate window
#if EKV_POOL || EKV_ADA
    // Pooled selection: the ranking value of a candidate j in R = [win_lo, W - win_tail) is the max / the average of the score row over
    // [j - r, j + r] clipped to R (torch's max_pool1d / avg_pool1d on the slice s[R], stride 1, padding r: the -inf padding of max leaves
    // an edge window fewer members, the zero padding of avg adds nothing to the sum and the divisor stays 2r + 1).  The stencil reads the
    // score row where it sits (sS: LDS, or the L2-resident scratch of the BIG build) and writes the selection keys (sKey: LDS in every
    // build) — the second row the stencil needs is the key row the select needs anyway, so the LDS plan is the unpooled scorer's.
    // Thread tid owns columns tid, tid + kNT, ...: lane l of a wave reads word base + l at every tap, one bank per lane, no conflict.
    // avg: the sum in ascending index order, one IEEE division (the library is built with -ffp-contract=off).  max: fmaxf drops a NaN,
    // so a window that holds one is set to NaN by hand; ekv_fkey ranks NaN largest.  The pooled values rank only: sS is not modified.
    {
      const int lo = a.win_lo, hi = W - a.win_tail, r = pool.radius;
      const float n_taps = (float)(2 * r + 1);
      for (int j = b.tid; j < W; j += kNT) {
        uint32_t key = 0xFFFFFFFFu;
        if (j >= lo && j < hi) {
          const int j0 = max(lo, j - r), j1 = min(hi - 1, j + r);
          float v;
          if (pool.op == EKV_POOL_AVG) {
            float acc = 0.f;
            for (int i = j0; i <= j1; ++i) acc += sS[i];
            v = acc / n_taps;
          } else {
            float m = EKV_NEG_INF;
            bool has_nan = false;
            for (int i = j0; i <= j1; ++i) {
              const float x = sS[i];
              has_nan = has_nan || x != x;
              m = fmaxf(m, x);
            }
            v = has_nan ? __builtin_nanf("") : m;
          }
          key = ekv_fkey(v);
        }
        sKey[j] = key;
      }
      __syncthreads();
#if EKV_ADA
      if (ada.phase == 0) {
        // the keys as the allot kernel reads them, then the two class boundaries: the evict_max smallest are forced or free, the evict_min
        // smallest of them forced.  Thread tid reads back only what it wrote itself (columns tid, tid + kNT, ...).
        uint32_t* const gkey = ada.keys + ada_row;
        uint8_t* const gcls = ada.cls + ada_row;
        for (int j = b.tid; j < W; j += kNT) gkey[j] = sKey[j];
        blk_mark_k_smallest(b, sKey, W, ada.evict_max, sHist);
        for (int j = b.tid; j < W; j += kNT) {
          gcls[j] = sKey[j] ? 1 : 2;
          sKey[j] = gkey[j];
        }
        __syncthreads();
        if (ada.evict_min > 0) {
          blk_mark_k_smallest(b, sKey, W, ada.evict_min, sHist);
          for (int j = b.tid; j < W; j += kNT)
            if (sKey[j]) gcls[j] = 0;
        }
        return;
      }
#endif
      blk_mark_k_smallest(b, sKey, W, k, sHist);
    }
#else
    if (k == 1) {
      unsigned long long best = ~0ull;
      for (int j = a.win_lo + b.tid; j < W - a.win_tail; j += kNT) {
        const unsigned long long x = ((unsigned long long)ekv_fkey(sS[j]) << 32) | (uint32_t)j;
        best = x < best ? x : best;
      }
      victim = (int)(blk_min_u64(b, best) & 0xFFFFFFFFu);
    } else {
      for (int j = b.tid; j < W; j += kNT)
        sKey[j] = (j >= a.win_lo && j < W - a.win_tail) ? ekv_fkey(sS[j]) : 0xFFFFFFFFu;
      __syncthreads();
      blk_mark_k_smallest(b, sKey, W, k, sHist);
    }
#endif
  }
  const bool roco = a.policy == EKV_POLICY_ROCO;
  EKV_SS_STAMP(4);

  if (victim >= 0) {
    // ---- 4a. single victim: everything behind it moves up by one, no scan needed ------------------------
    if (scored) {
      for (int d = b.tid; d < W; d += kNT) {
        const int j = d + (d >= victim ? 1 : 0);
        const bool tail = d == W - 1;
        a.score_sum[head_row + d] = tail ? 0.f : sS[j];
        if (roco) {
          a.score_sq[head_row + d] = tail ? 0.f : sQ[j];
          a.score_cnt[head_row + d] = tail ? 0.f : sC[j];
        }
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

  EKV_SS_STAMP(5);
  // ---- 5. write back compacted score rows, evict ids -------------------------------------------------
  if (scored) {
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
  }
  if (a.evict_ids != nullptr) {
    for (int j = b.tid; j < W; j += kNT) {
      const int d = (int)sKey[j];
      if (d < 0) a.evict_ids[((size_t)ll * a.n_kv_heads + h) * EKV_SS_IDS_PITCH + (-1 - d)] = off + j;
    }
  }

  // ---- 6. slot-map compaction: kept rows keep their order, victims' rows become the free tail -----
  __syncthreads();
  int32_t* sSlot = reinterpret_cast<int32_t*>(sS);
  for (int j = b.tid; j < W; j += kNT) sSlot[j] = a.slot_of_pos[head_row + off + j];
  __syncthreads();
  for (int j = b.tid; j < W; j += kNT) {
    const int d = (int)sKey[j];
    const int dst = d >= 0 ? d : (W - k) + (-1 - d);
    a.slot_of_pos[head_row + off + dst] = sSlot[j];
  }
  EKV_SS_STAMP(6);
}

#ifndef EKV_SS_DEVICE_ONLY
#if EKV_ADA && EKV_BF16       // (the adaptive instances: likewise)
#define ekv_score_select_kernel ekv_score_select_kernel_ada_bf16
#elif EKV_ADA
#define ekv_score_select_kernel ekv_score_select_kernel_ada
#elif EKV_POOL && EKV_BF16      // (the pooled instances: the scorer alone, under names of its own)
#define ekv_score_select_kernel ekv_score_select_kernel_pool_bf16
#elif EKV_POOL
#define ekv_score_select_kernel ekv_score_select_kernel_pool
#elif EKV_BF16   // (bf16 instances: the scorer under a tagged name; the head-mean row writes no 16-bit data and is built once)
#define ekv_score_select_kernel ekv_score_select_kernel_bf16
#endif
// EKV_SINK = 1 (the EKV_TOVA_MEAN_SINK line of the manifest): the head-mean TOVA row of a sink call (ekv_common.h, "attention sinks"), the
// one kernel of this file that rebuilds a softmax from exported logits alone: M = max(row maximum, a) and the sum gains exp(a - M).  The
// object holds that kernel only — the scorer itself takes (M, 1 / L) of every row from partials or row statistics that carry the sink.
#if EKV_SINK
#define ekv_tova_headmean_kernel ekv_tova_headmean_kernel_sink
#else
template <bool BIG>
__global__ void __launch_bounds__(kNT) ekv_score_select_kernel(const EkvScoreArgs a EKV_POOL_ONLY(, const EkvPoolArgs pool) EKV_ADA_ONLY(, const EkvAdaArgs ada)) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  ekv_score_select_body<BIG>(a, blockIdx.x, blockIdx.y, smem EKV_POOL_ONLY(, pool) EKV_ADA_ONLY(, ada));
}

#endif  // !EKV_SINK

#if !EKV_BF16 && !EKV_POOL && !EKV_ADA
// 'tova' in encoding/ppl mode: one last-query row averaged over ALL kv heads (easykv/easykv.py:456, :847)
__global__ void __launch_bounds__(kNT) ekv_tova_headmean_kernel(const EkvScoreArgs a EKV_SINK_ONLY(, const float* const sinks)) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int ll = blockIdx.x;
  const int T = a.n_slots, n = a.q_len, H = a.n_kv_heads;
  const int rep = a.n_q_heads / H;
  float* sM = reinterpret_cast<float*>(smem);
  float* sL = sM + H * rep;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int hr = wave; hr < H * rep; hr += kNWV) {
    const float* lg = a.logits + (((size_t)ll * a.n_q_heads + hr) * n + (n - 1)) * a.t_pad;
    float mx = EKV_NEG_INF;
    for (int j = lane; j < T; j += 64) mx = fmaxf(mx, lg[j]);
    mx = ekv_wave_max(mx);
#if EKV_SINK
    const float sink_a = sinks[(size_t)(a.layer_begin + ll) * a.n_q_heads + hr];
    mx = fmaxf(mx, sink_a);
#endif
    float sm = 0.f;
    for (int j = lane; j < T; j += 64) sm += expf(lg[j] - mx);
    sm = ekv_wave_sum(sm);
#if EKV_SINK
    sm += expf(sink_a - mx);      // the virtual key: no column, its share of the row's mass
#endif
    if (lane == 0) {
      sM[hr] = mx;
      sL[hr] = 1.f / sm;
    }
  }
  __syncthreads();
  for (int j = tid; j < T; j += kNT) {
    float acc = 0.f;
    for (int h = 0; h < H; ++h) {
      float pb = 0.f;
      for (int r = 0; r < rep; ++r) {
        const int hr = h * rep + r;
        const float x = a.logits[(((size_t)ll * a.n_q_heads + hr) * n + (n - 1)) * a.t_pad + j];
        pb += expf(x - sM[hr]) * sL[hr];
      }
      if (rep > 1) pb = pb / (float)rep;
      acc += pb;
    }
    a.tova_row[(size_t)ll * a.t_pad + j] = acc / (float)H;
  }
}
#endif

#endif  // EKV_SS_DEVICE_ONLY

}  // namespace

#ifndef EKV_SS_DEVICE_ONLY
#define EKV_SS_CAT_(a, b) a##b
#define EKV_SS_CAT(a, b) EKV_SS_CAT_(a, b)

#if EKV_SINK
hipError_t ekv_launch_tova_headmean_sink(const EkvScoreArgs& a, const float* sinks, int layer_count, hipStream_t s) {
  if (sinks == nullptr) return hipErrorInvalidValue;
  const size_t lds = (size_t)a.n_q_heads * 2 * 4;
  hipLaunchKernelGGL(ekv_tova_headmean_kernel, dim3(layer_count), dim3(kNT), lds, s, a, sinks);
  return hipGetLastError();
}
#else
#if EKV_POOL
hipError_t EKV_FN_SCORE_SELECT_POOL(EKV_SS_NT, EKV_ELEM)(const EkvScoreArgs& a, const EkvPoolArgs& pool, int layer_count, hipStream_t s) {
#elif EKV_ADA
hipError_t EKV_FN_SCORE_SELECT_ADA(EKV_SS_NT, EKV_ELEM)(const EkvScoreArgs& a, const EkvAdaArgs& ada, int layer_count, hipStream_t s) {
#else
hipError_t EKV_FN_SCORE_SELECT(EKV_SS_NT, EKV_ELEM)(const EkvScoreArgs& a, int layer_count, hipStream_t s) {
#endif
  const size_t lds = ekv_score_lds_bytes(kNT, a);
  if (lds > 160 * 1024) return hipErrorInvalidValue;
#if EKV_SS_NT == 1024
  if (a.big_rows != nullptr) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&ekv_score_select_kernel<true>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(ekv_score_select_kernel<true>, dim3(a.n_kv_heads, layer_count), dim3(kNT), lds, s, a EKV_POOL_ONLY(, pool) EKV_ADA_ONLY(, ada));
    return hipGetLastError();
  }
#endif
  if (a.big_rows != nullptr) return hipErrorInvalidValue;   // (the wide-row variant is the 1024-thread build)
  if (lds > 48 * 1024)
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&ekv_score_select_kernel<false>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL(ekv_score_select_kernel<false>, dim3(a.n_kv_heads, layer_count), dim3(kNT), lds, s, a EKV_POOL_ONLY(, pool) EKV_ADA_ONLY(, ada));
  return hipGetLastError();
}

#if !EKV_BF16 && !EKV_POOL && !EKV_ADA
hipError_t EKV_SS_CAT(ekv_launch_tova_headmean_nt, EKV_SS_NT)(const EkvScoreArgs& a, int layer_count, hipStream_t s) {
  const size_t lds = (size_t)a.n_q_heads * 2 * 4;
  hipLaunchKernelGGL(ekv_tova_headmean_kernel, dim3(layer_count), dim3(kNT), lds, s, a);
  return hipGetLastError();
}
#endif
#endif  // !EKV_SINK
#endif  // EKV_SS_DEVICE_ONLY
