// head_dim dispatch of the chunk (q_len > 1) attention kernels (which kernel and scheme a step takes: ekv_plan.cpp).
#include <cstdlib>

#include "ekv_common.h"
#include "ekv_kernels.h"

// ---- the instances (ekv_instances.def): launcher declarations, then one table entry per line
typedef hipError_t EkvChunkFn(const EkvAttnArgs&, int shape, int layer_count, hipStream_t, const EkvScoreArgs*);
typedef hipError_t EkvStepFn(const EkvAttnArgs&, const EkvScoreArgs&, int layer_count, hipStream_t);
#define EKV_CHUNK(d, m, elem) EkvChunkFn EKV_FN_CHUNK(d, m, elem);
#define EKV_CHUNK_CAP(elem, d, m) EkvChunkFn EKV_FN_CHUNK_CAP(d, m, elem);
#define EKV_WIDE(d, m, keys, elem) EkvChunkFn EKV_FN_WIDE(d, m, keys, elem);
// (the sink instances of the 16x16 kernel: their launchers take the sinks behind the arguments)
typedef hipError_t EkvSinkChunkFn(const EkvAttnArgs&, const float* sinks, int shape, int layer_count, hipStream_t, const EkvScoreArgs*);
#define EKV_CHUNK_SINK(elem, d, m) EkvSinkChunkFn EKV_FN_CHUNK_SINK(d, m, elem);
// (the window instances, alone and with sinks: one signature, `sinks` NULL in the window-alone ones)
typedef hipError_t EkvWinChunkFn(const EkvAttnArgs&, const float* sinks, const EkvWinArgs&, int shape, int layer_count, hipStream_t, const EkvScoreArgs*);
#define EKV_CHUNK_WIN(elem, d, m) EkvWinChunkFn EKV_FN_CHUNK_WIN(d, m, elem);
#define EKV_CHUNK_SINK_WIN(elem, d, m) EkvWinChunkFn EKV_FN_CHUNK_SINK_WIN(d, m, elem);
#define EKV_CHUNK_LDS(d, elem) EkvStepFn EKV_FN_D_ELEM(ekv_launch_chunk_lds, d, elem);
#define EKV_RESIDENT(d, elem) EkvStepFn EKV_FN_D_ELEM(ekv_launch_attn_resident, d, elem);
#include "ekv_instances.def"

namespace {
struct ChunkInstance {      // 16x16 kernel (rope: the fp16 builds rotate on read themselves) and wide-block kernel
  bool wide;
  int head_dim, mode;
  bool rope, bf16, capped;      // capped: the soft-capped builds of the 16x16 kernel (EKV_CHUNK_CAP)
  EkvChunkFn* fn;
};
const ChunkInstance kChunk[] = {
#define EKV_CHUNK(d, m, elem) {false, d, m, false, EKV_IS_##elem, false, EKV_FN_CHUNK(d, m, elem)},
#define EKV_CHUNK_CAP(elem, d, m) {false, d, m, false, EKV_IS_##elem, true, EKV_FN_CHUNK_CAP(d, m, elem)},
#define EKV_WIDE(d, m, keys, elem) {true, d, m, EKV_IS_##keys, EKV_IS_##elem, false, EKV_FN_WIDE(d, m, keys, elem)},
#include "ekv_instances.def"
};
struct SinkChunkInstance {
  int head_dim, mode;
  bool bf16;
  EkvSinkChunkFn* fn;
};
const SinkChunkInstance kSinkChunk[] = {
#define EKV_CHUNK_SINK(elem, d, m) {d, m, EKV_IS_##elem, EKV_FN_CHUNK_SINK(d, m, elem)},
#include "ekv_instances.def"
};
struct WinChunkInstance {
  int head_dim, mode;
  bool bf16, sink;
  EkvWinChunkFn* fn;
};
const WinChunkInstance kWinChunk[] = {
#define EKV_CHUNK_WIN(elem, d, m) {d, m, EKV_IS_##elem, false, EKV_FN_CHUNK_WIN(d, m, elem)},
#define EKV_CHUNK_SINK_WIN(elem, d, m) {d, m, EKV_IS_##elem, true, EKV_FN_CHUNK_SINK_WIN(d, m, elem)},
#include "ekv_instances.def"
};
struct StepInstance {      // whole-step kernels: logits in LDS, logits-resident
  bool resident;
  int head_dim;
  bool bf16;
  EkvStepFn* fn;
};
const StepInstance kStep[] = {
#define EKV_CHUNK_LDS(d, elem) {false, d, EKV_IS_##elem, EKV_FN_D_ELEM(ekv_launch_chunk_lds, d, elem)},
#define EKV_RESIDENT(d, elem) {true, d, EKV_IS_##elem, EKV_FN_D_ELEM(ekv_launch_attn_resident, d, elem)},
#include "ekv_instances.def"
};

EkvChunkFn* chunk_instance(bool wide, int head_dim, int mode, bool rope, bool bf16, bool capped = false) {
  for (const ChunkInstance& in : kChunk)
    if (in.wide == wide && in.head_dim == head_dim && in.mode == mode && in.rope == rope && in.bf16 == bf16 && in.capped == capped) return in.fn;
  return nullptr;
}
const StepInstance* step_instance(bool resident, int head_dim, bool bf16) {
  for (const StepInstance& in : kStep)
    if (in.resident == resident && in.head_dim == head_dim && in.bf16 == bf16) return &in;
  return nullptr;
}
}  // namespace

// rope_on_read: q' = q*cos[pos] + rotate_half(q)*sin[pos] with pos = T - n + i (llama_patch.py:311, :326), once per step,
// stored as an fp16 pair hi + lo (q' is an fp32 product; hi alone would cost ~5e-4 relative on the logits).
__global__ void __launch_bounds__(256) ekv_rope_q_kernel(const EkvAttnArgs a, int D, int n_rows) {
  // 256 / (D / 4) rows per workgroup, four consecutive d per thread (round 4: one 128-thread workgroup per row was 56 us of launch
  // overhead per configs[4] step — 153 600 workgroups)
  const int tpr = D / 4, rpb = 256 / tpr;
  const int r_in = blockIdx.x * rpb + threadIdx.x / tpr;       // (q head, query) of this layer
  if (r_in >= n_rows || (int)threadIdx.x >= rpb * tpr) return;      // (head_dim 96: 10 rows of 24 threads)
  const size_t row = (size_t)blockIdx.y * n_rows + r_in;       // (layer, q head, query)
  const int i = r_in % a.q_len;
  const int pos = a.n_slots - a.q_len + i;
  const __half* q = a.q + (size_t)blockIdx.y * n_rows * D + (size_t)(r_in / a.q_len) * a.q_hs + (size_t)i * a.q_ts;      // (ekv_step.q_*_stride)
  const int d0 = (threadIdx.x % tpr) * 4;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int d = d0 + e;
    const int dp = d < D / 2 ? d + D / 2 : d - D / 2;
    const float x = __half2float(q[d]), y = __half2float(q[dp]);
    const float qr = x * a.rope_cos[(size_t)pos * D + d] + (d < D / 2 ? -y : y) * a.rope_sin[(size_t)pos * D + d];
    const _Float16 hi = (_Float16)qr;
    reinterpret_cast<_Float16*>(a.q_rot_hi)[row * D + d] = hi;
    reinterpret_cast<_Float16*>(a.q_rot_lo)[row * D + d] = (_Float16)(qr - (float)hi);
  }
}

// 65..128-row blocks (qpw code 4): 8 waves x 2 query tiles — except the ONE-PASS kernel without rope-on-read, which runs SIXTEEN
// waves x 1 query tile (kernel code 8): <= 128 VGPRs per wave, so four waves per SIMD instead of two; the tile loop is a chain of
// LDS / MFMA / VALU latencies between two barriers and two waves per SIMD do not hide it (dense prefix 4906 tokens 411 -> 445
// TFLOP/s, 2048 tokens 319 -> 392).  The exact pass of the two-pass scheme stays on 8 waves: with 16 it writes twice the
// column-sum partial rows, which costs the scorer more than the attention kernel gains (C4 step 1.16 -> 1.25 ms, measured).
static int kernel_code(int qpw, bool rope, int mode) { return (qpw == 4 && !rope && mode == 0) ? 8 : qpw; }

// fuse_sc != nullptr: one-pass step with unsplit heads whose scorer runs as the tail of the attention kernel (no second launch)
// (kernel launches per call: ekv_attn_chunk_launches, ekv_plan.cpp)
hipError_t ekv_launch_attn_chunk(const EkvAttnArgs& a, int head_dim, int layer_count, bool wide, bool two_pass, hipStream_t s,
                                 const EkvScoreArgs* fuse_sc, int passes, const EkvScoreArgs* tail_sc, bool bf16, bool capped) {
  if (two_pass && (fuse_sc != nullptr || a.stats == nullptr || a.colsum == nullptr)) return hipErrorInvalidValue;
  if (tail_sc != nullptr && !(wide && two_pass && (passes & 2))) return hipErrorInvalidValue;
  int qb_rows, n_qblocks, qpw;
  // (a capped step is blocked as head_dim 256's, at either head_dim: the one-tile build is the only capped one)
  ekv_chunk_blocks(a.n_q_heads / a.n_kv_heads, a.q_len, &qb_rows, &n_qblocks, &qpw, capped ? kChunkNarrowD : head_dim);
  const bool rope = a.rope_cos != nullptr;
  if (capped && (wide || rope || !(a.softcap > 0.f) || a.softcap > 3.0e38f)) return hipErrorInvalidValue;      // (no capped wide or RoPE-on-read build)
  if (bf16 && rope) return hipErrorInvalidValue;   // (no bf16 RoPE-on-read build)
  if (rope && !wide) {      // (the wide-block kernel rotates its query rows itself, in the lane that holds them)
    if (a.q_rot_hi == nullptr || a.q_rot_lo == nullptr) return hipErrorInvalidValue;
    const int n_rows = a.n_q_heads * a.q_len, rpb = 256 / (head_dim / 4);
    hipLaunchKernelGGL(ekv_rope_q_kernel, dim3((n_rows + rpb - 1) / rpb, layer_count), dim3(256), 0, s, a, head_dim, n_rows);
  }
  if (wide) {
    if (fuse_sc != nullptr || (!two_pass && a.stats != nullptr)) return hipErrorInvalidValue;      // (mode 0 writes row statistics whenever the array is there)
    const int nwq = qpw == 4 ? 4 : 2;
    // one pass over K and V (output, and for a scored step every row's softmax statistics), then — scored steps — the column-sum
    // pass over K
    EkvChunkFn* const one = chunk_instance(true, head_dim, 0, rope, bf16);
    EkvChunkFn* const sums = chunk_instance(true, head_dim, 2, rope, bf16);
    if (one == nullptr || sums == nullptr) return hipErrorInvalidValue;
    hipError_t e = hipSuccess;
    if (passes & 1) {
      // a launch of at most one workgroup per CU (a layer-per-call model) runs 65..128-row blocks on 128-key tiles, 8 waves
      static const bool no_big = [] { const char* ev = std::getenv("EKV_NO_BIG_TILE"); return ev != nullptr && ev[0] == '1'; }();     // (A/B switch)
      // (... and key ranges long enough to hold several 128-key tiles: measured per one-layer call, 64-key / 128-key tiles — 96 rows x 640 keys
      //  per split 43.2 / 38.2 us; 64 rows x 272 keys 24.5 / 26.1; 32 layers x 8 KV heads x 1248 keys unsplit (configs[2]) 43.1 / 41.5)
      const bool small = (size_t)layer_count * a.n_kv_heads * a.n_split * a.n_qblocks <= 256 && a.rows_per_split >= 512;
      const int shape0 = (!rope && small && !no_big) ? (nwq == 4 ? 8 : 9) : nwq;      // workgroup-shape code of ekv_attn_wide.inc's entry (8 / 9: 128-key tiles)
      e = one(a, shape0, layer_count, s, nullptr);
    }
    if (two_pass && (passes & 2) && e == hipSuccess) {
      EkvAttnArgs a2 = a;
      a2.score_tail = tail_sc != nullptr ? 1 : 0;
      e = sums(a2, nwq, layer_count, s, tail_sc);
    }
    return e;
  }
  // (the fp16 instances of the 16x16 kernel hold the RoPE-on-read builds: one line per (head_dim, mode, element))
  auto go = [&](int m) {
    EkvChunkFn* const fn = chunk_instance(false, head_dim, m, false, bf16, capped);
    return fn ? fn(a, kernel_code(qpw, rope, m), layer_count, s, fuse_sc) : hipErrorInvalidValue;
  };
  hipError_t e = go(two_pass ? 1 : 0);
  if (two_pass && e == hipSuccess) e = go(2);
  return e;
}

// ---- attention sinks (the ekv_sink_* calls): the 16x16 kernel's sink instances, one pass (fuse_sc: with the scorer as its tail) or
// statistics pass + exact pass.  Blocked as head_dim 256's at either head_dim: the one-tile build is the only sink one.
hipError_t ekv_launch_attn_chunk_sink(const EkvAttnArgs& a, const float* sinks, int head_dim, int layer_count, bool two_pass, hipStream_t s,
                                      const EkvScoreArgs* fuse_sc, bool bf16) {
  if (sinks == nullptr || a.rope_cos != nullptr) return hipErrorInvalidValue;
  if (two_pass && (fuse_sc != nullptr || a.stats == nullptr || a.colsum == nullptr)) return hipErrorInvalidValue;
  int qb_rows, n_qblocks, qpw;
  ekv_chunk_blocks(a.n_q_heads / a.n_kv_heads, a.q_len, &qb_rows, &n_qblocks, &qpw, kChunkNarrowD);
  auto go = [&](int m) {
    for (const SinkChunkInstance& in : kSinkChunk)
      if (in.head_dim == head_dim && in.mode == m && in.bf16 == bf16) return in.fn(a, sinks, qpw, layer_count, s, fuse_sc);
    return hipErrorInvalidValue;
  };
  hipError_t e = go(two_pass ? 1 : 0);
  if (two_pass && e == hipSuccess) e = go(2);
  return e;
}

// ---- sliding windows (the ekv_win_* calls): the 16x16 kernel's window instances, with or without sinks, passes as the sink launcher's
hipError_t ekv_launch_attn_chunk_win(const EkvAttnArgs& a, const float* sinks, const EkvWinArgs& win, int head_dim, int layer_count, bool two_pass,
                                     hipStream_t s, const EkvScoreArgs* fuse_sc, bool bf16) {
  if (win.tok_pos == nullptr || win.windows == nullptr || a.rope_cos != nullptr) return hipErrorInvalidValue;
  if (two_pass && (fuse_sc != nullptr || a.stats == nullptr || a.colsum == nullptr)) return hipErrorInvalidValue;
  int qb_rows, n_qblocks, qpw;
  ekv_chunk_blocks(a.n_q_heads / a.n_kv_heads, a.q_len, &qb_rows, &n_qblocks, &qpw, kChunkNarrowD);
  auto go = [&](int m) {
    for (const WinChunkInstance& in : kWinChunk)
      if (in.head_dim == head_dim && in.mode == m && in.bf16 == bf16 && in.sink == (sinks != nullptr)) return in.fn(a, sinks, win, qpw, layer_count, s, fuse_sc);
    return hipErrorInvalidValue;
  };
  hipError_t e = go(two_pass ? 1 : 0);
  if (two_pass && e == hipSuccess) e = go(2);
  return e;
}

// ---- small-row chunk step with the logits in LDS (ekv_chunk_lds.inc) -------------------------------------------------------
hipError_t ekv_launch_chunk_lds(const EkvAttnArgs& a, const EkvScoreArgs& sc, int head_dim, int layer_count, hipStream_t s, bool bf16) {
  const StepInstance* in = step_instance(false, head_dim, bf16);
  return in ? in->fn(a, sc, layer_count, s) : hipErrorInvalidValue;
}

// ---- logits-resident scored chunk step (ekv_attn_resident.inc)
hipError_t ekv_launch_attn_resident(const EkvAttnArgs& a, const EkvScoreArgs& sc, int layer_count, hipStream_t s, bool bf16) {
  const StepInstance* in = step_instance(true, sc.head_dim, bf16);
  return in ? in->fn(a, sc, layer_count, s) : hipErrorInvalidValue;
}
