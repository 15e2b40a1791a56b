// Bank utility kernels and their launch code: slot-map iota, score-state init, row gather / scatter, in-place compaction, range
// eviction (+ its batch twin) and the ordered <-> slot-indexed conversion of the score rows.  The entry points that check the arguments
// are in ekv_abi.hip.
#include <cstdlib>

#include "ekv_common.h"
#include "ekv_kernels.h"

namespace {

__global__ void ekv_iota_rows_kernel(int32_t* slot, int cap, size_t n_rows) {
  const size_t row = blockIdx.y;
  for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < cap; j += gridDim.x * blockDim.x) slot[row * cap + j] = j;
  (void)n_rows;
}

// easykv/easykv.py:242-245 (mode 0), :412-416 (modes 1, 2)
__global__ void ekv_state_init_kernel(float* s, float* q, float* c, int cap, int width, int mode, int stride,
                                      size_t row0) {
  const size_t row = row0 + blockIdx.y;
  for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < cap; j += gridDim.x * blockDim.x) {
    float cv = 0.f;
    if (j < width) {
      if (mode == 0) cv = (float)(width - 1 - j);
      else if (mode == 1) cv = (float)(width - j) - (float)stride;
      else cv = j < width - stride ? 0.f : -(float)(j - (width - stride));
    }
    s[row * cap + j] = 0.f;
    q[row * cap + j] = 0.f;
    c[row * cap + j] = cv;
  }
}

// one 16-byte lane per 8 halfs; rows of D halfs
template <bool GATHER>
__global__ void ekv_rows_copy_kernel(__half* bank_k, __half* bank_v, const int32_t* slot, __half* lin_k, __half* lin_v,
                                     int n_kv_heads, int cap, int D, int layer_begin, int pos_begin, int n) {
  const int h = blockIdx.y, ll = blockIdx.z;
  const size_t head_row = ((size_t)(layer_begin + ll) * n_kv_heads + h) * cap;
  const int lpr = D / 8;
  const int rows_per_block = blockDim.x / lpr;
  if ((int)threadIdx.x >= rows_per_block * lpr) return;      // (head_dim 96: 21 rows of 12 pieces per 256 threads)
  const int sub = threadIdx.x % lpr;
  for (int i = blockIdx.x * rows_per_block + threadIdx.x / lpr; i < n; i += gridDim.x * rows_per_block) {
    const int row = slot[head_row + pos_begin + i];
    uint4* bk = reinterpret_cast<uint4*>(bank_k + (head_row + row) * D) + sub;
    uint4* bv = reinterpret_cast<uint4*>(bank_v + (head_row + row) * D) + sub;
    uint4* lk = reinterpret_cast<uint4*>(lin_k + (((size_t)ll * n_kv_heads + h) * n + i) * D) + sub;
    uint4* lv = reinterpret_cast<uint4*>(lin_v + (((size_t)ll * n_kv_heads + h) * n + i) * D) + sub;
    if (GATHER) {
      *lk = *bk;
      *lv = *bv;
    } else {
      *bk = *lk;
      *bv = *lv;
    }
  }
}

// Reference-shaped physical compaction (easykv/easykv.py:56-82) in place, identity layout.  One workgroup per
// (tensor, head, layer).  Destination d >= first victim takes source d + #victims <= source: a forward memmove by 1 .. n_evict rows.
// Chunks of 256 / (D/8) * CH rows ascend; inside a chunk every thread has its source rows in registers before any thread
// stores (one barrier).  Nothing else needs ordering: chunk c+1 reads rows above everything chunk c writes, and chunk c+1's writes
// only reach rows chunk c had read before ITS barrier — so the loads of chunk c+1 are issued BEFORE the stores of chunk c
// (two register sets), no thread ever waits for a store to complete, and there is one barrier per chunk instead of two.
template <int CH, bool SINGLE>
__global__ void __launch_bounds__(256) ekv_compact_inplace_kernel(__half* k, __half* v, const int32_t* evict, int n_kv_heads,
                                                                  int cap, int D, int layer_begin, int n_slots, int n_evict) {
  extern __shared__ int32_t s_ev[];
  const int which = blockIdx.x, h = blockIdx.y, ll = blockIdx.z;
  char* base = reinterpret_cast<char*>((which == 0 ? k : v) + ((size_t)(layer_begin + ll) * n_kv_heads + h) * cap * D);
  for (int i = threadIdx.x; i < n_evict; i += 256) s_ev[i] = evict[((size_t)ll * n_kv_heads + h) * n_evict + i];
  __syncthreads();
  const int lpr = D / 8, rpb = 256 / lpr;
  const int tix = min((int)threadIdx.x, rpb * lpr - 1);      // (head_dim 96: the 4 threads past 21 rows x 12 pieces repeat the last piece)
  const int sub = tix % lpr, rg = tix / lpr;
  const int first = s_ev[0], n_keep = n_slots - n_evict;
  const int row_bytes = D * 2;
  // source row of destination d = d + #{e : ev[e] - e <= d} (ev ascending, so ev[e] - e is non-decreasing: a branch-free binary
  // search with a launch-uniform number of steps; the single-victim decode step needs none).  Rows past the end are clamped:
  // the loads are unconditional.
  int n_bits = 0;
  while ((1 << n_bits) < n_evict + 1) ++n_bits;
  auto src_of = [&](int d) __attribute__((always_inline)) {
    d = min(d, n_keep - 1);
    if (SINGLE) return d + 1;              // (d >= first; template parameter: no victim walk between the loads of a chunk)
    int cnt = 0;                           // largest cnt with ev[cnt - 1] - (cnt - 1) <= d
    for (int b = n_bits - 1; b >= 0; --b) {
      const int c = cnt + (1 << b);
      const int e = min(c, n_evict) - 1;
      cnt = (c <= n_evict && s_ev[e] - e <= d) ? c : cnt;
    }
    return d + cnt;
  };
  if (first >= n_keep) return;
  ekv_u4 ra[CH], rb[CH];      // two register sets, roles alternate (a copy nxt -> cur would wait for the look-ahead loads)
  const int step = rpb * CH;
  auto load = [&](ekv_u4 (&r)[CH], int d0) __attribute__((always_inline)) {
#pragma unroll
    for (int c = 0; c < CH; ++c) r[c] = __builtin_nontemporal_load(reinterpret_cast<const ekv_u4*>(base + (size_t)src_of(d0 + c * rpb + rg) * row_bytes + sub * 16));
  };
  auto store = [&](const ekv_u4 (&r)[CH], int d0) __attribute__((always_inline)) {
    // every thread's rows of THIS chunk have landed (the CH newer loads stay in flight), then the stores
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(CH) : "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      const int d = d0 + c * rpb + rg;
      if (d < n_keep) __builtin_nontemporal_store(r[c], reinterpret_cast<ekv_u4*>(base + (size_t)d * row_bytes + sub * 16));
    }
  };
  load(ra, first);
  for (int d0 = first; d0 < n_keep; d0 += 2 * step) {
    load(rb, d0 + step);
    store(ra, d0);
    load(ra, d0 + 2 * step);
    store(rb, d0 + step);
  }
}

// EKV_POLICY_RANGE ('recency' / 'random', easykv/easykv.py:343-362, :491-499, :105-112): every head of every layer drops the
// same contiguous positions [start, start + k).  Nothing is scored, so nothing needs LDS-resident rows: only the slot map is
// compacted — entries behind the range move down by k, the victims' rows become the free tail [T - k, T) — whatever the cache
// length.  One workgroup per (head, layer); chunks ascend and every chunk is read completely before it is written, and a
// chunk's sources lie at or beyond the next chunk's destinations, so no entry is overwritten before it has moved.
__global__ void __launch_bounds__(256) ekv_range_evict_kernel(int32_t* slot_of_pos, int32_t* evict_ids, int n_kv_heads, int cap,
                                                              int layer_begin, int T, int start, int k) {
  extern __shared__ int32_t s_vict[];
  const int h = blockIdx.x, ll = blockIdx.y, tid = threadIdx.x;
  int32_t* map = slot_of_pos + ((size_t)(layer_begin + ll) * n_kv_heads + h) * cap;
  for (int i = tid; i < k; i += 256) {
    s_vict[i] = map[start + i];
    if (evict_ids != nullptr) evict_ids[((size_t)ll * n_kv_heads + h) * k + i] = start + i;
  }
  __syncthreads();
  constexpr int CH = 8;
  for (int d0 = start; d0 < T - k; d0 += 256 * CH) {
    int32_t buf[CH];
#pragma unroll
    for (int c = 0; c < CH; ++c) buf[c] = map[min(d0 + c * 256 + tid + k, T - 1)];   // unconditional (clamped) loads
    __syncthreads();
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      const int d = d0 + c * 256 + tid;
      if (d < T - k) map[d] = buf[c];
    }
    __syncthreads();
  }
  for (int i = tid; i < k; i += 256) map[T - k + i] = s_vict[i];
}

// The same for a batched decode step (ekv_batch_step_attend): workgroup (head, entry) takes T, the range and the victim count from
// its entry of the table (scalar loads from the kernel arguments) and addresses the map by the entry's bank layer; an entry that
// evicts nothing this step leaves its map alone.  evict_ids rows are k_max (the table's largest n_evict) apart.
__global__ void __launch_bounds__(256) ekv_range_evict_batch_kernel(int32_t* slot_of_pos, int32_t* evict_ids, int n_kv_heads, int cap,
                                                                    int k_max, const EkvSeqTable tb) {
  extern __shared__ int32_t s_vict[];
  const int h = blockIdx.x, ll = blockIdx.y, tid = threadIdx.x;
  const int T = tb.e[ll].n_slots, start = tb.e[ll].range_start, k = tb.e[ll].n_evict;
  if (k == 0) return;
  int32_t* map = slot_of_pos + ((size_t)tb.e[ll].layer * n_kv_heads + h) * cap;
  for (int i = tid; i < k; i += 256) {
    s_vict[i] = map[start + i];
    if (evict_ids != nullptr) evict_ids[((size_t)ll * n_kv_heads + h) * k_max + i] = start + i;
  }
  __syncthreads();
  constexpr int CH = 8;
  for (int d0 = start; d0 < T - k; d0 += 256 * CH) {
    int32_t buf[CH];
#pragma unroll
    for (int c = 0; c < CH; ++c) buf[c] = map[min(d0 + c * 256 + tid + k, T - 1)];
    __syncthreads();
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      const int d = d0 + c * 256 + tid;
      if (d < T - k) map[d] = buf[c];
    }
    __syncthreads();
  }
  for (int i = tid; i < k; i += 256) map[T - k + i] = s_vict[i];
}

// ---- ordered <-> slot-indexed score rows (ekv_decode_tail.h, "slot-indexed score rows") ------------------------------------------
// One workgroup per (head, layer); everything is read into LDS before anything is written (the conversions are in place).
// to_slots: entry j of the ordered rows (row = slot_of_pos[j]) becomes S[row], Q[row], C0[row] = C[j] (g = 0), birth[row] = j; the
// next birth is n_slots.  Entries of the slot map below n_slots are dead afterwards; the free list [n_slots, cap) stays.
__global__ void __launch_bounds__(256) ekv_rows_to_slots_kernel(const int32_t* slot_of_pos, float* S, float* Q, float* Cn, int32_t* birth,
                                                                float* cnt_tail, float* slot_state, int n_kv_heads, int cap, int layer_begin, int T) {
  extern __shared__ float s_rows[];      // [4][T]
  const int h = blockIdx.x, ll = blockIdx.y, tid = threadIdx.x;
  const size_t head = (size_t)(layer_begin + ll) * n_kv_heads + h, head_row = head * cap;
  // the ordered count row's tail [T, cap) — what the next appended entries start from (zeros after decode steps, 0, -1, -2 ... after
  // a strided chunk step) — has no place in a row-indexed array: parked, and put back by ekv_rows_to_order
  for (int j = T + tid; j < cap; j += 256) cnt_tail[head_row + j] = Cn ? Cn[head_row + j] : 0.f;
  for (int j = tid; j < T; j += 256) {
    s_rows[j] = S[head_row + j];
    s_rows[T + j] = Q ? Q[head_row + j] : 0.f;
    s_rows[2 * T + j] = Cn ? Cn[head_row + j] : 0.f;
    reinterpret_cast<int32_t*>(s_rows)[3 * T + j] = slot_of_pos[head_row + j];
  }
  __syncthreads();
  for (int j = tid; j < T; j += 256) {
    const int row = reinterpret_cast<const int32_t*>(s_rows)[3 * T + j];
    S[head_row + row] = s_rows[j];
    if (Q) Q[head_row + row] = s_rows[T + j];
    if (Cn) Cn[head_row + row] = s_rows[2 * T + j];
    birth[head_row + row] = j;
  }
  if (tid == 0) {
    slot_state[4 * head] = 0.f;
    reinterpret_cast<int32_t*>(slot_state)[4 * head + 1] = T;
    reinterpret_cast<uint32_t*>(slot_state)[4 * head + 2] = 0u;      // no threshold hint yet
    reinterpret_cast<uint32_t*>(slot_state)[4 * head + 3] = 0u;
  }
}

// to_order: the live rows are the rows that are not on the free list [T, cap); the order index of a row is the rank of its birth
// among them (counted: births are unique).  Rebuilds slot_of_pos[0, T), S / Q / C (C = C0 + g) in order, zero tails.
__global__ void __launch_bounds__(256) ekv_rows_to_order_kernel(int32_t* slot_of_pos, float* S, float* Q, float* Cn, const int32_t* birth,
                                                                const float* cnt_tail, const float* slot_state, int n_kv_heads, int cap, int layer_begin, int T) {
  extern __shared__ float s_rows[];      // [4][cap]: S, Q, C0, birth (-1 = not live)
  const int h = blockIdx.x, ll = blockIdx.y, tid = threadIdx.x;
  const size_t head = (size_t)(layer_begin + ll) * n_kv_heads + h, head_row = head * cap;
  int32_t* s_b = reinterpret_cast<int32_t*>(s_rows) + 3 * (size_t)cap;
  const float g = slot_state[4 * head];
  for (int r = tid; r < cap; r += 256) {
    s_rows[r] = S[head_row + r];
    s_rows[cap + r] = Q ? Q[head_row + r] : 0.f;
    s_rows[2 * cap + r] = Cn ? Cn[head_row + r] : 0.f;
    s_b[r] = birth[head_row + r];
  }
  __syncthreads();
  for (int i = T + tid; i < cap; i += 256) s_b[slot_of_pos[head_row + i]] = -1;      // the free list: distinct rows
  __syncthreads();
  for (int r = tid; r < cap; r += 256) {
    const int b = s_b[r];
    if (b >= 0) {
      int rank = 0;
      for (int x = 0; x < cap; ++x) {
        const int bx = s_b[x];
        rank += (bx >= 0 && bx < b) ? 1 : 0;
      }
      slot_of_pos[head_row + rank] = r;
      S[head_row + rank] = s_rows[r];
      if (Q) Q[head_row + rank] = s_rows[cap + r];
      if (Cn) Cn[head_row + rank] = s_rows[2 * cap + r] + g;
    }
  }
  // tails: S / Q are zero behind the live entries in every flow; the count tail is the parked one (an evicting slot-layout step
  // has zeroed its front entry, like the ordered step does)
  for (int j = T + tid; j < cap; j += 256) {
    S[head_row + j] = 0.f;
    if (Q) Q[head_row + j] = 0.f;
    if (Cn) Cn[head_row + j] = cnt_tail[head_row + j];
  }
}

}  // namespace

hipError_t ekv_launch_bank_reset(const ekv_bank* bank, hipStream_t s) {
  const size_t rows = (size_t)bank->n_layers * bank->n_kv_heads;
  hipLaunchKernelGGL(ekv_iota_rows_kernel, dim3((bank->cap + 255) / 256, (unsigned)rows), dim3(256), 0, s, bank->slot_of_pos, bank->cap, rows);
  if (bank->arrive != nullptr) {
    const hipError_t e = hipMemsetAsync(bank->arrive, 0, rows * 4, s);
    if (e != hipSuccess) return e;
  }
  return hipGetLastError();
}

hipError_t ekv_launch_state_init(const ekv_bank* bank, int layer_begin, int layer_count, int width, int mode, int stride, hipStream_t s) {
  const size_t row0 = (size_t)layer_begin * bank->n_kv_heads;
  hipLaunchKernelGGL(ekv_state_init_kernel, dim3((bank->cap + 255) / 256, layer_count * bank->n_kv_heads), dim3(256), 0, s, bank->score_sum,
                     bank->score_sq, bank->score_cnt, bank->cap, width, mode, stride, row0);
  return hipGetLastError();
}

hipError_t ekv_launch_rows_copy(const ekv_bank* bank, bool gather, int layer_begin, int layer_count, int pos_begin, int n, void* k_lin, void* v_lin,
                                hipStream_t s) {
  const int rpb = 256 / (bank->head_dim / 8);
  hipLaunchKernelGGL((gather ? ekv_rows_copy_kernel<true> : ekv_rows_copy_kernel<false>), dim3((n + rpb - 1) / rpb, bank->n_kv_heads, layer_count),
                     dim3(256), 0, s, static_cast<__half*>(bank->k), static_cast<__half*>(bank->v), bank->slot_of_pos, static_cast<__half*>(k_lin),
                     static_cast<__half*>(v_lin), bank->n_kv_heads, bank->cap, bank->head_dim, layer_begin, pos_begin, n);
  return hipGetLastError();
}

hipError_t ekv_launch_compact_inplace(const ekv_bank* bank, int layer_begin, int layer_count, int n_slots, int n_evict, const int32_t* evict_ids,
                                      hipStream_t s) {
  static const int ch = [] { const char* e = std::getenv("EKV_COMPACT_CH"); return e ? std::atoi(e) : 16; }();   // (tuning knob; 4 / 8 / 16 rows per thread in flight: 4.3 / 4.5 / 4.65 TB/s)
#define EKV_CI(CHV) hipLaunchKernelGGL((n_evict == 1 ? ekv_compact_inplace_kernel<CHV, true> : ekv_compact_inplace_kernel<CHV, false>), dim3(2, bank->n_kv_heads, layer_count), dim3(256), (size_t)n_evict * 4, \
                     s, static_cast<__half*>(bank->k), static_cast<__half*>(bank->v),                      \
                     evict_ids, bank->n_kv_heads, bank->cap, bank->head_dim, layer_begin, n_slots, n_evict)
  if (ch <= 2) EKV_CI(2); else if (ch <= 4) EKV_CI(4); else if (ch <= 8) EKV_CI(8); else EKV_CI(16);
#undef EKV_CI
  return hipGetLastError();
}

hipError_t ekv_launch_range_evict(const ekv_bank* bank, const ekv_step* st, const EkvSeqTable* tb, int32_t* evict_ids, hipStream_t s) {
  const dim3 grid(bank->n_kv_heads, st->layer_count);
  if (tb)
    hipLaunchKernelGGL(ekv_range_evict_batch_kernel, grid, dim3(256), (size_t)st->n_evict * 4, s, bank->slot_of_pos, evict_ids, bank->n_kv_heads,
                       bank->cap, st->n_evict, *tb);
  else
    hipLaunchKernelGGL(ekv_range_evict_kernel, grid, dim3(256), (size_t)st->n_evict * 4, s, bank->slot_of_pos, evict_ids, bank->n_kv_heads,
                       bank->cap, st->layer_begin, st->n_slots, st->range_start, st->n_evict);
  return hipGetLastError();
}

hipError_t ekv_launch_rows_to_slots(const ekv_bank* bank, int layer_begin, int layer_count, int n_slots, size_t lds, hipStream_t s) {
  if (lds > 48 * 1024) (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&ekv_rows_to_slots_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL(ekv_rows_to_slots_kernel, dim3(bank->n_kv_heads, layer_count), dim3(256), lds, s, bank->slot_of_pos, bank->score_sum,
                     bank->score_sq, bank->score_cnt, bank->birth, ekv_cnt_tail(bank), bank->slot_state, bank->n_kv_heads, bank->cap, layer_begin, n_slots);
  return hipGetLastError();
}

hipError_t ekv_launch_rows_to_order(const ekv_bank* bank, int layer_begin, int layer_count, int n_slots, size_t lds, hipStream_t s) {
  if (lds > 48 * 1024) (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&ekv_rows_to_order_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL(ekv_rows_to_order_kernel, dim3(bank->n_kv_heads, layer_count), dim3(256), lds, s, bank->slot_of_pos, bank->score_sum,
                     bank->score_sq, bank->score_cnt, bank->birth, ekv_cnt_tail(bank), bank->slot_state, bank->n_kv_heads, bank->cap, layer_begin, n_slots);
  return hipGetLastError();
}
