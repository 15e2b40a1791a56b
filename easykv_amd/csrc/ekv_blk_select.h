// Workgroup-wide reductions and the exact "k smallest" selection of the scorers, over a key array given by pointer (LDS in the generic
// scorer and the kernel tails, global scratch in the long-row scorer: ekv_score_long.inc).  Included inside the anonymous namespace of
// a kernel source, after it has defined  constexpr int kNT  (threads per workgroup) and  kNWV = kNT / 64.
//
// Selection is exact and deterministic: "k smallest" is an MSB-first radix select (8 bits per pass) on order-preserving uint32 keys
// (no sort); ties go to the lowest index, NaN ranks largest.

struct Blk {
  int tid, lane, wave;
  unsigned long long* red;  // 2 * kNWV entries
  int phase;
};

__device__ __forceinline__ float blk_max(Blk& b, float x) {
  x = ekv_wave_max(x);
  float* r = reinterpret_cast<float*>(b.red) + (b.phase & 1) * kNWV * 2;
  if (b.lane == 0) r[b.wave] = x;
  __syncthreads();
  float y = r[0];
  for (int i = 1; i < kNWV; ++i) y = fmaxf(y, r[i]);
  b.phase++;
  return y;
}
__device__ __forceinline__ float blk_sum(Blk& b, float x) {
  x = ekv_wave_sum(x);
  float* r = reinterpret_cast<float*>(b.red) + (b.phase & 1) * kNWV * 2;
  if (b.lane == 0) r[b.wave] = x;
  __syncthreads();
  float y = 0.f;
  for (int i = 0; i < kNWV; ++i) y += r[i];
  b.phase++;
  return y;
}
__device__ __forceinline__ int blk_sum_uniform(Blk& b, int wave_value) {  // value already wave-uniform
  int* r = reinterpret_cast<int*>(b.red) + (b.phase & 1) * kNWV * 2;
  if (b.lane == 0) r[b.wave] = wave_value;
  __syncthreads();
  int y = 0;
  for (int i = 0; i < kNWV; ++i) y += r[i];
  b.phase++;
  return y;
}
__device__ __forceinline__ unsigned long long blk_min_u64(Blk& b, unsigned long long x) {
  x = ekv_wave_min_u64(x);
  unsigned long long* r = b.red + (b.phase & 1) * kNWV;
  if (b.lane == 0) r[b.wave] = x;
  __syncthreads();
  unsigned long long y = r[0];
  for (int i = 1; i < kNWV; ++i) y = r[i] < y ? r[i] : y;
  b.phase++;
  return y;
}

// #{ j < n : pred(key[j], j) }, pred evaluated by every thread on a strided sweep
template <typename P>
__device__ __forceinline__ int blk_count(Blk& b, const uint32_t* key, int n, P pred) {
  int c = 0;
  const int n_round = (n + kNT - 1) / kNT * kNT;
  for (int j = b.tid; j < n_round; j += kNT) {
    const bool p = j < n && pred(key[j], j);
    c += __popcll(__ballot(p));
  }
  return blk_sum_uniform(b, c);
}

// k-th smallest key (1-indexed): MSB-first radix select, 8 bits per pass (4 passes, 2 barriers each).  Per pass: a
// 256-bin LDS histogram of the keys that still match the prefix (ds_add), then wave 0 scans the bins, publishes
// (bin, keys below it, keys in it) and clears the histogram for the next pass.  Also returns how many keys are smaller
// than / equal to the result, so the caller needs no extra counting sweeps.  Exact; no sort.
__device__ uint32_t blk_kth(Blk& b, const uint32_t* key, int n, int k, uint32_t* hist /* 256 + 3 words of LDS */,
                            int& n_less, int& n_eq) {
  uint32_t prefix = 0;
  int kk = k;   // rank still to find among the keys matching `prefix`
  int less = 0, eq = 0;
  for (int i = b.tid; i < 256; i += kNT) hist[i] = 0;
  __syncthreads();
  for (int shift = 24; shift >= 0; shift -= 8) {
    const uint32_t hi_mask = shift == 24 ? 0u : (0xFFFFFFFFu << (shift + 8));
    for (int j = b.tid; j < n; j += kNT) {
      const uint32_t x = key[j];
      if ((x & hi_mask) == prefix) atomicAdd(&hist[(x >> shift) & 255u], 1u);
    }
    __syncthreads();
    if (b.wave == 0) {
      const uint32_t c0 = hist[4 * b.lane], c1 = hist[4 * b.lane + 1], c2 = hist[4 * b.lane + 2], c3 = hist[4 * b.lane + 3];
      hist[4 * b.lane] = hist[4 * b.lane + 1] = hist[4 * b.lane + 2] = hist[4 * b.lane + 3] = 0;   // ready for the next pass
      const uint32_t mine = c0 + c1 + c2 + c3;
      uint32_t incl = mine;
      for (int o = 1; o < 64; o <<= 1) {
        const uint32_t y = __shfl_up(incl, o, 64);
        if (b.lane >= o) incl += y;
      }
      const uint32_t excl = incl - mine;
      if ((uint32_t)kk > excl && (uint32_t)kk <= incl) {   // exactly one lane owns the kk-th key
        uint32_t below = excl, bin = 4 * b.lane, cnt = c0;
        if ((uint32_t)kk > below + c0) { below += c0; bin++; cnt = c1;
          if ((uint32_t)kk > below + c1) { below += c1; bin++; cnt = c2;
            if ((uint32_t)kk > below + c2) { below += c2; bin++; cnt = c3; } } }
        hist[256] = bin;
        hist[257] = below;
        hist[258] = cnt;
      }
    }
    __syncthreads();
    prefix |= hist[256] << shift;
    kk -= (int)hist[257];
    less += (int)hist[257];
    eq = (int)hist[258];
    // (hist[256..258] are rewritten only after the next pass's barrier, by which time every thread has read them)
  }
  n_less = less;
  n_eq = eq;
  return prefix;
}

// block-wide minimum of two independent uint32 values in one barrier
__device__ __forceinline__ void blk_min2_u32(Blk& b, uint32_t& x, uint32_t& y) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    x = min(x, (uint32_t)__shfl_xor((int)x, off, 64));
    y = min(y, (uint32_t)__shfl_xor((int)y, off, 64));
  }
  uint32_t* r = reinterpret_cast<uint32_t*>(b.red + (b.phase & 1) * kNWV);
  if (b.lane == 0) {
    r[b.wave * 2] = x;
    r[b.wave * 2 + 1] = y;
  }
  __syncthreads();
  for (int i = 0; i < kNWV; ++i) {
    x = min(x, r[i * 2]);
    y = min(y, r[i * 2 + 1]);
  }
  b.phase++;
}

// Exclusive threshold `thr` on the pairs (key << 32 | j) such that exactly k pairs lie below it — the k smallest keys, ties
// to the lower index — or 0 if this fast path does not apply.  Keys >= `sent` (sentinels, NaN) are kept out of the range.
// Five barriers instead of the radix select's eight plus tie handling: range of the real keys, one 256-bin histogram over
// that range (score keys sit in a narrow band of exponents, so MSB-first digits would waste their first passes), the bin
// that holds rank k - 1, and its members (<= cap) ranked against each other.
__device__ unsigned long long blk_thr_hist(Blk& b, const uint32_t* key, int n, int k, uint32_t sent, uint32_t* hist /* 264 words */,
                                           unsigned long long* list, int cap) {
  uint32_t kmin = ~0u, nmax = ~0u;   // nmax = ~max
  for (int j = b.tid; j < n; j += kNT) {
    const uint32_t x = key[j];
    if (x < sent) {
      kmin = min(kmin, x);
      nmax = min(nmax, ~x);
    }
  }
  for (int i = b.tid; i < 264; i += kNT) hist[i] = 0;   // [256] members listed, [257] bin, [258] below, [260..261] result
  blk_min2_u32(b, kmin, nmax);                           // (its barrier also publishes the zeroed histogram)
  const uint32_t kmax = ~nmax;
  if (kmin > kmax) return 0;                             // no real key at all
  const uint32_t range = kmax - kmin;
  const int shift = range < 256u ? 0 : 24 - __clz(range);   // range >> shift < 256
  auto bin_of = [&](uint32_t x) { return x >= sent ? 255u : min(255u, (x - kmin) >> shift); };
  for (int j = b.tid; j < n; j += kNT) atomicAdd(&hist[bin_of(key[j])], 1u);
  __syncthreads();
  if (b.wave == 0) {                 // lane l owns bins 4l .. 4l+3; inclusive scan over the lanes
    const uint32_t c0 = hist[4 * b.lane], c1 = hist[4 * b.lane + 1], c2 = hist[4 * b.lane + 2], c3 = hist[4 * b.lane + 3];
    const uint32_t mine = c0 + c1 + c2 + c3;
    uint32_t incl = mine;
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t up = __shfl_up(incl, o, 64);
      if (b.lane >= o) incl += up;
    }
    const uint32_t excl = incl - mine, kk = (uint32_t)k;
    if (excl < kk && kk <= incl) {   // exactly one lane: the bin where the cumulative count reaches k
      uint32_t below = excl, bin = 4 * b.lane;
      if (below + c0 < kk) { below += c0; ++bin;
        if (below + c1 < kk) { below += c1; ++bin;
          if (below + c2 < kk) { below += c2; ++bin; } } }
      hist[257] = bin;
      hist[258] = below;
    }
  }
  __syncthreads();
  const uint32_t b_sel = hist[257], below = hist[258], in_bin = hist[b_sel];
  if ((int)in_bin > cap || (int)in_bin > kNT) {
    __syncthreads();                 // everyone has read the header before the caller's fallback reuses `hist`
    return 0;
  }
  for (int j = b.tid; j < n; j += kNT) {
    const uint32_t x = key[j];
    if (bin_of(x) == b_sel) list[atomicAdd(&hist[256], 1u)] = ((unsigned long long)x << 32) | (uint32_t)j;
  }
  __syncthreads();
  if (b.tid < (int)in_bin) {
    const unsigned long long e = list[b.tid];
    uint32_t rank = 0;
    for (int i = 0; i < (int)in_bin; ++i) rank += list[i] < e ? 1u : 0u;
    if (below + rank == (uint32_t)k - 1u) *reinterpret_cast<unsigned long long*>(hist + 260) = e + 1ull;
  }
  __syncthreads();
  const unsigned long long thr = *reinterpret_cast<const unsigned long long*>(hist + 260);
  __syncthreads();                   // (read before anybody zeroes `hist` again)
  return thr;
}

// key[j] <- 1 for the k smallest (key, index) pairs, 0 otherwise
// (`list_cap`: entries of the candidate list that follows the 264 histogram words; kNT by default)
__device__ void blk_mark_k_smallest(Blk& b, uint32_t* key, int n, int k, uint32_t* hist, uint32_t sent = 0xFFFFFFFFu, int list_cap = kNT) {
  uint32_t tau;
  int bound = n;
  if (k > 1) {
    unsigned long long* list = reinterpret_cast<unsigned long long*>(hist + 264);
    const unsigned long long thr = blk_thr_hist(b, key, n, k, sent, hist, list, list_cap);
    if (thr != 0) {
      for (int j = b.tid; j < n; j += kNT) key[j] = ((((unsigned long long)key[j]) << 32) | (uint32_t)j) < thr ? 1u : 0u;
      __syncthreads();
      return;
    }
  }
  if (k == 1) {
    unsigned long long best = ~0ull;
    for (int j = b.tid; j < n; j += kNT) {
      const unsigned long long x = ((unsigned long long)key[j] << 32) | (uint32_t)j;
      best = x < best ? x : best;
    }
    best = blk_min_u64(b, best);
    tau = (uint32_t)(best >> 32);
    bound = (int)(best & 0xFFFFFFFFu) + 1;
  } else {
    int n_less, n_eq;
    tau = blk_kth(b, key, n, k, hist, n_less, n_eq);
    const int need = k - n_less;
    if (n_eq != need) {  // ties at the threshold: lowest indices first
      int lo = 0, hi = n;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        const int c = blk_count(b, key, n, [tau, mid](uint32_t x, int j) { return x == tau && j < mid; });
        if (c >= need) hi = mid; else lo = mid + 1;
      }
      bound = lo;
    }
  }
  __syncthreads();
  for (int j = b.tid; j < n; j += kNT) {
    const uint32_t x = key[j];
    key[j] = (x < tau || (x == tau && j < bound)) ? 1u : 0u;
  }
  __syncthreads();
}
