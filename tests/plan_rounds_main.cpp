// The wave count and the phase-order word of the one-launch decode step as a stand-alone host program: links
// easykv_amd/csrc/ekv_plan.cpp and nothing else of the library (tests/test_rounds_plan.py builds it with -fsanitize=address,undefined
// and runs it once per setting of the knobs, which the planner reads once per process).  Nothing is dereferenced behind a descriptor's
// pointers and nothing is launched.
//
//   plan_rounds_main     no input.  Plans a decode step of every head count x step kind below and prints, per step,
//                        "W kind heads rc one_launch nw word info9"; checks on the way what holds under every setting: the low two bits
//                        of the word are the ekv_step_info field, bits 24-31 are zero, a word of rule source 3 belongs to an 8-wave
//                        plan and its threshold round-trips through EKV_ORDER_ROUND_BITS, and the packing macros invert each other.
//                        "OK <checks>" last; exit status 1 with a line "FAIL ..." on the first miss.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>

#include "../easykv_amd/csrc/ekv_plan.h"

namespace {
void* const kDummy = reinterpret_cast<void*>(256);      // (non-null, never dereferenced)
long n_checks = 0;
#define CHECK(cond, ...)                      \
  do {                                        \
    ++n_checks;                               \
    if (!(cond)) {                            \
      std::printf("FAIL %s: ", #cond);        \
      std::printf(__VA_ARGS__);               \
      std::printf("\n");                      \
      std::exit(1);                           \
    }                                         \
  } while (0)
}  // namespace

int main() {
  for (int wgs = 0; wgs <= 2040; wgs += 8) {
    const int bits = EKV_ORDER_ROUND_BITS(wgs);
    CHECK(EKV_ORDER_ROUND_THRESHOLD(bits) == wgs && (bits & ~0xFF00) == 0, "threshold %d -> %x -> %d", wgs, bits, EKV_ORDER_ROUND_THRESHOLD(bits));
    CHECK(EKV_ORDER_ROUND_THRESHOLD(bits | 0xFF00FF) == wgs, "threshold %d next to other fields", wgs);
  }
  CHECK(EKV_ORDER_ROUND_THRESHOLD(EKV_ORDER_ROUND_BITS(100000)) == 2040, "the threshold saturates");
  const int kLayers[] = {1, 7, 8, 16, 17, 18, 32, 40, 50};      // x 32 (or 40) heads: 32 .. 1600 heads in the launch
  const char* kKinds[] = {"roco", "h2o", "tova", "unscored", "gqa", "d64", "rope", "ordered", "cols12", "wide", "heads40", "kv8", "batch", "sink", "cap"};
  for (const char* kind : kKinds)
    for (int layers : kLayers) {
      const std::string k = kind;
      ekv_bank bank{};
      const int h = k == "heads40" ? 40 : 32;
      const int ext = k == "cols12" ? 3008 : (k == "wide" ? 6208 : 2112), T = ext - 63;
      bank.head_dim = k == "d64" ? 64 : 128, bank.n_kv_heads = h, bank.n_q_heads = k == "gqa" ? 2 * h : h, bank.n_layers = layers, bank.cap = ext;
      bank.k = bank.v = kDummy;
      bank.slot_of_pos = static_cast<int32_t*>(kDummy);
      bank.score_sum = bank.score_sq = bank.score_cnt = bank.slot_state = static_cast<float*>(kDummy);
      bank.birth = static_cast<int32_t*>(kDummy);
      bank.arrive = static_cast<uint32_t*>(kDummy);
      ekv_step st{};
      st.layer_count = layers, st.q_len = 1, st.n_slots = T, st.accumulate = 1, st.causal = 1, st.n_split = 1;
      st.policy = k == "h2o" ? EKV_POLICY_H2O_HEAD : (k == "tova" ? EKV_POLICY_TOVA : (k == "unscored" ? EKV_POLICY_NONE : EKV_POLICY_ROCO));
      st.n_evict = k == "unscored" ? 0 : 1, st.roco_k1 = T / 2, st.win_tail = k == "h2o" ? 100 : 0;
      st.phases = (k == "rope" || k == "ordered" || k == "batch") ? 0 : EKV_PHASE_SLOT_ROWS;
      st.rope_on_read = k == "rope" ? 1 : 0;
      st.count_add = 1.f, st.sm_div = std::sqrt((float)bank.head_dim), st.phys_extent = ext;
      const ekv_kv8 q8{kDummy, kDummy, static_cast<float*>(kDummy), static_cast<float*>(kDummy)};
      ekv_seq seqs[EKV_MAX_SEQS];
      const int n_seq = layers < EKV_MAX_SEQS ? layers : EKV_MAX_SEQS;
      for (int i = 0; i < n_seq; ++i) seqs[i] = ekv_seq{i, T, 0, st.n_evict, 0, 0, st.roco_k1, 0, ext};
      const EkvCall c = k == "kv8" ? kv8_call(&bank, &st, EKV_DTYPE_F16, &q8)
                      : k == "batch" ? batch_call(&bank, &st, EKV_DTYPE_F16, seqs, n_seq)
                      : k == "sink" ? sink_call(&bank, &st, EKV_DTYPE_F16, static_cast<const float*>(kDummy))
                      : k == "cap" ? cap_call(&bank, &st, EKV_DTYPE_F16, 30.f)
                                   : step_call(&bank, &st, EKV_DTYPE_F16);
      EkvResolved r;
      const int rc = resolve_call(c, &r);
      int32_t info[EKV_STEP_INFO_N];
      CHECK(call_info(c, info, EKV_STEP_INFO_N) == EKV_OK, "call_info %s %d", kind, layers);
      const int word = r.plan.fused_order, nw = r.plan.fused_nw;
      std::printf("W %s %d %d %d %d %d %d\n", kind, k == "batch" ? n_seq * h : layers * h, rc, r.plan.one_launch, nw, word, info[9]);
      if (rc != EKV_OK || !r.plan.one_launch) continue;
      CHECK((word & 3) == info[9], "%s %d: word %x, info %d", kind, layers, word, info[9]);
      CHECK((word >> 24) == 0, "%s %d: bits 24-31 of %x", kind, layers, word);
      CHECK(nw == 4 || nw == 8, "%s %d: %d waves", kind, layers, nw);
      if ((word & 3) == 1 && ((word >> 4) & 3) == 3) {
        CHECK(nw == 8, "%s %d: rule source 3 on %d waves", kind, layers, nw);
        const int t = EKV_ORDER_ROUND_THRESHOLD(word);
        CHECK(t % EKV_ORDER_ROUND_UNIT == 0 && (EKV_ORDER_ROUND_BITS(t) | (word & ~0xFF00)) == word, "%s %d: threshold %d of %x", kind, layers, t, word);
      }
      if ((word & 3) == 0) CHECK((word & 0xFFFF) == 0, "%s %d: rule bits in an all-F word %x", kind, layers, word);
    }
  std::printf("OK %ld\n", n_checks);
  return 0;
}
