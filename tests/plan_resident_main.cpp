// The resident rows of the one-launch decode step as a stand-alone host program: links easykv_amd/csrc/ekv_plan.cpp and nothing else of
// the library, so that the byte rule (ekv_decode_resident_rows), the budget setter and the way the value travels in the plan run under a
// sanitizer (tests/test_resident_plan.py builds it with -fsanitize=address,undefined).  Nothing is dereferenced behind a descriptor's
// pointers and nothing is launched.
//
//   plan_resident_main     no input.  Sweeps heads x extents x budgets and checks, for the rule: a multiple of 32, resident bytes within
//                          the budget, 32 more rows would exceed the budget or the rounded extent, budget 0 -> 0, everything fits -> the
//                          rounded extent; for the plan of a slot-indexed decode step of that geometry: the value packed into the kernel
//                          argument is the rule's, the ten ekv_step_info fields are those of budget 0, and the RoPE-on-read, quantised
//                          and batched calls of the geometry plan 0.
//                          Output: "F heads extent cap score_rows budget rows" per rule call, "P heads extent budget rows one_launch
//                          info[0..9]" per planned step, "OK <checks>" last; exit status 1 with a line "FAIL ..." on the first miss.
#include <cmath>
#include <cstdio>
#include <cstdlib>

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

int64_t resident_bytes(int64_t heads, int64_t row_bytes, int cap, int score_rows, int rows) {
  return heads * (2 * rows * row_bytes + 4 * (int64_t)cap * (score_rows + 2));
}
}  // namespace

int main() {
  const int kHeads[] = {32, 512, 544, 1024, 1600};
  const int kExtents[] = {1, 31, 32, 328, 2049, 2304, 6144};
  const int64_t kMB = 1 << 20;
  const int64_t kBudgets[] = {0, 1 * kMB, 64 * kMB, 220 * kMB, (int64_t)1 << 40};
  const int64_t row_bytes = 256;
  long n_resident = 0;
  for (int heads : kHeads)
    for (int ext : kExtents) {
      const int cap = (ext + 63 + 63) / 64 * 64;
      const int ext32 = (ext + 31) / 32 * 32;
      for (int score_rows : {1, 3})
        for (int64_t budget : kBudgets) {
          const int r = ekv_decode_resident_rows(heads, row_bytes, ext, cap, score_rows, budget);
          std::printf("F %d %d %d %d %lld %d\n", heads, ext, cap, score_rows, (long long)budget, r);
          CHECK(r >= 0 && r % 32 == 0 && r <= ext32, "rows %d", r);
          CHECK(r == 0 || resident_bytes(heads, row_bytes, cap, score_rows, r) <= budget, "rows %d over the budget", r);
          CHECK(r == ext32 || resident_bytes(heads, row_bytes, cap, score_rows, r + 32) > budget, "rows %d: 32 more fit", r);
          if (budget == 0) CHECK(r == 0, "budget 0 -> %d", r);
          if (resident_bytes(heads, row_bytes, cap, score_rows, ext32) <= budget) CHECK(r == ext32, "everything fits -> %d of %d", r, ext32);
          CHECK(EKV_RESIDENT_ROWS(EKV_RESIDENT_BITS(r) | 0xF04F) == r && ((EKV_RESIDENT_BITS(r) | 0xF04F) & 0xFFFF) == 0xF04F, "pack %d", r);
        }
      // the plan of a slot-indexed roco decode step of that geometry: H = 32 heads x heads / 32 layers, T = the extent
      ekv_bank bank{};
      bank.head_dim = 128, bank.n_q_heads = bank.n_kv_heads = 32, bank.n_layers = heads / 32, bank.cap = cap;
      bank.k = bank.v = kDummy;
      bank.slot_of_pos = static_cast<int32_t*>(kDummy);
      bank.score_sum = bank.score_sq = bank.score_cnt = bank.slot_state = static_cast<float*>(kDummy);
      bank.birth = static_cast<int32_t*>(kDummy);
      bank.arrive = static_cast<uint32_t*>(kDummy);
      ekv_step st{};
      st.layer_count = bank.n_layers, st.q_len = 1, st.n_slots = ext, st.policy = EKV_POLICY_ROCO, st.accumulate = 1, st.causal = 1;
      st.n_evict = ext > 1 ? 1 : 0, st.roco_k1 = ext > 1 ? (ext + 1) / 2 : 0, st.phases = EKV_PHASE_SLOT_ROWS;
      st.n_split = 1;      // (unsplit heads, as a caller asks who wants the one-launch step from a launch of < 1024 heads)
      st.count_add = 1.f, st.sm_div = std::sqrt(128.f), st.phys_extent = ext;
      int32_t info0[EKV_STEP_INFO_N];
      for (int64_t budget : kBudgets) {
        ekv_resident_set_budget_bytes(budget);
        CHECK(ekv_resident_budget_bytes() == budget, "the setter");
        for (int32_t dtype : {EKV_DTYPE_F16, EKV_DTYPE_BF16}) {
          const EkvCall c = step_call(&bank, &st, dtype);
          EkvResolved r;
          const int rc = resolve_call(c, &r);
          int32_t info[EKV_STEP_INFO_N];
          CHECK(call_info(c, info, EKV_STEP_INFO_N) == EKV_OK, "call_info");
          const bool fused = rc == EKV_OK && r.plan.one_launch && r.plan.n_list == 1 && r.plan.list[0].kind == EKV_RUN_FUSED_DECODE;
          const int rows = call_resident_rows(c);
          if (dtype == EKV_DTYPE_F16) {
            std::printf("P %d %d %lld %d %d", heads, ext, (long long)budget, rows, fused ? 1 : 0);
            for (int32_t x : info) std::printf(" %d", x);
            std::printf("\n");
          }
          if (budget == 0 && dtype == EKV_DTYPE_F16)
            for (int i = 0; i < EKV_STEP_INFO_N; ++i) info0[i] = info[i];
          for (int i = 0; i < EKV_STEP_INFO_N; ++i) CHECK(info[i] == info0[i], "info[%d] = %d under budget %lld, %d under 0", i, info[i], (long long)budget, info0[i]);
          if (fused) {
            // the kernel argument (ekv_abi.hip copies the plan's word): the rule's value round-trips, the order bits below it are untouched
            const int want = ekv_decode_resident_rows(heads, row_bytes, r.plan.phys_extent, cap, 3, budget);
            CHECK(EKV_RESIDENT_ROWS(r.plan.fused_order) == want && rows == want, "planned %d, rule %d", rows, want);
            CHECK((r.plan.fused_order & 3) == info[9] && (r.plan.fused_order >> 24) == 0, "order bits %x", r.plan.fused_order);
            n_resident += want > 0;
          } else {
            CHECK(rows == 0, "a step that is not the one-launch decode step plans %d", rows);
          }
          if (budget == 0) CHECK(rows == 0, "budget 0 plans %d", rows);
        }
        // the calls that keep their code: RoPE-on-read (ordered rows), the quantised formats, a batch
        ekv_step ro = st;
        ro.rope_on_read = 1, ro.phases = 0;
        CHECK(call_resident_rows(step_call(&bank, &ro, EKV_DTYPE_F16)) == 0, "RoPE-on-read");
        ekv_step od = st;
        od.phases = 0;
        const ekv_kv8 q8{kDummy, kDummy, static_cast<float*>(kDummy), static_cast<float*>(kDummy)};
        const ekv_kv4 q4{kDummy, kDummy, static_cast<uint8_t*>(kDummy), static_cast<uint8_t*>(kDummy)};
        const ekv_kv6 q6{kDummy, kDummy, static_cast<uint8_t*>(kDummy), static_cast<uint8_t*>(kDummy)};
        for (const ekv_step* s : {&st, &od}) {
          CHECK(call_resident_rows(kv8_call(&bank, s, EKV_DTYPE_F16, &q8)) == 0, "kv8");
          CHECK(call_resident_rows(kv4_call(&bank, s, EKV_DTYPE_F16, &q4)) == 0, "kv4");
          CHECK(call_resident_rows(kv6_call(&bank, s, EKV_DTYPE_BF16, &q6)) == 0, "kv6");
        }
        const int n_seq = bank.n_layers < EKV_MAX_SEQS ? bank.n_layers : EKV_MAX_SEQS;
        ekv_seq seqs[EKV_MAX_SEQS];
        for (int i = 0; i < n_seq; ++i) seqs[i] = ekv_seq{i, ext, 0, st.n_evict, 0, 0, st.roco_k1, 0, ext};
        CHECK(call_resident_rows(batch_call(&bank, &od, EKV_DTYPE_F16, seqs, n_seq)) == 0, "batch");
        CHECK(call_resident_rows(kv8_batch_call(&bank, &od, EKV_DTYPE_F16, &q8, seqs, n_seq)) == 0, "kv8 batch");
      }
      ekv_resident_set_budget_bytes(-1);
    }
  CHECK(n_resident > 0, "no planned step had resident rows");
  std::printf("OK %ld\n", n_checks);
  return 0;
}
