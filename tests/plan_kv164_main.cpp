// The kv164 calls (16-bit keys with MXFP4 values) of the step planner as a stand-alone host program: links easykv_amd/csrc/ekv_plan.cpp and
// nothing else of the library, so that the stages resolve_call applies to an ekv_kv164_* call (the two planes and bank->k, envelope and
// table, plan, refusals) run on raw caller descriptors under a sanitizer (tests/test_batch_kv164_cpu.py builds it with
// -fsanitize=address,undefined).  Nothing is dereferenced behind a descriptor's pointers and nothing is launched.
//
//   plan_kv164_main   cases from stdin, one per line of integers, in the layout tests/plan_host_main.cpp reads:
//                            the KEYS of tests/test_dispatch_table.py, then  dtype plane nullmask batch n_seq  and, for a batch, 9
//                            integers per table entry (ekv_seq).  Every case is a kv164 call: ekv_kv164_batch_* with batch != 0, else
//                            ekv_kv164_step_*.
//                          nullmask bits: 1 bank, 2 step, 4 bank.k, 8 bank.v, 16 bank.slot_of_pos, 32 the kv164 descriptor, 64 plane
//                            `plane` (0 v_codes, 1 v_exp; any other index: none) of the descriptor, 128 the table.
//                          Output per case: check, info rc, the ten info fields, workspace bytes.
#include <cmath>
#include <cstdio>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "../easykv_amd/csrc/ekv_plan.h"

namespace {
void* const kDummy = reinterpret_cast<void*>(256);      // (what the Python tests pass: non-null, never dereferenced)
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::vector<long long> v;
    for (long long x; in >> x;) v.push_back(x);
    if (v.empty()) continue;
    if (v.size() < 43) return 2;
    auto at = [&](size_t i) { return i < v.size() ? (int32_t)v[i] : 0; };
    const int32_t dtype = at(38), plane = at(39), nulls = at(40), batch = at(41), n_seq = at(42);
    auto ptr = [&](bool on) { return on ? kDummy : nullptr; };
    ekv_bank bank{};
    bank.head_dim = at(0), bank.n_q_heads = at(1), bank.n_kv_heads = at(2), bank.n_layers = at(3), bank.cap = at(4);
    bank.arrive = static_cast<uint32_t*>(ptr(at(5)));
    bank.birth = static_cast<int32_t*>(ptr(at(6)));
    bank.slot_state = static_cast<float*>(ptr(at(6)));
    bank.score_sum = static_cast<float*>(ptr(at(7)));
    bank.score_sq = bank.score_cnt = static_cast<float*>(ptr(at(8)));
    bank.k = ptr(!(nulls & 4)), bank.v = ptr(!(nulls & 8)), bank.slot_of_pos = static_cast<int32_t*>(ptr(!(nulls & 16)));
    ekv_step st{};
    int32_t* const f[] = {&st.layer_begin, &st.layer_count, &st.q_len, &st.n_slots, &st.score_off, &st.policy, &st.accumulate, &st.n_evict,
                          &st.win_lo, &st.win_tail, &st.roco_k1, &st.roco_tail, &st.range_start, &st.tova_head_mean, &st.causal,
                          &st.rope_on_read, &st.n_split, &st.phases, nullptr, &st.two_pass, &st.phys_extent, &st.defer_layers,
                          &st.defer_index, &st.q_token_stride, &st.q_head_stride, &st.kv_token_stride, &st.kv_head_stride,
                          &st.out_token_stride, &st.out_head_stride};
    for (size_t i = 0; i < sizeof(f) / sizeof(f[0]); ++i)
      if (f[i]) *f[i] = at(9 + i);
    st.count_add = (float)(at(27) / 2.0), st.count_tail_step = st.q_len > 1 ? -1.f : 0.f, st.sm_div = (float)std::sqrt((double)bank.head_dim);
    auto pl = [&](int i) { return ptr(!((nulls & 64) && plane == i)); };
    ekv_kv164 q164{pl(0), static_cast<uint8_t*>(pl(1))};
    const size_t n_entries = (v.size() - 43) / 9;
    std::unique_ptr<ekv_seq[]> seqs(new ekv_seq[n_entries]);      // exactly the entries on the line: a read past them is the sanitizer's to report
    for (size_t e = 0, i = 43; e < n_entries; ++e, i += 9) seqs[e] = {at(i), at(i + 1), at(i + 2), at(i + 3), at(i + 4), at(i + 5), at(i + 6), at(i + 7), at(i + 8)};
    const ekv_bank* b = (nulls & 1) ? nullptr : &bank;
    const ekv_step* s = (nulls & 2) ? nullptr : &st;
    const ekv_kv164* q = (nulls & 32) ? nullptr : &q164;
    const EkvCall c = batch ? kv164_batch_call(b, s, dtype, q, (nulls & 128) ? nullptr : seqs.get(), n_seq) : kv164_call(b, s, dtype, q);
    int32_t info[EKV_STEP_INFO_N];
    for (int32_t& x : info) x = -7;
    const int check = call_check(c);
    const int irc = call_info(c, info, EKV_STEP_INFO_N);
    std::printf("%d %d", check, irc);
    for (int32_t x : info) std::printf(" %d", x);
    std::printf(" %zu\n", call_workspace_bytes(c));
  }
  return 0;
}
