// The long-row call family of the step planner as a stand-alone host program: links easykv_amd/csrc/ekv_plan.cpp and nothing else of
// the library, so that the code that takes raw caller descriptors can run under a sanitizer (tests/test_plan_long_host_cpu.py builds it
// with -fsanitize=address,undefined).  Nothing is dereferenced behind a descriptor's pointers and nothing is launched.
//
//   plan_long_host_main        cases from stdin, one per line of integers: the KEYS of tests/test_dispatch_table.py, then dtype nullmask
//                              nullmask bits: 1 bank, 2 step, 4 bank.k, 8 bank.v, 16 bank.slot_of_pos, 32 the info array, 64 n_info = 0.
//                              Output per case: check, info rc, the twelve info fields of ekv_long_step_info, workspace bytes.
#include <cmath>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../easykv_amd/csrc/ekv_plan.h"

int main() {
  void* const dummy = reinterpret_cast<void*>(256);      // (what the Python tests pass: non-null, never dereferenced)
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::vector<long long> v;
    for (long long x; in >> x;) v.push_back(x);
    if (v.empty()) continue;
    if (v.size() < 40) return 2;
    auto at = [&](size_t i) { return (int32_t)v[i]; };
    const int32_t dtype = at(38), nulls = at(39);
    auto ptr = [&](bool on) { return on ? dummy : nullptr; };
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
    const EkvCall c = long_call((nulls & 1) ? nullptr : &bank, (nulls & 2) ? nullptr : &st, dtype);
    int32_t info[EKV_LONG_INFO_N];
    for (int32_t& x : info) x = -7;
    const int check = call_check(c);
    const int irc = call_info(c, (nulls & 32) ? nullptr : info, (nulls & 64) ? 0 : EKV_LONG_INFO_N);
    std::printf("%d %d", check, irc);
    for (int32_t x : info) std::printf(" %d", x);
    std::printf(" %zu\n", call_workspace_bytes(c));
  }
  return 0;
}
