// The step planner as a stand-alone host program: links easykv_amd/csrc/ekv_plan.cpp and nothing else of the library, so that the
// code that takes raw caller descriptors can run under a sanitizer (tests/test_plan_host_cpu.py builds it with
// -fsanitize=address,undefined).  Nothing is dereferenced behind a descriptor's pointers and nothing is launched.
//
//   plan_host_main             cases from stdin, one per line of integers:
//                                the KEYS of tests/test_dispatch_table.py, then optionally
//                                dtype kv8 nullmask batch n_seq  and, for a batch, 9 integers per table entry (ekv_seq)
//                              nullmask bits: 1 bank, 2 step, 4 bank.k, 8 bank.v, 16 bank.slot_of_pos, 32 kv8 descriptor, 64 one kv8 plane,
//                              128 the table.  Output per case: check, plan rc, n_split, fused, info rc, the ten info fields, workspace bytes
//                              (plan rc / n_split / fused are -7 for kv8 and batch calls, which have no ekv_step_plan).
//   plan_host_main --predicates   the geometry predicates over a fixed sweep that crosses every threshold, one "name count values..."
//                              line per function (tests/golden/dispatch/predicates.npz)
#include <cmath>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "../easykv_amd/csrc/ekv_plan.h"

namespace {

// ---- the byte counts under the names the predicate table was recorded with
size_t score_lds_nt(int nt, const EkvScoreArgs& a) { return ekv_score_lds_bytes(nt, a); }
size_t chunk_lds_bytes_d(int d, int rows, int e, int t) {
  return d == 32 ? ekv_chunk_lds_bytes<32>(rows, e, t) : d == 64 ? ekv_chunk_lds_bytes<64>(rows, e, t) : ekv_chunk_lds_bytes<128>(rows, e, t);
}

void* const kDummy = reinterpret_cast<void*>(256);      // (what the Python tests pass: non-null, never dereferenced)

int run_cases() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::vector<long long> v;
    for (long long x; in >> x;) v.push_back(x);
    if (v.empty()) continue;
    if (v.size() < 38) return 2;
    auto at = [&](size_t i) { return i < v.size() ? (int32_t)v[i] : 0; };
    const int32_t dtype = at(38), kv8 = at(39), nulls = at(40), batch = at(41), n_seq = at(42);
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
    ekv_kv8 q8{kDummy, kDummy, static_cast<float*>(ptr(!(nulls & 64))), static_cast<float*>(kDummy)};
    const size_t n_entries = v.size() > 43 ? (v.size() - 43) / 9 : 0;
    std::unique_ptr<ekv_seq[]> seqs(new ekv_seq[n_entries]);      // exactly the entries on the line: a read past them is the sanitizer's to report
    for (size_t e = 0, i = 43; e < n_entries; ++e, i += 9) seqs[e] = {at(i), at(i + 1), at(i + 2), at(i + 3), at(i + 4), at(i + 5), at(i + 6), at(i + 7), at(i + 8)};
    const ekv_bank* b = (nulls & 1) ? nullptr : &bank;
    const ekv_step* s = (nulls & 2) ? nullptr : &st;
    EkvCall c = step_call(b, s, dtype);
    if (kv8) c = kv8_call(b, s, dtype, (nulls & 32) ? nullptr : &q8);
    if (batch) c = batch_call(b, s, dtype, (nulls & 128) ? nullptr : seqs.get(), n_seq);
    int32_t info[EKV_STEP_INFO_N], ns = -7, fu = -7, prc = -7;
    for (int32_t& x : info) x = -7;
    const int check = call_check(c);
    if (!kv8 && !batch && dtype == EKV_DTYPE_F16) prc = call_plan(b, s, &ns, &fu);
    const int irc = call_info(c, info, EKV_STEP_INFO_N);
    std::printf("%d %d %d %d %d", check, prc, ns, fu, irc);
    for (int32_t x : info) std::printf(" %d", x);
    std::printf(" %zu\n", call_workspace_bytes(c));
  }
  return 0;
}

// ---- the predicate sweep: head_dim 32 / 64 / 96 / 128, GQA factors 1 .. 16, lengths in steps of 64 up to 16384 and 38 000 .. 40 000
struct Out {
  std::vector<long long> v;
  void emit(const char* name) {
    std::printf("%s %zu", name, v.size());
    for (long long x : v) std::printf(" %lld", x);
    std::printf("\n");
    v.clear();
  }
};

int run_predicates() {
  const int kD[] = {32, 64, 96, 128}, kPol[] = {EKV_POLICY_H2O_HEAD, EKV_POLICY_ROCO, EKV_POLICY_TOVA};
  const int kQ[] = {2, 8, 9, 16, 32, 33, 39, 40, 64, 65, 96, 128};
  std::vector<int> ts;
  for (int t = 64; t <= 16384; t += 64) ts.push_back(t);
  for (int t = 38000; t <= 40000; t += 64) ts.push_back(t);
  Out o;
  for (int d : kD) for (int rep = 1; rep <= 16; ++rep) for (int t : ts) for (int nw : {4, 8}) for (int e : {0, 64})
    o.v.push_back(ekv_decode_fused_supported(d, rep, t, t, t + e, 1, t + e, nw));
  for (int t : {2048, 6144}) for (int ev : {0, 2}) for (int cap : {t, t + 2, 8})
    o.v.push_back(ekv_decode_fused_supported(128, 1, t, t, t, ev, cap, 4));
  o.emit("ekv_decode_fused_supported");
  for (int rep = 1; rep <= 16; ++rep) for (int t : ts) for (int pol : kPol) for (int q : {1, 2}) {
    EkvScoreArgs sc{};
    sc.n_q_heads = rep, sc.n_kv_heads = 1, sc.q_len = q, sc.n_evict = 1, sc.cap = t, sc.n_slots = t - 1, sc.t_pad = t, sc.policy = pol;
    o.v.push_back(ekv_decode_score_supported(sc));
  }
  o.emit("ekv_decode_score_supported");
  for (int d : kD) for (int rep = 1; rep <= 16; ++rep) for (int q : kQ) for (int t : ts) for (int off : {0, 4})
    o.v.push_back(ekv_attn_resident_supported(d, rep, q, t, t - off));
  o.emit("ekv_attn_resident_supported");
  for (int t : ts) for (int w : {t - 64, t - 1, t, t + 1}) for (int n_wg : {1, 2}) o.v.push_back(ekv_wide_tail_supported(w, n_wg));
  o.emit("ekv_wide_tail_supported");
  for (int d : kD) for (int rep = 1; rep <= 16; ++rep) for (int q : {2, 4, 8}) for (int t : ts) for (int e : {0, 64}) for (int pol : kPol) {
    ekv_bank b{};
    ekv_step st{};
    b.head_dim = d, b.n_q_heads = rep, b.n_kv_heads = 1, b.cap = t + e;
    st.q_len = q, st.n_slots = t, st.policy = pol, st.accumulate = 1, st.causal = 1, st.n_evict = q;
    o.v.push_back(ekv_chunk_lds_supported(&b, &st, t + e, true));
  }
  o.emit("ekv_chunk_lds_supported");
  for (int d : kD) for (int rep = 1; rep <= 16; ++rep) for (int q : kQ) for (int pol : kPol) for (int rope : {0, 1}) for (int mode : {-1, 0, 1})
    o.v.push_back(ekv_chunk_two_pass(d, rep, q, pol, true, true, rope != 0, mode));
  o.emit("ekv_chunk_two_pass");
  for (int d : kD) for (int rep = 1; rep <= 16; ++rep) for (int q : kQ) for (int rope : {0, 1}) for (int tp : {0, 1}) for (int lg : {0, 1})
    o.v.push_back(ekv_chunk_wide(d, rep, q, rope != 0, tp != 0, lg != 0));
  o.emit("ekv_chunk_wide");
  for (int rep = 1; rep <= 16; ++rep) for (int q = 1; q <= 520; ++q) {
    int rows, blocks, qpw;
    ekv_chunk_blocks(rep, q, &rows, &blocks, &qpw);
    o.v.insert(o.v.end(), {rows, blocks, qpw});
  }
  o.emit("ekv_chunk_blocks");
  for (int nt : {256, 512, 1024}) {
    for (int rep : {1, 2, 3, 4, 8, 16}) for (int q : {1, 8, 64}) for (int t : ts) for (int var = 0; var < 3; ++var) for (int cs : {0, 1}) for (int big : {0, 1}) {
      static float present;
      EkvScoreArgs sc{};
      sc.n_q_heads = rep, sc.n_kv_heads = 1, sc.q_len = q, sc.n_slots = t, sc.score_off = var ? 4 : 0, sc.policy = var == 2 ? EKV_POLICY_NONE : EKV_POLICY_ROCO;
      sc.colsum = cs ? &present : nullptr, sc.big_rows = big ? &present : nullptr;
      o.v.push_back((long long)score_lds_nt(nt, sc));
    }
    o.emit(nt == 256 ? "ekv_score_lds_bytes_nt256" : nt == 512 ? "ekv_score_lds_bytes_nt512" : "ekv_score_lds_bytes_nt1024");
  }
  for (int t : ts) for (int w : {t - 1, t}) for (int rows : {0, 1, 2, 3, 4, 8, 16, 64, 128, 1024}) o.v.push_back(ekv_score_rows_exceed_lds(w, rows));
  o.emit("ekv_score_rows_exceed_lds");
  for (int d : {32, 64, 128}) {
    for (int rows = 1; rows <= 8; ++rows) for (int t : ts) for (int e : {0, 16, 64}) o.v.push_back((long long)chunk_lds_bytes_d(d, rows, t + e, t));
    o.emit(d == 32 ? "ekv_chunk_lds_bytes_d32" : d == 64 ? "ekv_chunk_lds_bytes_d64" : "ekv_chunk_lds_bytes_d128");
  }
  return 0;
}

}  // namespace

int main(int argc, char** argv) { return argc > 1 && !std::strcmp(argv[1], "--predicates") ? run_predicates() : run_cases(); }
