// The step planner over a head_dim-256 grid, as a stand-alone host program: links easykv_amd/csrc/ekv_plan.cpp and nothing else of the
// library (tests/test_d256_cpu.py builds it with -fsanitize=address,undefined and runs it as a child process).  Nothing is dereferenced
// behind a descriptor's pointers and nothing is launched.
//
// The grid is generated here: GQA factor x layers x cache length (up to 16 384) x policy x q_len (decode steps and chunk steps in
// every scheme), 16-bit calls in both element types, FP8 calls, and uniform and ragged batch tables.  One line per call:
//   <the case as tests/plan_host_main.cpp reads it: the KEYS of tests/test_dispatch_table.py, dtype kv8 nullmask batch n_seq, 9 integers
//    per table entry>  =>  check, plan rc, n_split, fused, info rc, the ten info fields, workspace bytes
// so that the test can put the same call to the library and compare.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <memory>
#include <vector>

#include "../easykv_amd/csrc/ekv_plan.h"

namespace {

void* const kDummy = reinterpret_cast<void*>(256);      // (non-null, never dereferenced)

struct Case {
  int32_t hq, h, n_layers, cap;
  ekv_step st;
  int32_t count_add2;
};

int align64(int x) { return (x + 63) / 64 * 64; }

// A valid decode step of `policy` at length T (tests/test_batch_cpu.py, _policy_kw)
void policy_fields(ekv_step* st, int policy, int T) {
  const int ev = (T >= 3 && policy != 0) ? 1 : 0;
  st->policy = policy, st->n_evict = ev, st->roco_k1 = std::max(ev, T - T / 3), st->win_lo = 0, st->win_tail = policy == 1 ? T / 4 : 0;
  st->range_start = (policy == 4 && ev) ? T / 2 : -1;
}

Case decode_case(int hq, int h, int layers, int T, int policy, int n_split) {
  Case c{};
  c.hq = hq, c.h = h, c.n_layers = layers, c.cap = align64(T + 64), c.count_add2 = 2;
  c.st.layer_count = layers, c.st.q_len = 1, c.st.n_slots = T, c.st.accumulate = 1, c.st.roco_tail = 10, c.st.causal = 1, c.st.n_split = n_split;
  policy_fields(&c.st, policy, T);
  return c;
}

// A strided chunk step of the prefill: n new rows onto T - n cached ones (tests/test_dispatch_table.py, _chunk)
Case chunk_case(int hq, int h, int layers, int T, int policy, int n, int two_pass, int n_split) {
  Case c{};
  const int t_prev = T - n;
  c.hq = hq, c.h = h, c.n_layers = layers, c.cap = align64(T + 64), c.count_add2 = 2 * n;
  c.st.layer_count = layers, c.st.q_len = n, c.st.n_slots = T, c.st.accumulate = 1, c.st.roco_tail = 10, c.st.causal = 1;
  c.st.policy = policy, c.st.n_evict = (t_prev > n && policy != 0) ? n : 0, c.st.win_lo = t_prev > 100 ? 4 : 0, c.st.win_tail = T / 10;
  c.st.roco_k1 = std::max(T - T / 10 - 4, n), c.st.range_start = (policy == 4 && c.st.n_evict) ? T / 3 : -1;
  c.st.two_pass = two_pass, c.st.n_split = n_split;
  return c;
}

void emit(const Case& c, int32_t dtype, bool kv8, const std::vector<ekv_seq>& seqs, bool batch) {
  ekv_bank bank{};
  bank.head_dim = 256, bank.n_q_heads = c.hq, bank.n_kv_heads = c.h, bank.n_layers = c.n_layers, bank.cap = c.cap;
  bank.arrive = static_cast<uint32_t*>(kDummy), bank.birth = static_cast<int32_t*>(kDummy), bank.slot_state = static_cast<float*>(kDummy);
  bank.score_sum = bank.score_sq = bank.score_cnt = static_cast<float*>(kDummy);
  bank.k = bank.v = kDummy, bank.slot_of_pos = static_cast<int32_t*>(kDummy);
  ekv_step st = c.st;
  st.count_add = (float)(c.count_add2 / 2.0), st.count_tail_step = st.q_len > 1 ? -1.f : 0.f, st.sm_div = 16.f;
  ekv_kv8 q8{kDummy, kDummy, static_cast<float*>(kDummy), static_cast<float*>(kDummy)};
  std::unique_ptr<ekv_seq[]> table(new ekv_seq[seqs.size()]);      // exactly the entries of the call: a read past them is the sanitizer's to report
  std::copy(seqs.begin(), seqs.end(), table.get());
  EkvCall call = step_call(&bank, &st, dtype);
  if (kv8) call = kv8_call(&bank, &st, dtype, &q8);
  if (batch) call = batch_call(&bank, &st, dtype, table.get(), (int32_t)seqs.size());
  if (batch && kv8) call = kv8_batch_call(&bank, &st, dtype, &q8, table.get(), (int32_t)seqs.size());
  int32_t info[EKV_STEP_INFO_N], ns = -7, fu = -7, prc = -7;
  for (int32_t& x : info) x = -7;
  const int check = call_check(call);
  if (!kv8 && !batch && dtype == EKV_DTYPE_F16) prc = call_plan(&bank, &st, &ns, &fu);
  const int irc = call_info(call, info, EKV_STEP_INFO_N);
  // the case, in the column order of KEYS
  std::printf("256 %d %d %d %d 1 1 1 1", c.hq, c.h, c.n_layers, c.cap);
  std::printf(" %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d 0 0 0 0 0 0", st.layer_begin, st.layer_count, st.q_len,
              st.n_slots, st.score_off, st.policy, st.accumulate, st.n_evict, st.win_lo, st.win_tail, st.roco_k1, st.roco_tail, st.range_start,
              st.tova_head_mean, st.causal, st.rope_on_read, st.n_split, st.phases, c.count_add2, st.two_pass, st.phys_extent, st.defer_layers,
              st.defer_index);
  std::printf(" %d %d 0 %d %zu", dtype, kv8 ? 1 : 0, batch ? 1 : 0, batch ? seqs.size() : (size_t)0);
  if (batch)
    for (const ekv_seq& e : seqs)
      std::printf(" %d %d %d %d %d %d %d %d %d", e.layer, e.n_slots, e.score_off, e.n_evict, e.win_lo, e.win_tail, e.roco_k1, e.range_start, e.phys_extent);
  std::printf(" => %d %d %d %d %d", check, prc, ns, fu, irc);
  for (int32_t x : info) std::printf(" %d", x);
  std::printf(" %zu\n", call_workspace_bytes(call));
}

}  // namespace

int main() {
  const int kHeads[][2] = {{8, 8}, {8, 4}, {12, 4}, {16, 4}, {28, 4}, {8, 1}, {24, 2}, {40, 1}};      // GQA factors 1, 2, 3, 4, 7, 8, 12, 40
  const int kLayers[] = {1, 4, 32, 64}, kT[] = {5, 64, 130, 300, 701, 2049, 5002, 16384}, kQ[] = {3, 8, 16, 64, 130};
  const std::vector<ekv_seq> none;
  for (const auto& hd : kHeads) for (int layers : kLayers) for (int T : kT) for (int policy = 0; policy <= 4; ++policy) {
    for (int n_split : {0, 1, 3}) {
      const Case c = decode_case(hd[0], hd[1], layers, T, policy, n_split);
      for (int32_t dtype : {EKV_DTYPE_F16, EKV_DTYPE_BF16}) emit(c, dtype, false, none, false);
      if (n_split == 0) {
        emit(c, EKV_DTYPE_F16, true, none, false);      // every quantised row format refuses the head_dim: the FP8 call stands for them
        Case rope = c;
        rope.st.rope_on_read = 1;
        emit(rope, EKV_DTYPE_F16, false, none, false);
      }
      if (n_split != 0 || layers < 4) continue;
      // batch tables of this step: uniform, and ragged (lengths 2 .. T, every other entry evicts nothing)
      const int n_seq = std::min(layers, 33);
      std::vector<ekv_seq> uniform, ragged;
      for (int i = 0; i < n_seq; ++i) {
        uniform.push_back({i, T,c.st.score_off, c.st.n_evict, c.st.win_lo, c.st.win_tail, c.st.roco_k1, c.st.range_start, 0});
        const int t = i == n_seq / 2 ? T : std::max(i == 0 ? 2 : 1, std::min(T, (int)((int64_t)T * (i + 1) / n_seq) - (i % 3)));
        ekv_step e{};
        policy_fields(&e, policy, t);
        if (i % 2 == 0 && t != T) e.n_evict = 0, e.range_start = -1;
        ragged.push_back({(5 * i + 1) % layers, t, 0, e.n_evict, 0, e.win_tail, std::max(e.n_evict, e.roco_k1), e.range_start, std::min(c.cap, t + i)});
      }
      // (layers of a table must differ: 5 i + 1 mod layers is a permutation for layers in {4, 32, 64})
      for (int32_t dtype : {EKV_DTYPE_F16, EKV_DTYPE_BF16}) {
        emit(c, dtype, false, uniform, true);
        emit(c, dtype, false, ragged, true);
      }
      emit(c, EKV_DTYPE_F16, true, uniform, true);
    }
    for (int n : kQ) {
      if (n >= T) continue;
      for (int two_pass : {0, 1, -1}) for (int n_split : {0, 2}) {
        const Case c = chunk_case(hd[0], hd[1], layers, T, policy, n, two_pass, n_split);
        emit(c, n_split ? EKV_DTYPE_BF16 : EKV_DTYPE_F16, false, none, false);
      }
      Case rope = chunk_case(hd[0], hd[1], layers, T, policy, n, 0, 0);
      rope.st.rope_on_read = 1;
      emit(rope, EKV_DTYPE_F16, false, none, false);
    }
    // the dense prefix: T rows at once, nothing scored
    if (policy == 0 && T >= 64) emit(chunk_case(hd[0], hd[1], layers, T, 0, T, 0, 0), EKV_DTYPE_F16, false, none, false);
  }
  return 0;
}
