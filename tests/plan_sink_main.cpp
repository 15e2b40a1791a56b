// The step planner over the sink call family (ekv_sink_*), as a stand-alone host program: links easykv_amd/csrc/ekv_plan.cpp and nothing
// else of the library (tests/test_sink_cpu.py builds it with -fsanitize=address,undefined and runs it as a child process).  Nothing is
// dereferenced behind a descriptor's pointers or behind the sinks, and nothing is launched.
//
// The grid is generated here: head_dim (64, 128 and the refused 96 / 256) x GQA factor x layers x cache length x policy x q_len (decode
// steps, chunk steps of 8 .. 130 rows in every scheme, the dense prefix), both element types, RoPE-on-read, the head-mean TOVA row and
// NULL sinks.  One line per call, the sink call and the plain call of the same step side by side:
//   head_dim hq h layers cap q_len T policy n_evict win_lo win_tail roco_k1 range_start rope n_split two_pass dtype tova_head_mean null
//     =>  sink: check, info rc, the ten info fields, workspace bytes | plain: check, the ten info fields, workspace bytes
// so that the test can put the same calls to the library and compare.
#include <algorithm>
#include <cstdio>

#include "../easykv_amd/csrc/ekv_plan.h"

namespace {

void* const kDummy = reinterpret_cast<void*>(256);      // (non-null, never dereferenced)

struct Case {
  int32_t d, hq, h, n_layers, cap;
  ekv_step st;
};

int align64(int x) { return (x + 63) / 64 * 64; }

Case decode_case(int d, int hq, int h, int layers, int T, int policy, int n_split) {
  Case c{};
  c.d = d, c.hq = hq, c.h = h, c.n_layers = layers, c.cap = align64(T + 64);
  ekv_step& st = c.st;
  st.layer_count = layers, st.q_len = 1, st.n_slots = T, st.accumulate = 1, st.roco_tail = 10, st.causal = 1, st.n_split = n_split;
  const int ev = (T >= 3 && policy != 0) ? 1 : 0;
  st.policy = policy, st.n_evict = ev, st.roco_k1 = std::max(ev, T - T / 3), st.win_tail = policy == 1 ? T / 4 : 0;
  st.range_start = (policy == 4 && ev) ? T / 2 : -1;
  st.count_add = 1.f;
  return c;
}

Case chunk_case(int d, int hq, int h, int layers, int T, int policy, int n, int two_pass, int n_split) {
  Case c{};
  const int t_prev = T - n;
  c.d = d, c.hq = hq, c.h = h, c.n_layers = layers, c.cap = align64(T + 64);
  ekv_step& st = c.st;
  st.layer_count = layers, st.q_len = n, st.n_slots = T, st.accumulate = policy != 0, st.roco_tail = 10, st.causal = 1;
  st.policy = policy, st.n_evict = (t_prev > n && policy != 0) ? n : 0, st.win_lo = t_prev > 100 ? 4 : 0, st.win_tail = T / 10;
  st.roco_k1 = std::max(T - T / 10 - 4, n), st.range_start = (policy == 4 && st.n_evict) ? T / 3 : -1;
  st.two_pass = two_pass, st.n_split = n_split;
  st.count_add = (float)n, st.count_tail_step = -1.f;
  return c;
}

void emit(const Case& c, int32_t dtype, bool null_sinks = false) {
  ekv_bank bank{};
  bank.head_dim = c.d, bank.n_q_heads = c.hq, bank.n_kv_heads = c.h, bank.n_layers = c.n_layers, bank.cap = c.cap;
  bank.arrive = static_cast<uint32_t*>(kDummy), bank.birth = static_cast<int32_t*>(kDummy), bank.slot_state = static_cast<float*>(kDummy);
  bank.score_sum = bank.score_sq = bank.score_cnt = static_cast<float*>(kDummy);
  bank.k = bank.v = kDummy, bank.slot_of_pos = static_cast<int32_t*>(kDummy);
  ekv_step st = c.st;
  st.sm_div = 8.f;
  const EkvCall sink = sink_call(&bank, &st, dtype, null_sinks ? nullptr : static_cast<const float*>(kDummy)), plain = step_call(&bank, &st, dtype);
  int32_t ci[EKV_STEP_INFO_N], pi[EKV_STEP_INFO_N];
  for (int i = 0; i < EKV_STEP_INFO_N; ++i) ci[i] = pi[i] = -7;
  const int cc = call_check(sink), pc = call_check(plain);
  const int irc = call_info(sink, ci, EKV_STEP_INFO_N);
  (void)call_info(plain, pi, EKV_STEP_INFO_N);
  std::printf("%d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d =>", c.d, c.hq, c.h, c.n_layers, c.cap, st.q_len, st.n_slots, st.policy,
              st.n_evict, st.win_lo, st.win_tail, st.roco_k1, st.range_start, st.rope_on_read, st.n_split, st.two_pass, dtype, st.tova_head_mean,
              null_sinks ? 1 : 0);
  std::printf(" %d %d", cc, irc);
  for (int32_t x : ci) std::printf(" %d", x);
  std::printf(" %zu | %d", call_workspace_bytes(sink), pc);
  for (int32_t x : pi) std::printf(" %d", x);
  std::printf(" %zu\n", call_workspace_bytes(plain));
}

}  // namespace

int main() {
  const int kHeads[][2] = {{8, 8}, {8, 4}, {12, 4}, {16, 4}, {16, 2}, {24, 2}, {40, 1}};      // GQA factors 1, 2, 3, 4, 8, 12, 40
  const int kD[] = {64, 128, 96, 256}, kLayers[] = {1, 32}, kT[] = {5, 130, 300, 2049, 5002, 16384}, kQ[] = {8, 33, 64, 128, 130};
  for (int d : kD) for (const auto& hd : kHeads) for (int layers : kLayers) for (int T : kT) for (int policy = 0; policy <= 4; ++policy) {
    for (int n_split : {0, 1, 3}) {
      const Case c = decode_case(d, hd[0], hd[1], layers, T, policy, n_split);
      for (int32_t dtype : {EKV_DTYPE_F16, EKV_DTYPE_BF16}) emit(c, dtype);
      if (n_split == 0) {
        Case rope = c;
        rope.st.rope_on_read = 1;
        emit(rope, EKV_DTYPE_F16);
        emit(c, EKV_DTYPE_F16, true);      // NULL sinks: an argument error
      }
    }
    for (int n : kQ) {
      if (n >= T) continue;
      for (int two_pass : {0, 1, -1}) for (int n_split : {0, 2}) emit(chunk_case(d, hd[0], hd[1], layers, T, policy, n, two_pass, n_split), n_split ? EKV_DTYPE_BF16 : EKV_DTYPE_F16);
      Case rope = chunk_case(d, hd[0], hd[1], layers, T, policy, n, 0, 0);
      rope.st.rope_on_read = 1;
      emit(rope, EKV_DTYPE_F16);
      if (policy == 3 && n == 8) {      // the head-mean TOVA row (encoding / ppl mode): served, by the sink build of its kernel
        Case mean = chunk_case(d, hd[0], hd[1], layers, T, policy, n, 0, 0);
        mean.st.tova_head_mean = 1;
        emit(mean, EKV_DTYPE_F16);
      }
    }
    if (policy == 0 && T >= 64) emit(chunk_case(d, hd[0], hd[1], layers, T, 0, T, 0, 0), EKV_DTYPE_F16);      // the dense prefix
  }
  return 0;
}
