// The step planner over the adaptive call family (ekv_ada_*), as a stand-alone host program: links easykv_amd/csrc/ekv_plan.cpp and nothing
// else of the library (tests/test_adaptive_cpu.py builds it with -fsanitize=address,undefined and runs it as a child process).  Nothing is
// dereferenced behind a descriptor's pointers and nothing is launched.
//
// The grid is generated here: head_dim x GQA factor x q_len x cache length x n_split x policy, many victims per step, both pooling ops,
// radius 0 and 3, bounds around n_evict (the driver's floor / ceiling and the degenerate evict_min = evict_max = n_evict), the deferred
// form, and every refusal and argument error.  One line per call: the adaptive call and, side by side, the call it must plan as — the
// pooled call of the same step (radius >= 1) or, for radius 0, the plain call with phases = 1 | 2:
//   head_dim hq h layers cap q_len T policy n_evict win_lo win_tail rope n_split two_pass dtype tova_head_mean phases defer_layers radius op
//   evict_min evict_max null(0 none, 1 struct, 2 n_evict_out)
//     =>  ada: check, info rc, the ten info fields, workspace bytes | twin: check, the ten info fields, workspace bytes
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

Case step_case(int d, int hq, int h, int layers, int T, int policy, int n, int n_evict, int two_pass, int n_split) {
  Case c{};
  c.d = d, c.hq = hq, c.h = h, c.n_layers = layers, c.cap = align64(T + 64);
  ekv_step& st = c.st;
  st.layer_count = layers, st.q_len = n, st.n_slots = T, st.accumulate = policy != 0, st.roco_tail = 10, st.causal = 1;
  st.policy = policy, st.n_evict = policy != 0 ? n_evict : 0, st.win_lo = 4, st.win_tail = n;
  st.roco_k1 = std::max(T - n - 4, n_evict), st.range_start = policy == 4 ? 4 : -1;
  st.two_pass = two_pass, st.n_split = n_split;
  st.count_add = (float)n, st.count_tail_step = -1.f;
  return c;
}

void emit(const Case& c, int32_t dtype, int radius, int op, int evict_min, int evict_max, int null = 0) {
  ekv_bank bank{};
  bank.head_dim = c.d, bank.n_q_heads = c.hq, bank.n_kv_heads = c.h, bank.n_layers = c.n_layers, bank.cap = c.cap;
  bank.arrive = static_cast<uint32_t*>(kDummy), bank.birth = static_cast<int32_t*>(kDummy), bank.slot_state = static_cast<float*>(kDummy);
  bank.score_sum = bank.score_sq = bank.score_cnt = static_cast<float*>(kDummy);
  bank.k = bank.v = kDummy, bank.slot_of_pos = static_cast<int32_t*>(kDummy);
  ekv_step st = c.st, st_plain = c.st;
  st.sm_div = st_plain.sm_div = 8.f;
  if (st_plain.phases == 0) st_plain.phases = 1 | 2;
  const ekv_ada ada{radius, op, evict_min, evict_max, null == 2 ? nullptr : static_cast<int32_t*>(kDummy)};
  const ekv_pool pool{radius, op};
  const EkvCall adaptive = ada_call(&bank, &st, dtype, null == 1 ? nullptr : &ada);
  const EkvCall twin = radius >= 1 ? pool_call(&bank, &st, dtype, &pool) : step_call(&bank, &st_plain, dtype);
  int32_t ci[EKV_STEP_INFO_N], pi[EKV_STEP_INFO_N];
  for (int i = 0; i < EKV_STEP_INFO_N; ++i) ci[i] = pi[i] = -7;
  const int cc = call_check(adaptive), pc = call_check(twin);
  const int irc = call_info(adaptive, ci, EKV_STEP_INFO_N);
  (void)call_info(twin, pi, EKV_STEP_INFO_N);
  std::printf("%d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d =>", c.d, c.hq, c.h, c.n_layers, c.cap, st.q_len, st.n_slots, st.policy,
              st.n_evict, st.win_lo, st.win_tail, st.rope_on_read, st.n_split, st.two_pass, dtype, st.tova_head_mean, st.phases, st.defer_layers, radius,
              op, evict_min, evict_max, null);
  std::printf(" %d %d", cc, irc);
  for (int32_t x : ci) std::printf(" %d", x);
  std::printf(" %zu | %d", call_workspace_bytes(adaptive), pc);
  for (int32_t x : pi) std::printf(" %d", x);
  std::printf(" %zu\n", call_workspace_bytes(twin));
}

}  // namespace

int main() {
  const int kHeads[][2] = {{8, 8}, {8, 4}, {16, 2}, {40, 1}, {64, 64}, {65, 65}, {128, 128}};      // GQA 1, 2, 8, 40; 64 KV heads and beyond
  const int kD[] = {64, 128}, kLayers[] = {1, 32}, kT[] = {300, 1500, 4096, 12000, 38000, 39500}, kQ[] = {1, 8, 32, 64};
  for (int d : kD) for (const auto& hd : kHeads) for (int layers : kLayers) for (int T : kT) for (int n : kQ) {
    if (n + 4 + 64 >= T) continue;
    const int C = T - n - 4;
    for (int policy : {1, 3}) for (int n_evict : {T / 2, T - 64 - n}) {
      if (n_evict > C) continue;
      const int K = C - n_evict, lo = std::max(0, C - 2 * K), hi = C - K / 5;      // the driver's ceiling 2.0 and floor 0.2
      for (int n_split : {0, 2}) for (int radius : {0, 3}) {
        const int32_t dtype = n_split == 2 ? EKV_DTYPE_BF16 : EKV_DTYPE_F16;
        const Case c = step_case(d, hd[0], hd[1], layers, T, policy, n, n_evict, 0, n_split);
        emit(c, dtype, radius, policy == 1 ? EKV_POOL_MAX : EKV_POOL_AVG, lo, hi);
        emit(c, dtype, radius, policy == 1 ? EKV_POOL_MAX : EKV_POOL_AVG, n_evict, n_evict);
        emit(c, dtype, radius, EKV_POOL_AVG, 0, C);
      }
    }
    // the refusals, on a step the adaptive call takes with h2o_head: roco, the range policies, no policy, RoPE-on-read, the head-mean TOVA
    // row, slot-indexed score rows; then the argument errors: a NULL struct, NULL n_evict_out, a negative radius, an unknown op, bounds
    // out of order, an element type that does not exist
    if (layers == 1 && T <= 4096 && hd[1] <= 64) {
      const int k = T / 2;
      for (int policy : {0, 2, 4}) emit(step_case(d, hd[0], hd[1], layers, T, policy, n, k, 0, 0), EKV_DTYPE_F16, 3, EKV_POOL_MAX, k / 2, std::min(C, k + k / 2));
      Case c = step_case(d, hd[0], hd[1], layers, T, 1, n, k, 0, 0);
      c.st.rope_on_read = 1;
      emit(c, EKV_DTYPE_F16, 3, EKV_POOL_MAX, k, k);
      c = step_case(d, hd[0], hd[1], layers, T, 3, n, k, 0, 0);
      c.st.tova_head_mean = 1;
      emit(c, EKV_DTYPE_F16, 3, EKV_POOL_AVG, k, k);
      c = step_case(d, hd[0], hd[1], layers, T, 1, n, n == 1 ? 1 : k, 0, 0);
      c.st.phases = EKV_PHASE_SLOT_ROWS;
      emit(c, EKV_DTYPE_F16, 3, EKV_POOL_MAX, c.st.n_evict, c.st.n_evict);
      c = step_case(d, hd[0], hd[1], layers, T, 1, n, k, 0, 0);
      emit(c, EKV_DTYPE_F16, 3, EKV_POOL_MAX, k, k, 1);
      emit(c, EKV_DTYPE_F16, 3, EKV_POOL_MAX, k, k, 2);
      emit(c, EKV_DTYPE_F16, -1, EKV_POOL_MAX, k, k);
      emit(c, EKV_DTYPE_F16, 3, 2, k, k);
      emit(c, EKV_DTYPE_F16, 3, EKV_POOL_MAX, -1, k);
      emit(c, EKV_DTYPE_F16, 3, EKV_POOL_MAX, k + 1, k + 1);
      emit(c, EKV_DTYPE_F16, 3, EKV_POOL_MAX, k - 1, k - 1);
      emit(c, EKV_DTYPE_F16, 3, EKV_POOL_MAX, k, C + 1);
      emit(c, 2, 3, EKV_POOL_MAX, k, k);
      c.st.n_evict = 0;
      emit(c, EKV_DTYPE_F16, 3, EKV_POOL_MAX, 0, 0);
    }
  }
  // the deferred form of a layer-per-call model: attention + fold of one layer (phases 1 | 4), then the three launches for all layers (phases 8)
  for (int d : {64, 128}) for (const auto& hd : kHeads) for (int n : {8, 32}) for (int T : {300, 1500, 4096}) for (int policy : {1, 3}) {
    for (int ph : {1 | 4, 8}) for (int radius : {0, 3}) {
      Case c = step_case(d, hd[0], hd[1], 4, T, policy, n, T / 2, 0, 2);
      c.st.defer_layers = 4, c.st.phases = ph;
      if (ph == 5) c.st.layer_begin = 1, c.st.layer_count = 1, c.st.defer_index = 1;
      emit(c, EKV_DTYPE_F16, radius, policy == 1 ? EKV_POOL_MAX : EKV_POOL_AVG, T / 4, std::min(T - n - 4, 3 * T / 4));
    }
  }
  return 0;
}
