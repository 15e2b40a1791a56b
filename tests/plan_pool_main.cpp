// The step planner over the pooled call family (ekv_pool_*), as a stand-alone host program: links easykv_amd/csrc/ekv_plan.cpp and nothing
// else of the library (tests/test_oneshot_cpu.py builds it with -fsanitize=address,undefined and runs it as a child process).  Nothing is
// dereferenced behind a descriptor's pointers and nothing is launched.
//
// The grid is generated here: head_dim x GQA factor x q_len (a decode step, observation windows of 8 .. 130 rows) x cache length x
// n_split x policy, many victims per step (T / 2 and T - 64, as a one-shot prompt compression asks for), both pooling ops, and every
// refusal.  One line per call, the pooled call (phases = 0) and the plain call of the same step with phases = 1 | 2 side by side — the
// plain call's own way of saying "attention, then the generic scorer, no in-kernel tail":
//   head_dim hq h layers cap q_len T policy n_evict win_lo win_tail roco_k1 rope n_split two_pass dtype tova_head_mean phases radius op null
//     =>  pool: check, info rc, the ten info fields, workspace bytes | plain: check, the ten info fields, workspace bytes
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

void emit(const Case& c, int32_t dtype, int radius, int op, bool null_pool = false) {
  ekv_bank bank{};
  bank.head_dim = c.d, bank.n_q_heads = c.hq, bank.n_kv_heads = c.h, bank.n_layers = c.n_layers, bank.cap = c.cap;
  bank.arrive = static_cast<uint32_t*>(kDummy), bank.birth = static_cast<int32_t*>(kDummy), bank.slot_state = static_cast<float*>(kDummy);
  bank.score_sum = bank.score_sq = bank.score_cnt = static_cast<float*>(kDummy);
  bank.k = bank.v = kDummy, bank.slot_of_pos = static_cast<int32_t*>(kDummy);
  ekv_step st = c.st, st_plain = c.st;
  st.sm_div = st_plain.sm_div = 8.f;
  if (st_plain.phases == 0) st_plain.phases = 1 | 2;
  const ekv_pool pool{radius, op};
  const EkvCall pooled = pool_call(&bank, &st, dtype, null_pool ? nullptr : &pool), plain = step_call(&bank, &st_plain, dtype);
  int32_t ci[EKV_STEP_INFO_N], pi[EKV_STEP_INFO_N];
  for (int i = 0; i < EKV_STEP_INFO_N; ++i) ci[i] = pi[i] = -7;
  const int cc = call_check(pooled), pc = call_check(plain);
  const int irc = call_info(pooled, ci, EKV_STEP_INFO_N);
  (void)call_info(plain, pi, EKV_STEP_INFO_N);
  std::printf("%d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d =>", c.d, c.hq, c.h, c.n_layers, c.cap, st.q_len, st.n_slots, st.policy,
              st.n_evict, st.win_lo, st.win_tail, st.roco_k1, st.rope_on_read, st.n_split, st.two_pass, dtype, st.tova_head_mean, st.phases, radius,
              op, null_pool ? 1 : 0);
  std::printf(" %d %d", cc, irc);
  for (int32_t x : ci) std::printf(" %d", x);
  std::printf(" %zu | %d", call_workspace_bytes(pooled), pc);
  for (int32_t x : pi) std::printf(" %d", x);
  std::printf(" %zu\n", call_workspace_bytes(plain));
}

}  // namespace

int main() {
  const int kHeads[][2] = {{8, 8}, {8, 4}, {12, 4}, {16, 4}, {16, 2}, {40, 1}};      // GQA factors 1, 2, 3, 4, 8, 40
  const int kD[] = {32, 64, 96, 128, 256}, kLayers[] = {1, 32}, kT[] = {200, 300, 1500, 2049, 4096, 12000, 38000, 39500}, kQ[] = {1, 8, 32, 33, 64, 130};
  for (int d : kD) for (const auto& hd : kHeads) for (int layers : kLayers) for (int T : kT) for (int n : kQ) {
    if (n + 4 + 64 >= T) continue;
    for (int policy : {1, 3}) for (int n_evict : {T / 2, T - 64 - n}) {
      if (n_evict > T - n - 4) continue;
      for (int n_split : {0, 1, 2}) for (int two_pass : {0, 1, -1}) {
        if (two_pass != 0 && (n == 1 || layers == 32)) continue;
        emit(step_case(d, hd[0], hd[1], layers, T, policy, n, n_evict, two_pass, n_split), n_split == 2 ? EKV_DTYPE_BF16 : EKV_DTYPE_F16, n_split == 1 ? 1 : 3,
             policy == 1 ? EKV_POOL_MAX : EKV_POOL_AVG);
      }
    }
    // the refusals, on a step the pooled call takes with h2o_head: roco, the range policies, no policy, RoPE-on-read, the head-mean TOVA
    // row, slot-indexed score rows; a NULL struct, radius 0, an unknown op
    if (layers == 1 && T <= 4096) {
      const int k = T / 2;
      for (int policy : {0, 2, 4}) emit(step_case(d, hd[0], hd[1], layers, T, policy, n, k, 0, 0), EKV_DTYPE_F16, 3, EKV_POOL_MAX);
      Case c = step_case(d, hd[0], hd[1], layers, T, 1, n, k, 0, 0);
      c.st.rope_on_read = 1;
      emit(c, EKV_DTYPE_F16, 3, EKV_POOL_MAX);
      c = step_case(d, hd[0], hd[1], layers, T, 3, n, k, 0, 0);
      c.st.tova_head_mean = 1;
      emit(c, EKV_DTYPE_F16, 3, EKV_POOL_AVG);
      c = step_case(d, hd[0], hd[1], layers, T, 1, n, n == 1 ? 1 : k, 0, 0);
      c.st.phases = EKV_PHASE_SLOT_ROWS;
      emit(c, EKV_DTYPE_F16, 3, EKV_POOL_MAX);
      c = step_case(d, hd[0], hd[1], layers, T, 1, n, k, 0, 0);
      emit(c, EKV_DTYPE_F16, 3, EKV_POOL_MAX, true);
      emit(c, EKV_DTYPE_F16, 0, EKV_POOL_MAX);
      emit(c, EKV_DTYPE_F16, 3, 2);
      emit(c, 2, 3, EKV_POOL_MAX);      // (an element type that does not exist)
    }
  }
  // the deferred form of a layer-per-call model: attention + fold of one layer (phases 1 | 4), then the scorer of all layers (phases 8)
  for (int d : {64, 128}) for (const auto& hd : kHeads) for (int n : {8, 32, 64}) for (int T : {300, 1500, 4096}) for (int policy : {1, 3}) {
    for (int ph : {1 | 4, 8}) {
      Case c = step_case(d, hd[0], hd[1], 4, T, policy, n, T / 2, 0, 2);
      c.st.defer_layers = 4, c.st.phases = ph;
      if (ph == 5) c.st.layer_begin = 1, c.st.layer_count = 1, c.st.defer_index = 1;
      emit(c, EKV_DTYPE_F16, 3, policy == 1 ? EKV_POOL_MAX : EKV_POOL_AVG);
    }
  }
  return 0;
}
