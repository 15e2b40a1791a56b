// The step planner over the heads call family (ekv_heads_*), as a stand-alone host program: links easykv_amd/csrc/ekv_plan.cpp and nothing
// else of the library (tests/test_heads_cpu.py builds it with -fsanitize=address,undefined and runs it as a child process).  Only the HOST
// copy of the table is read; the device pointer is a dummy, nothing is dereferenced behind a descriptor's pointers, nothing is launched.
//
// The grid is generated here: head_dim x GQA factor x policy x element type x n_split x (whole step, phases 1 | 4 with defer_layers, phases
// 8 with defer_layers) x (grow, evict) x (a table of equal counts, a ragged table whose longest head sits in the LAST layer, so that the
// envelope of a deferred layer call spans layers), then every refusal and argument error.  One line per call: the heads call and, side by
// side, the call it must plan as — the _typed call of the same step with n_slots = the envelope (the whole-step form: with phases = 1 | 2):
//   head_dim hq h layers cap q_len T_envelope policy n_evict rope n_split dtype tova_head_mean phases defer_layers grow
//   kind(0 equal counts, 1 ragged, 2 NULL struct, 3 NULL rows, 4 NULL rows_host, 5 grow < 0, 6 a count < 1, 7 T > cap, 8 deferred layers outside the bank,
//        9 a head too short for the step's selection window)
//     =>  heads: check, info rc, the ten info fields, workspace bytes | twin: check, the ten info fields, workspace bytes
#include <algorithm>
#include <cstdio>
#include <vector>

#include "../easykv_amd/csrc/ekv_plan.h"

namespace {

void* const kDummy = reinterpret_cast<void*>(256);      // (non-null, never dereferenced)
const int kLayers = 4;

struct Case {
  int32_t d, hq, h, cap, rows;      // rows: the longest head's count in the table
  ekv_step st;
};

Case step_case(int d, int hq, int h, int rows, int policy, int n_evict, int n_split, int cap_slack = 64) {
  Case c{};
  c.d = d, c.hq = hq, c.h = h, c.rows = rows, c.cap = (rows + cap_slack + 3) / 4 * 4;
  ekv_step& st = c.st;
  st.layer_count = kLayers, st.q_len = 1, st.n_slots = 7 /* ignored */, st.accumulate = policy != 0, st.roco_tail = 10, st.causal = 1;
  st.policy = policy, st.n_evict = policy != 0 ? n_evict : 0, st.win_lo = 0, st.win_tail = policy == 1 ? 8 : 0;
  st.roco_k1 = 24, st.range_start = policy == 4 ? 4 : -1;
  st.n_split = n_split, st.count_add = 1.f, st.sm_div = 8.f;
  return c;
}

// form: 0 whole, 5 the layer call (layer 1), 8 the flush
void set_form(Case* c, int form) {
  if (form == 0) return;
  c->st.defer_layers = kLayers, c->st.phases = form;
  if (form == 5) c->st.layer_begin = c->st.defer_index = 1, c->st.layer_count = 1;
}

void emit(const Case& c, int32_t dtype, int kind, int grow = 0) {
  ekv_bank bank{};
  bank.head_dim = c.d, bank.n_q_heads = c.hq, bank.n_kv_heads = c.h, bank.n_layers = kLayers, bank.cap = c.cap;
  bank.arrive = static_cast<uint32_t*>(kDummy), bank.birth = static_cast<int32_t*>(kDummy), bank.slot_state = static_cast<float*>(kDummy);
  bank.score_sum = bank.score_sq = bank.score_cnt = static_cast<float*>(kDummy);
  bank.k = bank.v = kDummy, bank.slot_of_pos = static_cast<int32_t*>(kDummy);
  std::vector<int32_t> table((size_t)kLayers * c.h, c.rows);
  if (kind == 1)      // ragged: as short as 40 rows, the longest head in the last layer only
    for (int l = 0; l < kLayers; ++l)
      for (int h = 0; h < c.h; ++h)
        if (!(l == kLayers - 1 && h == c.h - 1)) table[(size_t)l * c.h + h] = std::max(40, c.rows - 1 - (l * 37 + h * 101) % c.rows);
  if (kind == 6) table[table.size() / 2] = 0;
  if (kind == 9) table[0] = 1;      // T = 2: fewer candidates than victims outside the protected tail
  if (kind == 7) table[1] = c.cap - grow;      // T = cap + 1
  ekv_step st = c.st, twin_st = c.st;
  if (kind == 8) st.layer_begin = 2, st.defer_index = 3;      // deferred layers -1 .. 2
  twin_st.n_slots = c.rows + grow + 1;
  if ((twin_st.phases & ~(EKV_PHASE_SLOT_ROWS | EKV_PHASE_SLOT_TAIL_OK)) == 0) twin_st.phases |= 1 | 2;
  const ekv_heads hd{kind == 3 ? nullptr : static_cast<const int32_t*>(kDummy), kind == 4 ? nullptr : table.data(), kind == 5 ? -1 : grow};
  const EkvCall heads = heads_call(&bank, &st, dtype, kind == 2 ? nullptr : &hd);
  const EkvCall twin = step_call(&bank, &twin_st, dtype);
  int32_t ci[EKV_STEP_INFO_N], pi[EKV_STEP_INFO_N];
  for (int i = 0; i < EKV_STEP_INFO_N; ++i) ci[i] = pi[i] = -7;
  const int cc = call_check(heads), pc = call_check(twin);
  const int irc = call_info(heads, ci, EKV_STEP_INFO_N);
  (void)call_info(twin, pi, EKV_STEP_INFO_N);
  std::printf("%d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d =>", c.d, c.hq, c.h, kLayers, c.cap, st.q_len, twin_st.n_slots, st.policy, st.n_evict,
              st.rope_on_read, st.n_split, dtype, st.tova_head_mean, st.phases, st.defer_layers, grow, kind);
  std::printf(" %d %d", cc, irc);
  for (int32_t x : ci) std::printf(" %d", x);
  std::printf(" %zu | %d", call_workspace_bytes(heads), pc);
  for (int32_t x : pi) std::printf(" %d", x);
  std::printf(" %zu\n", call_workspace_bytes(twin));
}

}  // namespace

int main() {
  const int kHeads[][2] = {{8, 8}, {8, 4}, {8, 2}, {8, 1}, {66, 66}, {12, 4}};      // GQA 1, 2, 4, 8; 66 KV heads; GQA 3
  const int kD[] = {32, 64, 96, 128, 256}, kRows[] = {128, 700, 3000};
  for (int d : kD) for (const auto& hd : kHeads) for (int rows : kRows) for (int policy : {0, 1, 2, 3}) for (int n_evict : {0, 1}) {
    if (policy == 0 && n_evict) continue;
    for (int n_split : {1, 2, 3}) for (int form : {0, 5, 8}) for (int kind : {0, 1}) {
      const int32_t dtype = (n_split + form) & 1 ? EKV_DTYPE_BF16 : EKV_DTYPE_F16;
      Case c = step_case(d, hd[0], hd[1], rows, policy, n_evict, n_split);
      set_form(&c, form);
      emit(c, dtype, kind, kind == 1 ? 3 : 0);
    }
  }
  // the whole step with a split count of the planner's choosing (the deferred forms need an explicit one)
  for (int d : {64, 128}) for (const auto& hd : kHeads) for (int rows : kRows) for (int policy : {1, 3}) for (int kind : {0, 1})
    emit(step_case(d, hd[0], hd[1], rows, policy, 1, 0), EKV_DTYPE_F16, kind);
  // the refusals, each on a step the family takes: q_len 2, RoPE-on-read, slot-indexed rows, the head-mean TOVA row, two victims, a GQA
  // factor of 16, the range compaction, rows past the fast scorer (6144 slots), cap % 4 != 0 under a scored policy
  for (int d : {64, 128}) for (int form : {0, 5, 8}) {
    Case c = step_case(d, 8, 4, 700, 1, 1, 2);
    set_form(&c, form);
    emit(c, EKV_DTYPE_F16, 1);
    Case r = c;
    r.st.q_len = 2;
    emit(r, EKV_DTYPE_F16, 1);
    r = c, r.st.rope_on_read = 1;
    emit(r, EKV_DTYPE_F16, 1);
    r = c, r.st.phases |= EKV_PHASE_SLOT_ROWS;
    emit(r, EKV_DTYPE_F16, 1);
    r = c, r.st.policy = 3, r.st.tova_head_mean = 1;
    emit(r, EKV_DTYPE_F16, 1);
    r = c, r.st.n_evict = 2;
    emit(r, EKV_DTYPE_F16, 1);
    r = c, r.hq = 64;
    emit(r, EKV_DTYPE_F16, 1);
    r = c, r.st.policy = 4, r.st.range_start = 4;
    emit(r, EKV_DTYPE_F16, 1);
    r = step_case(d, 8, 4, 6200, 1, 1, 2);
    set_form(&r, form);
    emit(r, EKV_DTYPE_F16, 1);
    r = c, r.cap += 2;
    emit(r, EKV_DTYPE_F16, 1);
    // the argument errors
    for (int kind : {2, 3, 4, 5, 6, 7}) emit(c, EKV_DTYPE_F16, kind);
    if (form) emit(c, EKV_DTYPE_F16, 8);
    emit(c, 2, 1);      // an element type that does not exist
    emit(c, EKV_DTYPE_F16, 9);      // a one-row head has no candidate to give: the uniform step's own argument error, from the shortest head
  }
  return 0;
}
