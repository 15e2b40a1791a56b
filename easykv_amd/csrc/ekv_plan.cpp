// The step planner: every decision about a call of the step family — what the kernel families take, the tiling, the workspace layout,
// the argument checks and the launch sequence — from the caller's descriptors alone.  Host-only: no kernel, no launch, no HIP call,
// nothing behind a descriptor's pointers is read.  The byte counts and bounds come from ekv_geometry.h, the header the kernels and their
// launchers run on.  The environment switches that change a PLAN are read here, once per process; launch-time knobs stay with their
// launchers.
#include "ekv_plan.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>

namespace {

typedef int64_t i64;      // (descriptors arrive unchecked: sums and products of their fields are taken in 64 bits)

bool env_is_1(const char* name) { const char* e = std::getenv(name); return e != nullptr && e[0] == '1'; }
int env_int(const char* name, int otherwise) { const char* e = std::getenv(name); return e != nullptr ? std::atoi(e) : otherwise; }

bool pow2_to_16(int rep) { return rep == 1 || rep == 2 || rep == 4 || rep == 8 || rep == 16; }

}  // namespace

int check_bank(const ekv_bank* b) {
  if (!b || !b->k || !b->v || !b->slot_of_pos) return EKV_E_ARG;
  if (b->n_layers <= 0 || b->n_kv_heads <= 0 || b->n_q_heads % b->n_kv_heads || b->cap <= 0) return EKV_E_ARG;
  if (b->head_dim != 32 && b->head_dim != 64 && b->head_dim != 96 && b->head_dim != 128 && b->head_dim != 256) return EKV_E_UNSUPPORTED;
  return EKV_OK;
}

int check_layers(const ekv_bank* b, int begin, int count) {
  return (begin < 0 || count <= 0 || (i64)begin + count > b->n_layers) ? EKV_E_ARG : EKV_OK;
}

// ---- decode steps ------------------------------------------------------------------------------------------------------------------
// any GQA factor (repeat_kv, llama_patch.py:19-29): factors <= 8 on the build of the next power of two, wider ones in groups of 8
bool ekv_attn_decode_supported(int head_dim, int rep) {
  return (head_dim == 32 || head_dim == 64 || head_dim == 96 || head_dim == 128 || head_dim == 256) && rep >= 1;
}

// The whole decode step in one launch: possible when a head is not split, at most one victim, and the row fits.
// nw = 4: up to four workgroups per CU (LDS <= 80 KB keeps >= 2); nw = 8: one or two workgroups per CU.
// Two rounds (rounds_shape: the step runs the 8-wave instance that has both phase orders — head_dim 128, one query head per KV head,
// 16-bit rows, plain keys, slot-indexed rows, a scored policy, an extent of at most 2304 rows, the 5-column build): a launch of 1024 heads or more runs
// as 8-wave workgroups, two resident per CU, the rest dispatched as the first ones end, every workgroup in order K (the rule by
// dispatch round with threshold 0, ekv_decode_fused_order).  EKV_FUSED_ROUNDS = 0 / 1 (A/B knob, read once) over the compile-time
// default, which is what the headline comparison of DESIGN.md §8 "two rounds" decided: 170.4 -> 165.4 us at 1024 heads (roco; h2o_head
// and tova measured there too), 287.0 -> 282.0 us at the 1600 heads of the 13B shape.
#ifndef EKV_FUSED_ROUNDS_DEFAULT
#define EKV_FUSED_ROUNDS_DEFAULT 1
#endif
// First workgroup, in dispatch order, that runs order K on such a launch.  Measured on the flagship launch (1024 heads, us per launch,
// DESIGN.md §8 "two rounds"): 0 -> 164.2 .. 164.8, 64 -> 164.8 .. 165.2, 128 -> 165.7 .. 166.4, 256 -> 168.2 .. 168.5, 512 (the second
// round alone) 168.3 .. 170.1, 768 -> 168.2 .. 169.3; order K in the FIRST round alone 170.6 .. 171.2; all F 171.6 .. 173.4; the 4-wave
// launch with its slot rule 168.4 .. 169.4.  With two 8-wave workgroups per CU the K stream of one falls under the V stream or the tail
// of the other from the first round on, so every workgroup takes order K: threshold 0.
#ifndef EKV_FUSED_ROUNDS_THRESHOLD
#define EKV_FUSED_ROUNDS_THRESHOLD 0
#endif
// Fewest heads of a launch the planner runs this way by itself: two full rounds on 256 CUs.  At 576 heads (18 layers: one round and an
// eighth) the 8-wave launch is level with the 4-wave one, 110.1 against 110.2 us, so those launches keep four waves.
#ifndef EKV_FUSED_ROUNDS_MIN_HEADS
#define EKV_FUSED_ROUNDS_MIN_HEADS 1024
#endif
namespace {
int fused_nw_forced() {
  static const int force = env_int("EKV_FUSED_NW", 0);   // (A/B knob)
  return force == 4 || force == 8 ? force : 0;
}
}  // namespace
int ekv_decode_fused_nw(i64 n_heads_in_launch, bool rounds_shape) {
  static const int rounds = env_int("EKV_FUSED_ROUNDS", EKV_FUSED_ROUNDS_DEFAULT);
  if (fused_nw_forced()) return fused_nw_forced();
  if (n_heads_in_launch >= 256 && n_heads_in_launch <= 512) return 8;
  return (rounds > 0 && rounds_shape && n_heads_in_launch >= EKV_FUSED_ROUNDS_MIN_HEADS) ? 8 : 4;
}

// Mixed phase orders of the fused decode step: the default mode and rule (ekv_decode_fused_order).  Rule: order K for the workgroups
// whose hardware slot on the CU (HW_ID.TG_ID) has bit 1 set — slots 2 and 3 of the four a CU holds.  The four workgroups of a CU do
// not advance together: the oldest slot is served first and ends its stream ~85 us before the youngest (cycle stamps,
// docs/TUNING.md §8 "phase orders"), so the tails of slots 0 and 1 already run under their neighbours' streams; what is exposed is
// the tail of the LAST workgroup.  With slots 2 and 3 in order K the last thing a CU does is stream V.  Measured (us per launch,
// Llama2-7B shape): all F 185.6, slots {2, 3} 175.1, {1, 2, 3} 176.4, {3} 178.0, {1, 3} 180.3, all K 181.4, {0, 2} 189.7, {0, 1} 191.4.
#ifndef EKV_FUSED_ORDER_DEFAULT
#define EKV_FUSED_ORDER_DEFAULT 1
#endif
#define EKV_FUSED_ORDER_SRC 0
#define EKV_FUSED_ORDER_MASK 2
#define EKV_FUSED_ORDER_BOUND 2
#define EKV_FUSED_ORDER_INVERT 1

// Which phase order the workgroups of a one-launch decode step run in (ekv_plan.h).  Order K exists in the instances that serve the
// flagship shape: head_dim 128, one query head per KV head, slot-indexed rows, 4-wave workgroups of at most 2304 physical rows (the
// rule by hardware slot, below) or 8-wave workgroups of at most 6144 (the rule by dispatch round, in the function), and only
// a scored policy has a tail to move.  Mixed needs at least two workgroups on a CU (256 CUs): per-layer and short stage launches keep
// order F.  EKV_FUSED_ORDER = 0 all F / 1 mixed / 2 all K and EKV_FUSED_ORDER_RULE = source, mask, bound, invert as "s,m,b,i" (A/B knobs, read once).
int ekv_decode_fused_order(int head_dim, int rep, bool scored, bool slot_rows, int nw, i64 n_heads_in_launch, int phys_extent) {
  static const int knob = env_int("EKV_FUSED_ORDER", EKV_FUSED_ORDER_DEFAULT);
  static const bool rule_given = std::getenv("EKV_FUSED_ORDER_RULE") != nullptr;
  auto pack = [](int s, int m, int b, int inv) { return ((s & 3) << 4) | ((inv & 1) << 6) | ((m & 15) << 8) | ((b & 15) << 12); };
  static const int rule = [&] {
    int s = EKV_FUSED_ORDER_SRC, m = EKV_FUSED_ORDER_MASK, b = EKV_FUSED_ORDER_BOUND, inv = EKV_FUSED_ORDER_INVERT;
    if (const char* e = std::getenv("EKV_FUSED_ORDER_RULE")) std::sscanf(e, "%d,%d,%d,%d", &s, &m, &b, &inv);
    return pack(s, m, b, inv);
  }();
  if (knob <= 0 || knob > 2 || head_dim != 128 || rep != 1 || !scored || !slot_rows) return 0;
  if (nw == 8) {
    // The 8-wave instances (extents up to 6144 rows).  Launches of 256 .. 512 heads are one round of one or two workgroups per CU and
    // keep order F in every mode.  More heads run in rounds: on such a launch the hardware slot says nothing about who ends last, the
    // position in the dispatch order does — rule source 3 (ekv_kernels.h, EKV_ORDER_ROUND_*) with the invert bit set: order K from
    // workgroup EKV_FUSED_ROUNDS_THRESHOLD on.  That threshold is 0, so every workgroup of the launch decides by the rule and takes order K
    // (512, the first workgroup that has to wait for a slot on 256 CUs, measured slower: see the macro).  Fewer than 256 heads on 8 waves only exist under EKV_FUSED_NW = 8: all K
    // on request, mixed under an explicit EKV_FUSED_ORDER_RULE (tests and A/B runs).
    if (phys_extent > 6144 || (n_heads_in_launch >= 256 && n_heads_in_launch <= 512)) return 0;
    if (knob == 2) return 2;
    if (rule_given) return 1 | rule;
    return n_heads_in_launch > 512 ? (1 | (3 << 4) | (1 << 6) | EKV_ORDER_ROUND_BITS(EKV_FUSED_ROUNDS_THRESHOLD)) : 0;
  }
  if (nw != 4 || phys_extent > 2304) return 0;
  if (knob == 2) return 2;
  // (rule source 3 is compiled into the 8-wave instances alone: a 4-wave launch ignores an EKV_FUSED_ORDER_RULE that names it and keeps
  //  its slot rule, instead of reading the nibbles as the mask and bound of another source)
  const int rule4 = ((rule >> 4) & 3) == 3 ? pack(EKV_FUSED_ORDER_SRC, EKV_FUSED_ORDER_MASK, EKV_FUSED_ORDER_BOUND, EKV_FUSED_ORDER_INVERT) : rule;
  return n_heads_in_launch >= 512 ? (1 | rule4) : 0;
}

// Resident rows of the one-launch decode step (ekv_plan.h).  Step i + 1 reads the rows of step i except one per head, and the chip has a
// 256 MiB Infinity Cache: a fixed share of the bank read with default-policy loads can be served from it, while the rest is streamed
// non-temporally as before.  The default budget is what the sweep of tools/experiments/exp_resident.py measured best
// (profiles/resident_sweep.json); 0 = every K/V load non-temporal, the code before the resident rows.
#ifndef EKV_RESIDENT_MB_DEFAULT
#define EKV_RESIDENT_MB_DEFAULT 224
#endif
namespace {
i64 g_resident_bytes = -1;      // ekv_set_resident_bytes; < 0: the environment / compile-time default
}
i64 ekv_resident_budget_bytes() {
  static const i64 dflt = (i64)std::max(0, std::min(env_int("EKV_RESIDENT_MB", EKV_RESIDENT_MB_DEFAULT), 1 << 20)) << 20;
  return g_resident_bytes < 0 ? dflt : g_resident_bytes;
}
void ekv_resident_set_budget_bytes(i64 bytes) { g_resident_bytes = bytes; }

int ekv_decode_resident_rows(i64 n_heads_in_launch, i64 row_bytes, int phys_extent, int cap, int score_rows, i64 budget_bytes) {
  static const int force = env_int("EKV_RESIDENT_ROWS", -1);   // (A/B and test knob)
  if (n_heads_in_launch <= 0 || row_bytes <= 0 || phys_extent <= 0 || cap <= 0 || score_rows < 0) return 0;
  const i64 unit = EKV_RESIDENT_UNIT;
  const i64 ext = std::min<i64>(((i64)phys_extent + unit - 1) / unit * unit, 255 * unit);      // (what the kernel field holds)
  if (budget_bytes <= 0) return 0;      // (a caller that switched the resident rows off keeps them off, whatever the knob says)
  if (force >= 0) return (int)std::min<i64>(force / unit * unit, ext);
  const i64 heads = std::min<i64>(n_heads_in_launch, 1 << 20);
  const i64 score = heads * 4 * cap * (score_rows + 2);      // score rows + slot map + birth, `cap` words each
  const i64 per_unit = heads * 2 * unit * std::min<i64>(row_bytes, 1 << 16);      // K + V of 32 rows of every head
  if (budget_bytes < score) return 0;
  return (int)(std::min<i64>((budget_bytes - score) / per_unit, ext / unit) * unit);
}

bool ekv_decode_fused_supported(int head_dim, int rep, int n_slots, int t_pad, int l_pad, int n_evict, int cap, int nw) {
  // (the slot map and the score rows are fetched 16 bytes at a time: rows must be 16-byte aligned)
  if (!ekv_attn_decode_supported(head_dim, rep) || rep > 8 || n_evict > 1 || n_slots > 256 * 24 || (cap & 3) != 0 || cap < 16) return false;
  size_t lds = 1 << 30;
  switch (head_dim) {
    case 32: lds = ekv_fused_lds_max<32>(rep, t_pad, l_pad, nw); break;
    case 64: lds = ekv_fused_lds_max<64>(rep, t_pad, l_pad, nw); break;
    case 96: lds = ekv_fused_lds_max<96>(rep, t_pad, l_pad, nw); break;
    case 128: lds = ekv_fused_lds_max<128>(rep, t_pad, l_pad, nw); break;
    case 256: lds = ekv_fused_lds_max<256>(rep, t_pad, l_pad, nw); break;
  }
  return lds <= (size_t)(nw == 8 ? 150 : 80) * 1024;   // 80 KB still leaves two 4-wave workgroups per CU
}

// the split path's fast scorer (ekv_decode_score.inc: the tail of the fused kernel as a launch of its own)
bool ekv_decode_score_supported(const EkvScoreArgs& sc) {
  const int rep = sc.n_q_heads / sc.n_kv_heads;
  if (sc.q_len != 1 || sc.n_evict > 1 || (sc.cap & 3) != 0 || sc.n_slots > 256 * 24) return false;
  if (rep < 1 || rep > 8) return false;      // (wider GQA factors: the generic scorer)
  return ekv_decode_score_lds(rep <= 2 ? rep : (rep <= 4 ? 4 : 8), sc.t_pad, sc.policy) <= 150 * 1024;
}

// Which one-launch decode steps run on the slot-indexed layout: plain keys, a scored policy over the whole cache (score_off = 0), no
// protected sink window (win_lo = 0: the recent tail is a birth threshold, a sink window would need ranks), at most one victim,
// GQA factor <= 4 and an extent of at most 9 (4-wave workgroups) / 5 (8-wave) rows per thread — the builds whose thread-owned
// columns stay in registers without spills.
static bool ekv_slot_rows_supported(const ekv_bank* bank, const ekv_step* st, int phys_extent, int t_pad) {
  const bool scored = st->policy == EKV_POLICY_H2O_HEAD || st->policy == EKV_POLICY_ROCO || st->policy == EKV_POLICY_TOVA;
  const int rep = bank->n_q_heads / bank->n_kv_heads;
  if (!bank->birth || !bank->slot_state || !scored || st->q_len != 1 || st->rope_on_read || st->n_evict > 1) return false;
  if (!bank->score_sq || !bank->score_cnt) return false;      // (the tail keeps the count base of EVERY policy's appended row in score_cnt)
  if (st->score_off != 0 || st->win_lo != 0 || st->tova_head_mean || rep > 4 || !st->accumulate) return false;
  if (st->count_add != (float)(int)st->count_add) return false;      // counts stay exact integers (count = base + running sum)
  const int max_rows = 6144;      // (columns per thread in registers: 5 / 9 up to 2560 / 2304 rows, 12 / 24 beyond — 8-wave / 4-wave build)
  if (phys_extent > max_rows || bank->cap > 9600) return false;      // (cap: ekv_rows_to_order stages four rows of `cap` words in LDS)
  return 2 * ekv_align((size_t)phys_extent, 256) <= 3 * ekv_align((size_t)t_pad, 256);      // (LDS: two rows over [0, E) instead of three over [0, T))
}

// ---- chunk steps -------------------------------------------------------------------------------------------------------------------
// Two-pass scheme (16x16 kernel: statistics pass + exact pass with in-kernel column sums, ekv_attn_chunk.inc; wide-block kernel: one
// pass for output + row statistics, then a K-only column-sum pass, ekv_attn_wide.inc) for scored chunk
// steps.  It trades one extra read of K (and a third MFMA product) for the rep x n x T logits never touching HBM: at rep*n = 96
// the logits are 384 B per key against 512 B of K + V, written once and read once.  Measured on MI355X (docs/TUNING.md §8): in
// round 1 the one-pass path won at every BASELINE shape (C4 1.89 vs 2.31 ms); with the round-2 instruction diet of the MFMA
// kernel the two passes win from ~40 query rows up (C4: 1.17 vs 1.48 ms per step, stride 64: 0.43 vs 0.49), so `auto` picks
// them there.  Not with rope-on-read (every product is three MFMAs on the hi/lo pairs: C5 1.98 vs 2.59 ms).
// ekv_step.two_pass = 1 / -1 selects a scheme explicitly (every golden case runs under both).  tova needs the last query row
// itself, not column sums, and always uses the one-pass kernel.
// Round 4: with rope-on-read the two passes run on the wide-block kernel's RoPE variants (head_dim 64 / 128: K rotated in LDS, no
// logits in HBM) from the same 40 rows; head_dim 32 keeps the one-pass 16x16 kernel.
bool ekv_chunk_two_pass(int head_dim, int rep, int q_len, int policy, bool scored, bool accumulate, bool rope, int mode) {
  const bool can = q_len > 1 && scored && accumulate && policy != EKV_POLICY_TOVA && pow2_to_16(rep);   // rep query heads share a 16-lane row
  if (!can || mode < 0) return false;
  // measured crossover: 32 rows 0.34 (one pass) vs 0.36 ms, 48 rows 0.42 vs 0.41 ms.  RoPE-on-read steps keep the two passes too (round 5,
  // end): with the logits exported by the wide kernel's one pass and swept by the scorer, a configs[4] step is 2190 vs 2205 us
  return mode > 0 || ((!rope || head_dim == 64 || head_dim == 128) && (i64)rep * q_len >= 40);
}

// head_dim 256 runs the one-tile-per-wave build of the 16x16x32 kernel alone (ekv_chunk_blocks, ekv_geometry.h): a query's rep folded
// rows must fit one block of 32
bool ekv_attn_chunk_supported(int head_dim, int rep, int q_len) {
  if (head_dim == kChunkNarrowD) return rep >= 1 && rep <= kChunkNarrowRows && q_len >= 1;
  return (head_dim == 32 || head_dim == 64 || head_dim == 96 || head_dim == 128) && rep >= 1 && rep <= 128 && q_len >= 1;
}

// Wide query blocks (33..128 GQA-folded rows) run on the 32x32x16 kernel of ekv_attn_wide.inc: the dense prefix and every wide
// strided chunk step are bound by the MFMA kernel itself, not by HBM (docs/TUNING.md §3.5).  EKV_NO_WIDE=1 in the environment keeps
// the 16x16x32 kernel (A/B measurements on one box).
bool ekv_chunk_wide(int head_dim, int rep, int q_len, bool rope, bool two_pass, bool wants_logits) {
  static const bool off = env_is_1("EKV_NO_WIDE");
  if (off || q_len < 2 || (head_dim != 64 && head_dim != 128)) return false;
  int qb_rows, n_qblocks, qpw;
  ekv_chunk_blocks(rep, q_len, &qb_rows, &n_qblocks, &qpw);
  if (qpw < 2) return false;                                  // <= 32 rows: HBM-bound shapes, the small-tile kernels
  if (two_pass) return pow2_to_16(rep);                       // the column-sum pass folds the rep query heads in registers
  // only the RoPE builds export logits, and only for single-block steps (every key of the range is visited) of a power-of-two GQA factor
  return !wants_logits || (rope && n_qblocks == 1 && pow2_to_16(rep));
}

// The scorer as the tail of the wide column-sum pass holds the score rows of a head in registers (24 columns per thread of a
// 256-thread workgroup) and the selection keys in the pass's tile buffers; only heads whose column sums come from ONE workgroup
// (a last-arriver election for split heads was built and measured slower than the stand-alone scorer: ekv_wide_tail.h)
bool ekv_wide_tail_supported(i64 W, i64 n_wg) {
  static const bool off = env_is_1("EKV_NO_WIDE_TAIL");     // (A/B switch)
  return !off && W >= 1 && W <= 24 * 256 && n_wg == 1;
}

// Kernel launches of ekv_launch_attn_chunk (ekv_attn_chunk.hip) for the same arguments: the query rotation of the 16x16 RoPE path, one
// launch per pass of the wide kernel (`passes` bits), two for the 16x16 two-pass scheme.
int ekv_attn_chunk_launches(bool wide, bool rope, bool two_pass, int passes) {
  if (wide) return ((passes & 1) ? 1 : 0) + ((two_pass && (passes & 2)) ? 1 : 0);
  return (rope ? 1 : 0) + (two_pass ? 2 : 1);
}

// LDS bytes of the logits-in-LDS chunk kernel for a head_dim the manifest holds an instance of; SIZE_MAX for any other
static size_t chunk_lds_bytes(int head_dim, int rows, int phys_extent, int n_slots) {
#define EKV_CHUNK_LDS(d, elem) \
  if (head_dim == d && !EKV_IS_##elem) return ekv_chunk_lds_bytes<d>(rows, phys_extent, n_slots);
#include "ekv_instances.def"
  return SIZE_MAX;
}

// Small-row chunk step with the logits in LDS (ekv_chunk_lds.inc).  Eligible: a scored, accumulating chunk step (plain keys, score
// rows over the whole cache) with at most 8 GQA-folded query rows whose logits fit LDS next to a second workgroup of the CU (<= 80 KB),
// one victim set per head.
bool ekv_chunk_lds_supported(const ekv_bank* bank, const ekv_step* st, int phys_extent, bool scored) {
  const int rep = bank->n_q_heads / bank->n_kv_heads;
  if (st->q_len < 2 || (i64)rep * st->q_len > 8 || ((unsigned)rep & ((unsigned)rep - 1u)) != 0 || !scored || !st->accumulate || st->rope_on_read || st->score_off != 0) return false;
  if (st->phases != 0 || st->n_split == -1 || st->two_pass != 0 || !st->causal) return false;   // (two_pass = -1: "exported logits")
  if (st->policy == EKV_POLICY_TOVA && st->tova_head_mean) return false;   // needs every head of the layer first
  if (st->n_slots > kLItems * 256 || st->n_evict >= st->n_slots || st->n_evict > 16) return false;
  if (phys_extent > (1 << 20)) return false;      // (its logits alone are far beyond 80 KB; keeps the byte count below in range)
  return chunk_lds_bytes(bank->head_dim, rep * st->q_len, phys_extent, st->n_slots) <= 80 * 1024;
}

// Logits-resident scored chunk step (ekv_attn_resident.inc).  Which steps: a whole scored chunk step (roco / h2o_head, accumulating) of
// an unsplit head on plain keys, head_dim 128, GQA factor 1 / 2 / 4 / 8, 9..64 folded rows in one query block (fewer: the logits-in-LDS
// kernel) against at most 1280 keys, or at most 32 rows against at most 2560 keys.
bool ekv_attn_resident_supported(int head_dim, int rep, int q_len, int n_slots, i64 W) {
  static const bool off = env_is_1("EKV_NO_RESIDENT");     // (A/B switch)
  static const int min_rows = env_int("EKV_RESIDENT_MIN_ROWS", 9);      // (A/B switch; see the kernel's header)
  const i64 rows = (i64)rep * q_len;
  const bool shape = (rows <= 64 && n_slots <= RL<false>::TMAX) || (rows <= 32 && n_slots <= RL<true>::TMAX);      // (LONG = false / true)
  return !off && head_dim == R_D && (rep == 1 || rep == 2 || rep == 4 || rep == 8) && rows >= min_rows && shape && n_slots >= q_len && W >= 1 &&
         W <= n_slots && ekw_tail_lds_bytes(R_NT, (int)W) <= (size_t)RL<false>::OFF_P;
}

// ---- one step ----------------------------------------------------------------------------------------------------------------------
EkvScoreArgs score_args(const ekv_bank* bank, const ekv_step* st, const EkvStepPlan& P) {
  EkvScoreArgs sa{};
  sa.n_q_heads = bank->n_q_heads;
  sa.n_kv_heads = bank->n_kv_heads;
  sa.head_dim = bank->head_dim;
  sa.cap = bank->cap;
  sa.n_slots = st->n_slots;
  sa.q_len = st->q_len;
  sa.n_split = P.n_partials;
  sa.t_pad = P.t_pad;
  sa.layer_begin = st->layer_begin;
  sa.score_off = st->score_off;
  sa.policy = st->policy;
  sa.accumulate = st->accumulate;
  sa.n_evict = st->n_evict;
  sa.win_lo = st->win_lo;
  sa.win_tail = st->win_tail;
  sa.roco_k1 = st->roco_k1;
  sa.roco_tail = st->roco_tail;
  sa.range_start = st->range_start;
  sa.tova_head_mean = st->tova_head_mean;
  sa.causal = st->causal;
  sa.count_add = st->count_add;
  sa.count_tail_step = st->count_tail_step;
  sa.o_ts = P.strides[4], sa.o_hs = P.strides[5];
  sa.n_col_parts = P.n_col_parts;
  sa.big_stride = P.t_pad;
  return sa;
}

namespace {

// What every stage of ekv_plan_step reads of a step that has something to tile.
struct StepShape {
  const ekv_bank* bank;
  ekv_step st;            // the caller's step without the slot-layout phase bits
  bool slot_rows;         // EKV_PHASE_SLOT_ROWS: the bank's score rows are in the slot-indexed layout (ekv_rows_to_slots)
  bool slot_tail_ok;      // EKV_PHASE_SLOT_TAIL_OK
  bool scored;
  int T, n, D, rep;
  i64 W;                  // score columns
  int LC;                 // layers the workspace is laid out for: all deferred layers (ekv_step.defer_layers), whatever this call launches
  int max_rows;           // rows an unsplit chunk workgroup may walk (its slot entries live in LDS): 6144 with RoPE-on-read, 16384 plain
  bool long_rows;         // a long call (ekv_plan_step): the long-row scorer where the plan would end in the generic one
  bool capped;            // a capped call (ekv_plan_step): chunk steps on the one-tile build of the 16x16x32 kernel alone
  bool no_orders;         // the call runs instances without the phase order K (quantised rows, a batch, sinks): no two-round launch
  int Dblk;               // the head_dim a chunk step's query blocks are cut for: D, or kChunkNarrowD for a capped call (blocks of <= 32 rows)
  bool pooled;            // a pooled call (resolve_call): the step ends in the generic scorer — no one-launch kernel, no in-kernel scorer tail
};

// ---- stage 1: tiling
void plan_tiling(const StepShape& s, EkvStepPlan* P) {
  const ekv_bank* bank = s.bank;
  const ekv_step* st = &s.st;
  const int T = s.T, n = s.n, D = s.D, rep = s.rep;
  // (head, layer) pairs of the launch; every rule below compares it, or a small multiple, with at most 1024: capped so that products stay in range
  const i64 heads = std::min<i64>((i64)s.LC * bank->n_kv_heads, 1 << 20);
  P->t_pad = (int)ekv_align((size_t)T, 64);
  P->qb_rows = P->n_qblocks = 1;
  int qpw = 1;
  if (n > 1) ekv_chunk_blocks(rep, n, &P->qb_rows, &P->n_qblocks, &qpw, s.Dblk);
  // physical extent E of the step (every live row has a physical index < E): the caller's value when it is consistent, else cap
  P->phys_extent = (st->phys_extent >= T && st->phys_extent <= bank->cap) ? st->phys_extent : bank->cap;
  // pitch of a logits row in the fused decode kernel's LDS: logical positions (RoPE-on-read streams in position order, the rotation
  // needs the position index) or physical rows [0, E)
  P->l_pad = st->rope_on_read ? P->t_pad : (int)ekv_align((size_t)P->phys_extent, 64);
  const int wg_unit = n == 1 ? 128 : 64;
  i64 n_split = st->n_split;
  // (the 5-column 8-wave instance with both phase orders, two workgroups per CU: what a launch of 1024 heads or more runs in two rounds)
  const bool rounds_shape = n == 1 && D == 128 && rep == 1 && !st->rope_on_read && s.slot_rows && s.scored && !s.no_orders && P->phys_extent <= 2304;
  P->fused_nw = ekv_decode_fused_nw(heads, rounds_shape);
  if (n_split <= 0 && n == 1 && heads >= 256 && P->fused_nw == 8 && !s.pooled &&
      ekv_decode_fused_supported(D, rep, T, P->t_pad, P->l_pad, st->n_evict, bank->cap, 8)) {
    n_split = 1;   // >= 1 head per CU: one 8-wave workgroup per head beats key-range splits + a second kernel (GQA shapes)
  }
  // A whole scored step small enough for the logits-resident kernel (ekv_attn_resident.inc: one launch, one workgroup per head, K and V
  // read once) runs there, unsplit, whatever the number of heads in the launch.  Measured per step (us, resident / two passes): 256
  // (head, layer) pairs of configs[2] 49.8 / 81.9-82.4; 1024 pairs of 64 rows x 1152 keys 193.7-197.0 / 225.3-226.2; blocks of 9..32
  // rows against the 16x16 kernel + scorer tail: 256 pairs, 32 / 16 rows 44.0 / 43.3 against 71.5-73.9 / 61.5-62.2; <= 32 rows x 2064 keys
  // 63.7-64.0 against 110.7-111.8.  Not for steps that force a scheme or a split, run in phases or defer their scorer (a layer-per-call
  // model: those launches hold 8..32 heads, and their column-sum pass + scorer run once over all layers).  The kernel's scorer is the
  // wide column-sum pass's tail (ekv_wide_tail.h): where that tail is off (EKV_NO_WIDE_TAIL) the step is planned as any other.  It is
  // laid out as an unsplit two-pass step of the wide-block kernel (the workspace of one is never touched).
  P->resident = (n > 1 && !s.capped && !s.pooled && st->phases == 0 && !s.slot_rows && st->defer_layers == 0 && st->two_pass == 0 && n_split <= 1 &&
                 (st->policy == EKV_POLICY_H2O_HEAD || st->policy == EKV_POLICY_ROCO) && st->accumulate && !st->rope_on_read &&
                 P->n_qblocks == 1 && st->score_off >= 0 && st->score_off < T && ekv_attn_resident_supported(D, rep, n, T, s.W) &&
                 ekv_wide_tail_supported(s.W, 1)) ? 1 : 0;
  if (P->resident) n_split = 1;
  P->two_pass = (P->resident || (n > 1 && ekv_chunk_two_pass(D, rep, n, st->policy, s.scored, st->accumulate != 0, st->rope_on_read != 0, st->two_pass))) ? 1 : 0;
  P->wide = (P->resident || (n > 1 && !s.capped && ekv_chunk_wide(D, rep, n, st->rope_on_read != 0, P->two_pass, !P->two_pass && s.scored && st->accumulate != 0))) ? 1 : 0;
  if (n_split <= 0 && n > 1) {
    // Chunk steps (two or three workgroups per CU): a split costs a partial per query row and split, a fold in the scorer and a
    // shorter stream per workgroup, so the grid is filled to the 256..512 workgroups that are resident at a time — not to 1024:
    // the fewest splits (powers of two, <= 8) that give every CU a workgroup, doubled once more if a split then still streams
    // >= 1024 rows.  Measured (us per step, MI355X, round 3 sweep; this rule / what the 1024- or 3072-target picked):
    //   wide kernel, 8 KV heads x 1 layer, 64 rows, T = 1248 / 2176 / 5098:  46.7 / 54.7 / 76.2   (50.0 / 61.4 / 84.8)
    //   wide kernel, 32 heads x 1 layer, 96 rows:                            63.9 / 76.6 / 110.5  (69.6 / 91.6 / 155.9)
    //   wide kernel, 128 (head, layer) pairs, 96 rows:                       97.8 / 110.8 / 182.0 (108.6 / 132.5 / 208.6)
    //   wide kernel, 256 pairs (configs[2]: 8 KV heads x 32 layers):         87.2 / 131.7 / 239.7 (116.3 / 154.1 / 265.4)
    //   RoPE-on-read (16x16 kernel), 32 heads x 1 layer, 96 rows, T = 2176 / 4205:  127.4 / 166.4  (152.3 / 228.7)
    //   16x16 kernel, GQA x4 stride 8 (32 rows), 64 pairs, T = 2176 / 4205:  57.9 / 87.9   (72.9 / 110.0);  256 pairs: 109.4 / 190.4 (126.8 / 207.5)
    //   16x16 kernel, stride 16 MHA, 256 pairs:                              93.3 / 155.6  (99.4 / 173.0)
    const i64 wgs = heads * P->n_qblocks;
    n_split = 1;
    while (wgs * n_split < 256 && n_split < 8) n_split *= 2;
    if (wgs * n_split < 512 && n_split < 8 && T / (2 * n_split) >= 1024) n_split *= 2;
    n_split = std::max<i64>(1, std::min<i64>(n_split, ((i64)T + 255) / 256));
  }
  if (n_split <= 0) {      // decode: >= 1024 workgroups (4 per CU, one round), never fewer than 128 positions per split
    n_split = std::max<i64>(1, std::min<i64>((1024 + heads - 1) / heads, ((i64)T + 127) / 128));
    // decode launches of a few heads (one layer per call): the launch is latency-bound and ends with the fold of the key-range
    // partials, whose loads go out in batches of 8 — up to 8 splits are ONE round trip.  Measured at 32 heads, T = 2049
    // (us per layer, attention + in-kernel fold): 5 splits 15.4, 6..8 13.7, 10..17 14.6..14.7.
    if (n_split > 8 && heads * 8 >= 256) n_split = 8;
  }
  // the chunk kernel caches the slot indices of its key range in LDS next to its tiles and query block: bound the range (an unsplit
  // 32 k-slot head would need 128 KB of indices alone; split heads fold through the partials instead)
  if (n > 1) n_split = std::max<i64>(n_split, ((i64)T + s.max_rows - 1) / s.max_rows);
  P->rows_per_split = (int)ekv_align((size_t)(((i64)T + n_split - 1) / n_split), wg_unit);
  P->n_split = (int)(((i64)T + P->rows_per_split - 1) / P->rows_per_split);
  // partials per query row: one per split (decode, wide chunk kernel) or one per split and key half (16x16 chunk kernel)
  P->n_partials = (n == 1 || P->wide) ? P->n_split : 2 * P->n_split;
  if (P->wide) {
    // the column-sum pass of the wide kernel walks the query blocks of a (head, key range) inside the workgroup and leaves ONE row of
    // column sums; a launch of few (head, layer) pairs (one layer of a decoder stack) spreads them over up to 16 workgroups
    const i64 wgs = heads * P->n_split;
    P->n_col_parts = (int)std::max<i64>(1, std::min<i64>(std::min(P->n_qblocks, 16), (512 + wgs - 1) / wgs));
  } else {      // column-sum partial rows per head: query-tile waves per workgroup x query blocks
    P->n_col_parts = (int)((i64)ekv_chunk_col_parts(qpw, st->rope_on_read != 0) * P->n_qblocks);
  }
  // unsplit chunk steps fold the two key halves inside the attention kernel (one-pass scored steps also get the final row
  // statistics from it)
  P->fold_in_kernel = (n > 1 && P->n_split == 1) ? 1 : 0;
}

// ---- stage 2: workspace layout
void plan_layout(const StepShape& s, EkvStepPlan* P) {
  const ekv_bank* bank = s.bank;
  const ekv_step* st = &s.st;
  const int n = s.n, D = s.D;
  const size_t LC = (size_t)s.LC;
  const size_t rowsq = LC * bank->n_q_heads * n;
  size_t off = 0;
  auto carve = [&](int64_t& at, bool present, size_t bytes) {
    at = present ? (int64_t)off : -1;
    if (present) off += ekv_align(bytes, 256);
  };
  // statistics partials + column sums instead of the logits (two passes); the scorer only needs the logits when it accumulates
  carve(P->stats, P->two_pass, rowsq * P->n_partials * 2 * 4);
  carve(P->colsum, P->two_pass, LC * bank->n_kv_heads * P->n_col_parts * 2 * P->t_pad * 4);
  carve(P->logits, !P->two_pass && s.scored && st->accumulate, rowsq * P->t_pad * 4);
  carve(P->partials, true, rowsq * P->n_partials * ((size_t)D + 2) * 4);
  carve(P->tova_row, true, LC * P->t_pad * 4);
  // W > ~10 000: rows in scratch, keys in LDS
  carve(P->big_rows, s.scored && ekv_score_rows_exceed_lds(s.W, P->two_pass ? 0 : (i64)s.rep * n), LC * bank->n_kv_heads * 3 * P->t_pad * 4);
  // one-pass scored steps with the in-kernel fold: the scorer still needs (M, L) per row
  carve(P->row_stats, P->fold_in_kernel && !P->two_pass && s.scored && st->accumulate, rowsq * 2 * 4);
  // deferred scorer of a layer-per-call model, wide two-pass chunk steps: the column-sum pass is deferred with it (one launch over
  // all layers at the flush instead of a 256-workgroup launch per layer) — it needs every layer's raw queries
  carve(P->q_keep, st->defer_layers > 0 && n > 1 && P->wide && P->two_pass, rowsq * D * 2);
  // (16x16 kernel only: the wide-block kernel rotates Q in its prologue)
  carve(P->q_rot, st->rope_on_read && n > 1 && !P->wide, 2 * rowsq * D * 2);
  P->bytes = off;
}

// ---- stage 3: argument checks, in the order the call reports them; fills in the row strides and, for a deferred call, moves the
// layout's offsets to the call's slice
int plan_checks(const StepShape& s, int bank_rc, EkvStepPlan* P) {
  const ekv_bank* bank = s.bank;
  const ekv_step* st = &s.st;
  const int T = s.T, n = s.n, D = s.D;
  const i64 W = s.W;
  if (bank_rc) return bank_rc;
  if (int e = check_layers(bank, st->layer_begin, st->layer_count)) return e;
  if (T < n || T > bank->cap || st->n_evict < 0 || st->n_evict >= T) return EKV_E_ARG;
  if (s.scored && (!bank->score_sum || st->score_off < 0 || st->score_off >= T)) return EKV_E_ARG;
  if (st->policy == EKV_POLICY_ROCO && (!bank->score_sq || !bank->score_cnt)) return EKV_E_ARG;
  if (st->policy < EKV_POLICY_NONE || st->policy > EKV_POLICY_RANGE) return EKV_E_ARG;
  if (st->n_evict > 0) {
    if (st->policy == EKV_POLICY_NONE) return EKV_E_ARG;
    if (st->policy == EKV_POLICY_RANGE && (st->range_start < 0 || (i64)st->range_start + st->n_evict > T)) return EKV_E_ARG;
    if (st->policy == EKV_POLICY_ROCO && (st->roco_k1 < st->n_evict || st->roco_k1 > W)) return EKV_E_ARG;
    if ((st->policy == EKV_POLICY_H2O_HEAD || st->policy == EKV_POLICY_TOVA) &&
        (st->win_lo < 0 || st->win_tail < 0 || W - st->win_tail - st->win_lo < st->n_evict))
      return EKV_E_ARG;
  }
  // row strides (ABI 8): both zero = dense; q_len = 1 makes the token stride irrelevant and only takes head rows head_dim apart
  const int32_t strides[6] = {st->q_token_stride, st->q_head_stride, st->kv_token_stride, st->kv_head_stride, st->out_token_stride, st->out_head_stride};
  for (int i = 0; i < 6; i += 2) {
    int32_t ts = strides[i], hs = strides[i + 1];
    if (ts < 0 || hs < 0) return EKV_E_ARG;
    if (n == 1) {
      if (hs != 0 && hs != D) return EKV_E_UNSUPPORTED;
      ts = hs = 0;
    }
    if (ts == 0 && hs == 0) {
      ts = D;
      hs = (int32_t)((i64)n * D);
    } else if (ts < D || hs < D || (ts & 7) || (hs & 7)) {
      return EKV_E_ARG;
    }
    P->strides[i] = ts, P->strides[i + 1] = hs;
  }
  if (st->defer_layers != 0) {   // deferred scorer: decode AND chunk steps (ABI 5), explicit splits, attention + fold now / scorer later
    if (st->defer_layers < 0 || st->defer_index < 0 || (i64)st->defer_index + st->layer_count > st->defer_layers || st->n_split <= 0 ||
        (st->phases != (1 | 4) && st->phases != 8))
      return EKV_E_ARG;
    // this call's slice of the per-layer arrays; chunk steps: what the deferred scorer reads of the attention launches — column sums
    // (two passes) or row statistics (one pass)
    const size_t rows0 = (size_t)st->defer_index * bank->n_q_heads * n, li = st->defer_index;
    auto slice = [](int64_t& at, size_t bytes) { if (at >= 0) at += (int64_t)bytes; };
    slice(P->logits, rows0 * P->t_pad * 4);
    slice(P->partials, rows0 * P->n_partials * ((size_t)D + 2) * 4);
    slice(P->tova_row, li * P->t_pad * 4);
    slice(P->big_rows, li * bank->n_kv_heads * 3 * P->t_pad * 4);
    slice(P->stats, rows0 * P->n_partials * 2 * 4);
    slice(P->colsum, li * bank->n_kv_heads * P->n_col_parts * 2 * P->t_pad * 4);
    slice(P->row_stats, rows0 * 2 * 4);
    slice(P->q_keep, rows0 * D * 2);
  }
  // head_dim 256: plain keys only — no RoPE-on-read build of the decode stream or of the chunk kernel exists at that head_dim
  if (D == kChunkNarrowD && st->rope_on_read) return EKV_E_UNSUPPORTED;
  return EKV_OK;
}

void run(EkvStepPlan* P, int32_t kind, int32_t kernels, int32_t skip_fold = 0, int32_t passes = 0, bool fuse = false, bool tail = false) {
  P->list[P->n_list++] = EkvLaunch{kind, kernels, skip_fold, passes, fuse ? 1 : 0, tail ? 1 : 0};
  P->n_launches += kernels;
}

// ---- stage 4a: the steps that are ONE launch whatever their phases say.  Returns true when the step is settled (*rc is the call's code).
bool plan_whole_step(const StepShape& s, EkvStepPlan* P, int* rc) {
  const ekv_bank* bank = s.bank;
  const ekv_step* st = &s.st;
  const i64 heads_now = (i64)st->layer_count * bank->n_kv_heads;
  *rc = EKV_OK;
  // whole decode step in one launch when no head has to be split
  if (s.n == 1 && st->phases == 0 && P->n_split == 1 && !s.pooled &&
      ekv_decode_fused_supported(s.D, s.rep, s.T, P->t_pad, P->l_pad, st->n_evict, bank->cap, P->fused_nw)) {
    if (s.slot_rows && !ekv_slot_rows_supported(bank, st, P->phys_extent, P->t_pad)) {
      *rc = EKV_E_UNSUPPORTED;
      return true;
    }
    P->slot_rows = s.slot_rows ? 1 : 0;
    P->slot_tail_ok = s.slot_rows && s.slot_tail_ok ? 1 : 0;
    P->one_launch = 1;
    P->fused_order = ekv_decode_fused_order(s.D, s.rep, s.scored, s.slot_rows, P->fused_nw, heads_now, P->phys_extent);
    // resident rows: the instances that read them (ekv_attn_decode.inc, kResident) — 16-bit rows (resolve_call clears the field for the
    // quantised and the batch calls), head_dim 128, one query head per KV head, slot-indexed score rows (so plain keys, physical order)
    if (s.D == 128 && s.rep == 1 && s.slot_rows && !st->rope_on_read)
      P->fused_order |= EKV_RESIDENT_BITS(ekv_decode_resident_rows(heads_now, 2 * s.D, P->phys_extent, bank->cap,
                                                                   st->policy == EKV_POLICY_ROCO ? 3 : 1, ekv_resident_budget_bytes()));
    run(P, EKV_RUN_FUSED_DECODE, 1);
    return true;
  }
  if (s.slot_rows) {      // every other kernel reads the ordered layout: ekv_rows_to_order first
    *rc = EKV_E_UNSUPPORTED;
    return true;
  }
  // small-row chunk step (configs[1]: stride 8): one launch, logits in LDS, K and V read once
  if (s.n > 1 && !s.capped && !s.pooled && ekv_chunk_lds_supported(bank, st, P->phys_extent, s.scored) && (heads_now >= 256 || s.T <= 1024)) {
    P->one_launch = 1;
    run(P, EKV_RUN_CHUNK_LDS, 1);
    return true;
  }
  return false;
}

// How a step that is not one launch by itself ends (plan_ending): which scorer runs, and where.
struct StepEnding {
  bool fuse_chunk;      // the scorer runs as the tail of the 16x16 one-pass kernel: the whole chunk step is ONE launch
  bool flush_colsum;    // the flush of a deferred wide two-pass step: the column-sum pass of all layers runs now
  bool tail_step;       // the scorer runs as the tail of the wide column-sum pass (ekv_wide_tail.h)
  bool fold_only;       // nothing to score and nothing to evict ('full', any unknown policy string), or phases = attention + fold
  bool range_only;      // 'recency' / 'random': no score rows at all, only the slot map is compacted — any cache length
  bool fast_scorer;     // decode steps: the split path's fast scorer (ekv_decode_score.inc)
};

// ---- stage 4b: how the step ends, decided BEFORE anything is launched: a shape no scorer can take must be refused while the bank is
// still untouched (the attention kernel appends the new rows).  Also settles flush_unsplit and fold_in_decode.
int plan_ending(const StepShape& s, EkvStepPlan* P, StepEnding* end) {
  const ekv_bank* bank = s.bank;
  const ekv_step* st = &s.st;
  const int T = s.T, n = s.n, D = s.D, rep = s.rep;
  const i64 W = s.W;
  const bool scored = s.scored;
  // phases: 0 = whole step; else a bit mask: 1 attention kernel, 2 scorer (fold + score), 4 fold only, 8 scorer
  // without the fold (4 and 8 let the caller run the scorer on a side stream, off the critical path)
  const int ph = st->phases;
  if (ph < 0 || ph > 15 || ((ph & 2) && (ph & (4 | 8)))) return EKV_E_ARG;
  // the scorer's LDS footprint reads the shape and whether column sums / scratch rows replace the logits / LDS rows
  static float present;      // (an address for "is there", never dereferenced)
  EkvScoreArgs shape = score_args(bank, st, *P);
  shape.colsum = P->colsum >= 0 ? &present : nullptr;
  shape.big_rows = P->big_rows >= 0 ? &present : nullptr;
  // Whole chunk step in ONE launch: unsplit heads (the kernel folds its own output), one-pass logits, a scored policy, and the
  // scorer's LDS rows fit next to two workgroups per CU.  The scorer of a head then runs as the tail of the workgroup that
  // streamed it and overlaps the K/V stream of the workgroups still running (tova_head_mean needs all heads of a layer first).
  // (not on the wide-block kernel: it has no scorer tail — an unsplit scored step of 33..64 rows that exports no logits, i.e. the
  //  first strided chunk of an encoding-mode prefill, runs as wide attention + scorer launch)
  const bool fuse_chunk = n > 1 && ph == 0 && !s.pooled && P->fold_in_kernel && !P->two_pass && !P->wide && scored && P->n_qblocks == 1 &&
                          (i64)rep * n <= 64 && !(st->policy == EKV_POLICY_TOVA && st->tova_head_mean && st->accumulate) &&
                          ekv_score_lds_bytes(256, shape) <= 64 * 1024 && st->n_split != -1;
  // Two-pass step on the wide-block kernel (whole step, or the flush of a layer-per-call step whose column-sum pass was deferred):
  // the scorer runs as the TAIL of the column-sum pass (ekv_wide_tail.h, round 5) — score rows in registers, keys in the pass's
  // tile buffers, four workgroups per CU — instead of a 1024-thread-per-CU scorer launch behind it.  Only for heads whose column sums
  // come from one workgroup (no key-range splits, one query-block group): split heads keep the stand-alone scorer (measured faster).
  // Not with RoPE-on-read: those passes run two workgroups per CU, where a head's ~50 us tail costs more stream than the launch it saves.
  const bool flush_colsum = (ph & 8) && !(ph & 1) && n > 1 && P->q_keep >= 0;
  // The flush's column-sum launch covers ALL deferred layers: with >= 512 (head, layer, query-block group) units it runs UNSPLIT whatever
  // key-range split the one-layer calls of the one pass used (that split exists to fill the chip from 32 heads) — 1024 workgroups in one
  // resident round instead of 8192 short ones, and the scorer as its tail.
  // ADVICE r5 asked for this branch to be tied to the tail or measured on its own.  Measured (round 6, one layer per call, flush over 40
  // layers x 40 heads, configs[4] shape with RoPE-on-read, where the tail does NOT run): unsplit flush 92.4-93.0 us per layer against
  // 94.1-94.8 us with the one-layer calls' key-range split kept — so a flush runs unsplit WHENEVER the key range fits what an unsplit
  // workgroup may walk (the row bound the tiling applies to n_split: slot entries of the range live in LDS — 6144 rows with
  // RoPE-on-read, 16384 plain), tail or not; beyond that bound it keeps the split.
  const bool tail_shape = n > 1 && P->wide && P->two_pass && P->big_rows < 0 && scored && st->accumulate &&
                          st->policy != EKV_POLICY_TOVA && !st->rope_on_read;
  P->flush_unsplit = flush_colsum && P->wide && P->two_pass && T <= s.max_rows &&
                     (size_t)st->layer_count * bank->n_kv_heads * P->n_col_parts >= 512;
  const i64 tail_wgs = (i64)(P->flush_unsplit ? 1 : P->n_split) * P->n_col_parts;
  const bool tail_step = tail_shape && !s.pooled && (ph == 0 || flush_colsum) && ekv_wide_tail_supported(W, tail_wgs);

  const bool wants_scorer = ph == 0 || (ph & (2 | 8));
  const bool fold_only = (!scored && st->n_evict == 0) || !wants_scorer;
  const bool range_only = wants_scorer && st->policy == EKV_POLICY_RANGE;
  const bool fast_scorer = wants_scorer && !fold_only && !range_only && !fuse_chunk && !s.pooled && ekv_decode_score_supported(shape);
  const bool generic_scorer = wants_scorer && !fold_only && !range_only && !fuse_chunk && !fast_scorer;
  if (generic_scorer && !s.long_rows && ekv_score_lds_bytes(shape.big_rows != nullptr ? 1024 : 512, shape) > 160 * 1024)
    return EKV_E_UNSUPPORTED;   // even the selection keys alone exceed one CU's LDS (W > ~39 000): see DESIGN.md "size limits"
  // (a long call: the keys are in scratch, so no width bound; what its sweep keeps in LDS is the (M, 1 / L) pair of every logits row —
  //  the term the bound above also carries, and the same 160 KB)
  if (generic_scorer && s.long_rows && ekv_long_sweep_lds(shape.colsum != nullptr ? 0 : (i64)rep * n) > 160 * 1024) return EKV_E_UNSUPPORTED;
  if (n == 1 ? !ekv_attn_decode_supported(D, rep) : !ekv_attn_chunk_supported(s.Dblk, rep, n)) return EKV_E_UNSUPPORTED;
  // the 16x16x32 chunk kernel keeps the slot entries of its key range, its K/V tiles and (some builds) the query block in LDS: one CU's
  // 160 KB bound every launch of the step (ekv_chunk_step_lds, ekv_geometry.h — the arithmetic its launcher sizes the launch with).  The
  // row bound of the tiling (max_rows) keeps every head_dim up to 256 inside it; a step beyond it is refused here, not at the launch.
  if (n > 1 && !P->wide && !P->resident) {
    int qb_rows, n_qblocks, qpw;
    ekv_chunk_blocks(rep, n, &qb_rows, &n_qblocks, &qpw, s.Dblk);
    if (ekv_chunk_step_lds(D, qpw, st->rope_on_read != 0, P->two_pass != 0, P->rows_per_split, P->fold_in_kernel != 0) > 160 * 1024)
      return EKV_E_UNSUPPORTED;
  }

  // decode split path whose partials are folded right behind the attention kernel (attention + fold phases, or a step that has
  // nothing to score): the last-arriving split of a head folds them inside the attention kernel — no fold launch
  // (GQA factors > 8 run several query-head groups per KV head, ekv_attn_decode.inc: the arrival counter counts one group's splits)
  P->fold_in_decode = n == 1 && rep <= 8 && bank->arrive != nullptr && (ph == 0 || (ph & 1)) && !P->fold_in_kernel &&
                      ((ph & 4) || (ph == 0 && (fold_only || range_only)));
  *end = StepEnding{fuse_chunk, flush_colsum, tail_step, fold_only, range_only, fast_scorer};
  return EKV_OK;
}

// ---- stage 4c: attention launches, fold and scorer, by the step's phases
int plan_launches(const StepShape& s, EkvStepPlan* P) {
  StepEnding end;
  if (int e = plan_ending(s, P, &end)) return e;
  const ekv_step* st = &s.st;
  const int n = s.n, ph = st->phases;
  const bool fuse_chunk = end.fuse_chunk, flush_colsum = end.flush_colsum, tail_step = end.tail_step, fold_only = end.fold_only,
             range_only = end.range_only, fast_scorer = end.fast_scorer;
  const bool rope = st->rope_on_read != 0;
  if (ph == 0 || (ph & 1)) {
    if (n == 1) {
      run(P, EKV_RUN_DECODE, 1);
    } else if (P->resident) {
      // small enough for the logits to stay in the register file: one launch, K and V read once (ekv_attn_resident.inc)
      P->one_launch = 1;
      run(P, EKV_RUN_RESIDENT, 1);
      return EKV_OK;
    } else if (tail_step && ph == 0) {
      // one pass (output / partials + row statistics) -> fold of the key-range partials, if any -> column-sum pass with the scorer as
      // its tail: two launches for an unsplit head
      run(P, EKV_RUN_CHUNK, ekv_attn_chunk_launches(P->wide, rope, true, 1), 1, 1);
      if (!P->fold_in_kernel) run(P, EKV_RUN_FOLD, 1, 1);
      run(P, EKV_RUN_CHUNK, ekv_attn_chunk_launches(P->wide, rope, true, 2), 1, 2, false, true);
      return EKV_OK;
    } else {
      // (deferred wide two-pass step: only the one pass now — the column-sum pass runs with the scorer at the flush)
      const int passes = P->q_keep >= 0 ? 1 : 3;
      run(P, EKV_RUN_CHUNK, ekv_attn_chunk_launches(P->wide, rope, P->two_pass, passes), fuse_chunk ? 1 : 0, passes, fuse_chunk);
    }
  }
  if (fuse_chunk) P->one_launch = 1;
  if (ph == 1 || fuse_chunk) return EKV_OK;

  if ((ph & 4) || fold_only || range_only) {
    // (not even the fold when the attention kernel has already written the output)
    if ((!(ph & 8) || (ph & 4)) && !P->fold_in_kernel && !P->fold_in_decode) run(P, EKV_RUN_FOLD, 1);
    if (fold_only) return EKV_OK;
  }
  if (range_only) {
    if (st->n_evict > 0) run(P, EKV_RUN_RANGE, 1);
    return EKV_OK;
  }
  if (flush_colsum) {
    // the flush of a deferred chunk step: the column-sum pass of ALL layers (queries from the kept copies, the chunk's own rows from
    // the cache slots the one pass of each layer wrote them to), then the scorer — as the tail of that pass where it can be
    run(P, EKV_RUN_FLUSH, ekv_attn_chunk_launches(P->wide, rope, true, 2), 0, 2, false, tail_step);
    if (tail_step) return EKV_OK;
  }
  const int skip_fold = ((ph & 8) || P->fold_in_kernel) ? 1 : 0;
  if (fast_scorer) {   // decode steps: the fast scorer (same tail as the fused kernel)
    run(P, EKV_RUN_DECODE_SCORE, 1, skip_fold);
    return EKV_OK;
  }
  // a long call, exactly here: a fold launch of its own where the generic scorer would have folded the output, then sweep + select in
  // place of the generic scorer's launch.  `passes` of the two entries: 1 = the plain plan keeps its score rows in scratch (which build
  // of the generic scorer the plain call runs, and with it the batches its fold takes the partials in: ekv_score_select_threads)
  const int plain_big = P->big_rows >= 0 ? 1 : 0;
  if (s.long_rows && !skip_fold) run(P, EKV_RUN_LONG_FOLD, 1, 0, plain_big);
  if (st->policy == EKV_POLICY_TOVA && st->tova_head_mean && st->accumulate) run(P, EKV_RUN_TOVA_MEAN, 1, skip_fold);
  if (s.long_rows) {
    run(P, EKV_RUN_LONG_SCORE, 2, 1, plain_big);
    P->long_rows = 1;
    P->long_tiles = (int32_t)ekv_long_tiles(s.W);
    return EKV_OK;
  }
  run(P, EKV_RUN_SCORE_SELECT, 1, skip_fold);
  return EKV_OK;
}

// ---- stage 5, long calls only: the scratch of the long-row scorer, BEHIND everything the plain layout holds (every other offset, and
// with it every other kernel's view of the workspace, is the plain call's): the working copies of the score rows unless the plain
// layout has them already, then the selection keys, one row of t_pad words per (layer, head); a deferred call's slices as in plan_checks
void plan_long_layout(const StepShape& s, EkvStepPlan* P) {
  const size_t LC = (size_t)s.LC, H = (size_t)s.bank->n_kv_heads, li = s.st.defer_layers != 0 ? (size_t)s.st.defer_index : 0;
  size_t off = P->bytes;
  if (P->big_rows < 0) {
    P->big_rows = (int64_t)(off + li * H * 3 * P->t_pad * 4);
    off += ekv_align(LC * H * 3 * P->t_pad * 4, 256);
  }
  P->key_rows = (int64_t)(off + li * H * P->t_pad * 4);
  off += ekv_align(LC * H * P->t_pad * 4, 256);
  P->bytes = off;
}

}  // namespace

// The whole dispatch of ekv_step_attend for a step, in four stages: the tiling, the workspace layout, the argument / shape / capability
// checks (the return code of the call, in the order the call reports them) and the launch sequence (whole-step kernels, else ending + launches).  The tiling and the layout are
// filled in for every step that has something to tile, also when the step is refused (ekv_workspace_bytes and ekv_step_info report them).
//
// Long rows (the ekv_long_* calls), the rule of the family stated once: a long call plans exactly as the plain call of the same (bank,
// step, dtype) — tiling, layout, checks, whole-step kernels, ending — except that wherever that plan would end in EKV_RUN_SCORE_SELECT
// (whole steps, phases & 2, phases & 8, the deferred flush over all layers) it ends in the long-row scorer (ekv_score_long.inc:
// EKV_RUN_LONG_SCORE, two kernels; a preceding EKV_RUN_TOVA_MEAN stays; EKV_RUN_LONG_FOLD in front where the generic scorer would have
// folded the output itself), the width refusal of plan_ending does not apply, and the workspace grows by that scorer's scratch
// (plan_long_layout).  A step that ends anywhere else plans field for field as the plain call.
int ekv_plan_step(const ekv_bank* bank, const ekv_step* step, EkvStepPlan* P, bool long_rows, bool capped, bool no_orders, bool pooled) {
  *P = EkvStepPlan{};
  P->key_rows = -1;
  const int bank_rc = check_bank(bank);
  if (!bank || !step) return bank_rc ? bank_rc : EKV_E_ARG;
  StepShape s{};
  s.bank = bank;
  // EKV_PHASE_SLOT_ROWS: the bank's score rows are in the slot-indexed layout (ekv_rows_to_slots) — only the one-launch decode step
  // runs on it; every stage sees the remaining phase bits
  s.slot_rows = (step->phases & EKV_PHASE_SLOT_ROWS) != 0;
  s.slot_tail_ok = (step->phases & EKV_PHASE_SLOT_TAIL_OK) != 0;
  s.st = *step;
  s.st.phases &= ~(EKV_PHASE_SLOT_ROWS | EKV_PHASE_SLOT_TAIL_OK);
  s.T = step->n_slots, s.n = step->q_len, s.D = bank->head_dim;
  if (bank->n_kv_heads <= 0 || step->layer_count < 1 || s.n < 1 || s.T < 1) return bank_rc ? bank_rc : EKV_E_ARG;   // (nothing to tile)
  s.rep = bank->n_q_heads / bank->n_kv_heads;
  s.scored = step->policy == EKV_POLICY_H2O_HEAD || step->policy == EKV_POLICY_ROCO || step->policy == EKV_POLICY_TOVA;
  s.W = (i64)s.T - (s.scored ? step->score_off : 0);
  s.LC = step->defer_layers > 0 ? step->defer_layers : step->layer_count;
  s.max_rows = step->rope_on_read ? 6144 : 16384;
  s.long_rows = long_rows;
  s.no_orders = no_orders;
  s.capped = capped;
  s.pooled = pooled;
  s.Dblk = capped ? kChunkNarrowD : s.D;

  plan_tiling(s, P);
  plan_layout(s, P);
  if (int e = plan_checks(s, bank_rc, P)) return e;
  int rc;
  if (plan_whole_step(s, P, &rc)) return rc;
  rc = plan_launches(s, P);
  if (rc == EKV_OK && P->long_rows) plan_long_layout(s, P);
  return rc;
}

// ---- one call ----------------------------------------------------------------------------------------------------------------------
// What each row format takes, beyond decode steps (q_len == 1) on plain keys — all a quantised bank serves: its head_dims (0: none) and
// the largest GQA factor.  kv8: head_dim 64 / 128.  kv4: head_dim 128 (a lane's 16-byte piece = one 32-element block), GQA factors up
// to 4 (32 output floats per lane and head).  kv6: the geometry of kv4, so its shapes.  kv84: head_dim 128 (its V blocks), GQA factors as kv8 takes them (its geometry).  kv164: head_dim 128 (its V blocks), every GQA factor (the 16-bit geometry and plan).  resolve_call refuses by it, and the bank conversions (ekv_abi.hip) ask for the head_dim.
namespace {
struct RowsRule {
  int32_t head_dims[2], max_rep;
};
const RowsRule kRowsRules[] = {/* kv16 */ {{0, 0}, 1 << 30}, /* kv8 */ {{64, 128}, 1 << 30}, /* kv4 */ {{128, 0}, 4}, /* kv6 */ {{128, 0}, 4}, /* kv84 */ {{128, 0}, 1 << 30}, /* kv164 */ {{128, 0}, 1 << 30}};
}  // namespace
bool ekv_rows_head_dim(EkvRows rows, int head_dim) {
  const RowsRule& rule = kRowsRules[rows];
  return head_dim > 0 && (head_dim == rule.head_dims[0] || head_dim == rule.head_dims[1]);
}

// The return code of the call, in the order the call reports its errors.  Stages: element type -> the bank a quantised call runs on ->
// envelope and table of a batch -> the plan of the (16-bit, uniform) step -> what the row format and the batching do not take.
//
// The element type only picks the kernel instances: a bf16 step is planned as the fp16 step.  RoPE-on-read keeps hi / lo fp16 planes
// of the rotated keys and queries (ekv_attn_wide.inc, ekv_rope_q_kernel) and has no bf16 build.
// Quantised rows (kv8, kv4, kv6, kv84): the code planes stand where the 16-bit rows were (bank->k / bank->v are not read; a missing plane is an
// argument error before anything else of the call is read), and the plan is that of the 16-bit step of the same shape (the scorers
// read logits and partials, never a K/V element, so splits, launches and workspace carry over), run on that format's instances of the
// two decode attention kernels — which is all a quantised bank has: decode steps, plain keys, and the shapes of kRowsRules.
// kv164 keeps its keys in the bank's 16-bit K rows: the call reads bank->k (NULL is an argument error like a missing plane) and only
// bank->v is replaced by a plane.
// A batched decode step (include/easykv_hip.h, ekv_seq): the plan of the uniform step of the batch's ENVELOPE — the longest entry, the
// widest extent, one "layer" per entry: same splits, launches and workspace pitches, so a uniform table plans field for field as the
// multi-layer step it spells out.  The entries keep their own bounds inside those pitches (the kernels' batch instances read them
// from the table, whose entries have phys_extent resolved as ekv_plan_step resolves a step's).
// The two axes apply independently: the table of a quantised batch is checked against the bank the code planes stand in, and the
// refusals of either axis hold unchanged (a head_dim the row format does not take, in a table: EKV_E_UNSUPPORTED with zero launches
// and zero bytes).  The plan is the 16-bit batched call's of the same table.
// the struct of a window call: complete, and nothing negative in what the host can read (windows_host: optional, bank->n_layers entries)
static bool ekv_win_ok(const ekv_win* w, const ekv_bank* bank) {
  if (!w || !w->tok_pos || !w->windows || w->q_pos0 < 0) return false;
  if (w->windows_host && check_bank(bank) != EKV_E_ARG)      // (n_layers is read only from a bank whose fields have been checked: a bad bank is reported as such by the call)
    for (int i = 0; i < bank->n_layers; ++i)
      if (w->windows_host[i] < 0) return false;
  return true;
}

// the struct of an adaptive call: complete, the pooling words valid (radius 0 = no pooling), the bounds in order around the step's n_evict
// and inside its candidate range (only the step's own integers are read)
static bool ekv_ada_ok(const ekv_ada* a, const ekv_step* st) {
  if (!a || !a->n_evict_out || a->radius < 0 || (a->op != EKV_POOL_MAX && a->op != EKV_POOL_AVG)) return false;
  if (!st) return true;      // (the call reports the missing step itself)
  const i64 C = (i64)st->n_slots - st->score_off - st->win_lo - st->win_tail;
  return a->evict_min >= 0 && a->evict_min <= st->n_evict && st->n_evict >= 1 && st->n_evict <= a->evict_max && a->evict_max <= C;
}

// Adaptive calls: the three-kernel ending and its scratch, BEHIND everything the pooled layout holds (every other offset is the pooled
// call's): the ranking keys, one row of t_pad words per (layer, head), then the class bytes, one row of t_pad bytes; a deferred call's
// slices as in plan_checks
static void plan_ada_layout(const ekv_bank* bank, const ekv_step* st, EkvStepPlan* P) {
  for (int i = 0; i < P->n_list; ++i)
    if (P->list[i].kind == EKV_RUN_SCORE_SELECT) P->list[i].kernel_count += 2, P->n_launches += 2;
  const size_t LC = (size_t)(st->defer_layers > 0 ? st->defer_layers : st->layer_count), H = (size_t)bank->n_kv_heads;
  const size_t li = st->defer_layers != 0 ? (size_t)st->defer_index : 0;
  size_t off = P->bytes;
  P->ada_keys = (int64_t)(off + li * H * P->t_pad * 4);
  off += ekv_align(LC * H * P->t_pad * 4, 256);
  P->ada_cls = (int64_t)(off + li * H * P->t_pad);
  off += ekv_align(LC * H * P->t_pad, 256);
  P->bytes = off;
}

// The envelope of a heads call (include/easykv_hip.h, ekv_heads): the largest and the smallest T = rows_host[l][h] + grow + 1 over the
// layers the call's pitches must serve — its own, or all deferred ones.  Reads the host copy alone.  EKV_E_ARG for anything the table
// cannot be read with (a bank or layers out of range) or holds out of range.
static int ekv_heads_envelope(const ekv_bank* bank, const ekv_step* st, const ekv_heads* hd, int32_t* t_max, int32_t* t_min) {
  if (!hd || !hd->rows || !hd->rows_host || hd->grow < 0 || !bank || !st) return EKV_E_ARG;
  if (bank->n_layers <= 0 || bank->n_kv_heads <= 0 || bank->cap <= 0) return EKV_E_ARG;
  i64 l0 = st->layer_begin, lc = st->layer_count;
  if (st->defer_layers > 0) l0 = (i64)st->layer_begin - st->defer_index, lc = st->defer_layers;
  if (l0 < 0 || lc < 1 || l0 + lc > bank->n_layers) return EKV_E_ARG;
  i64 hi = 0, lo = (i64)1 << 40;
  for (i64 i = l0 * bank->n_kv_heads; i < (l0 + lc) * bank->n_kv_heads; ++i) {
    const i64 rows = hd->rows_host[i];
    if (rows < 1) return EKV_E_ARG;
    hi = std::max(hi, rows), lo = std::min(lo, rows);
  }
  if (hi + hd->grow + 1 > bank->cap) return EKV_E_ARG;
  *t_max = (int32_t)(hi + hd->grow + 1), *t_min = (int32_t)(lo + hd->grow + 1);
  return EKV_OK;
}

int resolve_call(const EkvCall& c, EkvResolved* r) {
  EkvStepPlan* P = &r->plan;
  *P = EkvStepPlan{};
  const bool quant = c.rows != EKV_ROWS_kv16;
  r->bank = quant ? nullptr : c.bank;
  r->step = c.step;
  r->tb = nullptr;
  if (c.dtype != EKV_DTYPE_F16 && c.dtype != EKV_DTYPE_BF16) return EKV_E_ARG;
  if (quant) {
    const bool own_k = c.rows == EKV_ROWS_kv164;      // (the keys are the bank's own rows)
    if (!c.bank || !ekv_planes_complete(c.rows, c.planes) || (own_k && !c.bank->k)) return EKV_E_ARG;
    r->bank_q = *c.bank;
    r->bank_q.k = own_k ? c.bank->k : c.planes.k_codes;
    r->bank_q.v = c.planes.v_codes;
    r->bank = &r->bank_q;
  }
  const ekv_bank* bank = r->bank;
  if (c.batch) {
    const ekv_seq* seqs = c.seqs;
    if (!bank || !c.step || !seqs || c.n_seq < 1 || c.n_seq > EKV_MAX_SEQS) return EKV_E_ARG;
    ekv_step* env = &r->env;
    *env = *c.step;
    env->layer_begin = 0;
    env->layer_count = c.n_seq;
    env->n_slots = env->n_evict = env->phys_extent = 0;
    env->score_off = seqs[0].score_off;
    for (int i = 0; i < c.n_seq; ++i) {
      const ekv_seq& e = seqs[i];
      ekv_seq& t = r->table.e[i];
      t = e;
      t.phys_extent = (e.phys_extent >= e.n_slots && e.phys_extent <= bank->cap) ? e.phys_extent : bank->cap;
      env->n_slots = std::max(env->n_slots, e.n_slots);
      env->n_evict = std::max(env->n_evict, e.n_evict);
      env->phys_extent = std::max(env->phys_extent, t.phys_extent);
      env->score_off = std::min(env->score_off, e.score_off);
    }
    // (selection windows are bounds, not pitches: the envelope carries the widest candidate set an entry's checks can leave)
    env->win_lo = env->win_tail = env->range_start = 0;
    env->roco_k1 = env->n_evict;
    // the table first: an entry the single-sequence step would refuse as an argument error is one here, whatever the envelope says
    for (int i = 0; i < c.n_seq; ++i) {
      const ekv_seq& e = seqs[i];
      if (e.layer < 0 || e.layer >= bank->n_layers || e.n_slots < 1 || e.n_slots > bank->cap) return EKV_E_ARG;
      for (int j = 0; j < i; ++j)
        if (seqs[j].layer == e.layer) return EKV_E_ARG;
    }
    r->step = env;
    r->tb = &r->table;
  }

  // (a long call is a 16-bit, single-sequence call: its entry points spell nothing else, and no other combination has an instance)
  // Capped calls (ekv_cap_*), the rule of the family stated once.  "Capped" is one more independent variant of a call; its entry points
  // spell 16-bit rows and one sequence only, and no other combination has an instance.  The cap must be finite and > 0 (argument error,
  // behind the element type, before anything is planned).  A decode step plans field for field as the uncapped call of the same (bank,
  // step, dtype) — splits, launches, workspace, phase order and resident rows — and runs the `cap` decode instances.  A chunk step or
  // dense prefix plans onto the 16x16x32 kernel alone, in its one-tile build, at head_dim 128 as head_dim 256 always does (blocks of at
  // most 32 folded rows; one pass or statistics + exact pass by the existing rules): never the wide, the logits-in-LDS or the
  // logits-resident kernel.  Refused with zero launches and zero bytes: RoPE-on-read, head_dim 32 / 64 / 96, a chunk step whose GQA
  // factor exceeds a block (EKV_E_UNSUPPORTED).
  if (c.capped && !(c.softcap > 0.f && c.softcap <= 3.0e38f)) return EKV_E_ARG;
  // Sink calls (ekv_sink_*), likewise stated once.  "Sink" is one more independent variant of a call; its entry points spell 16-bit rows,
  // one sequence and uncapped logits only, and no other combination has an instance.  NULL sinks are an argument error, behind the element
  // type and before anything is planned; the pointer is never dereferenced here.  A decode step plans as the plain call of the same (bank,
  // step, dtype) — splits, launches, workspace — and runs the sink decode instances, in which the phase order K and the resident rows are
  // compiled out (as in the kv164 ones): the plan says order F and no resident rows (info [9] = 0, ekv_step_resident_rows' rule gives 0).
  // A chunk step or dense prefix plans by the capped call's rule: the 16x16x32 kernel alone, one-tile build, blocks of at most 32 folded
  // rows, one pass (the scorer as its tail where the step is one unsplit block) or statistics + exact pass + generic scorer.  Refused with
  // zero launches and zero bytes (EKV_E_UNSUPPORTED): RoPE-on-read, a head_dim other than 64 / 128, a chunk step whose GQA factor
  // exceeds a block.  The head-mean TOVA row (tova_head_mean) runs the sink build of its kernel.
  if (c.sink && c.sinks == nullptr) return EKV_E_ARG;
  // Window calls (ekv_win_*), likewise stated once.  "Window" is one more independent variant of a call, allowed together with "sink"
  // (win->s_aux != NULL) and with nothing else.  A NULL struct, NULL tok_pos / windows, a negative q_pos0 and a negative entry of the
  // host copy of the windows are argument errors, behind the element type and before anything is planned; no device pointer is
  // dereferenced here.  A decode step plans as the SINK call of the same (bank, step, dtype) — order F, no resident rows, the same
  // splits, launches and workspace — with or without sinks, and runs the window decode instances; the token position of the appended
  // row is stamped at the kernels' append site, so the plan has no launch of its own for it.  A chunk step or dense prefix plans by the
  // sink call's rule (the 16x16x32 kernel alone, blocks of at most 32 folded rows, wide = 0).  Refused with zero launches and zero bytes
  // (EKV_E_UNSUPPORTED): RoPE-on-read, a head_dim other than 128 (window alone) / 64 (with sinks), and what the sink call refuses (a chunk
  // step whose GQA factor exceeds a block).  The head-mean TOVA row (tova_head_mean) is rebuilt from the exported logits, whose masked
  // columns are -inf (exp -> 0), by the plain build of its kernel, or by the sink build where the call has sinks.
  if (c.window && !ekv_win_ok(c.win, bank)) return EKV_E_ARG;
  // Pooled calls (ekv_pool_*), likewise stated once.  "Pooled" is one more independent variant of a call, combined with nothing else: its
  // entry points spell 16-bit rows and one sequence, and there is no pooled long, capped, sink or window call.  A NULL struct, a radius
  // < 1 and an unknown op are argument errors, behind the element type and before anything is planned.  The ONE rule: a pooled step plans
  // as the plain call of the same (bank, step, dtype) with every in-kernel scorer tail switched off — no one-launch decode step, no
  // fast scorer behind the split kernel, no logits-in-LDS kernel, no scorer as the tail of the 16x16 one-pass kernel or of the wide
  // column-sum pass, no logits-resident kernel — so that wherever the step scores it ends in EKV_RUN_SCORE_SELECT (whole steps, phases
  // & 2, phases & 8, the deferred flush over all layers), which call_attend runs on the EKV_POOL instances of the generic scorer.  The
  // tiling, the scheme (two passes, or one pass with exported logits), the workspace layout and the width bound are the plain call's
  // rules: the stencil reads the score row where it sits and writes the key row, so the pooled LDS plan is the unpooled one and the widest
  // pooled row is the generic scorer's (ekv_geometry.h).  Refused with zero launches and zero bytes (EKV_E_UNSUPPORTED): a policy other
  // than h2o_head / tova (roco's two-stage rule has no single row to pool; EKV_POLICY_RANGE and EKV_POLICY_NONE have no row at all),
  // RoPE-on-read, tova_head_mean, slot-indexed score rows, a row beyond the generic scorer's width.
  if (c.pooled && !(c.pool != nullptr && c.pool->radius >= 1 && (c.pool->op == EKV_POOL_MAX || c.pool->op == EKV_POOL_AVG))) return EKV_E_ARG;
  // Adaptive calls (ekv_ada_*; include/easykv_hip.h, "adaptive head budgets"), likewise stated once.  "Adaptive" is one more independent
  // variant of a call, combined with nothing else.  A NULL struct, NULL n_evict_out, a radius < 0, an unknown op and bounds out of order
  // (ekv_ada_ok: 0 <= evict_min <= n_evict <= evict_max <= the candidates of the step, n_evict >= 1) are argument errors, behind the
  // element type and before anything is planned.  The ONE rule: an adaptive step plans as the POOLED call of the same (bank, step, dtype)
  // — field for field, refusals included — and where that plan ends in EKV_RUN_SCORE_SELECT the entry counts three kernels (rank, allot,
  // select: call_attend) and the workspace grows, behind everything the pooled layout holds, by the exported ranking keys and class
  // bytes (plan_ada_layout).  Refused on top of the pooled refusals (EKV_E_UNSUPPORTED, zero launches, zero bytes): more than 64 KV heads
  // (the allot kernel keeps one counter pair per head in LDS).
  if (c.adaptive && !ekv_ada_ok(c.ada, c.step)) return EKV_E_ARG;
  // Heads calls (ekv_heads_*; include/easykv_hip.h, "heads"), likewise stated once.  "Heads" is one more independent variant of a call,
  // combined with nothing else.  A NULL struct or pointer, grow < 0, a host count < 1, a resulting T > cap and layers the table cannot be
  // read for are argument errors, behind the element type and before anything is planned; only the HOST copy of the table is read.  The
  // ONE rule: a heads call plans as the plain call of its ENVELOPE — the caller's step with n_slots = the largest T of the host table
  // over the call's layers, or over all deferred layers, so that the layer calls and the flush agree on every pitch — field for field,
  // run on instances without the phase order K; the whole-step form plans as phases = 1 | 2 of that step, because the family has no
  // one-launch build.  EKV_RUN_DECODE and EKV_RUN_DECODE_SCORE run the EKV_HEADS instances; the fold launch is the uniform one (it reads
  // no per-step field).  Refused with zero launches and zero bytes (EKV_E_UNSUPPORTED): q_len > 1, RoPE-on-read, slot-indexed score rows,
  // tova_head_mean, more than one victim, a GQA factor > 8, and a plan with any other launch (the generic scorer, the range compaction).
  int32_t heads_t_min = 0;
  if (c.heads) {
    int32_t t_max = 0;
    if (int e = ekv_heads_envelope(bank, c.step, c.hd, &t_max, &heads_t_min)) return e;
    r->env = *c.step;
    r->env.n_slots = t_max;
    if ((r->env.phases & ~(EKV_PHASE_SLOT_ROWS | EKV_PHASE_SLOT_TAIL_OK)) == 0) r->env.phases |= 1 | 2;
    r->step = &r->env;
  }
  const int variants = (c.long_rows ? 1 : 0) + (c.capped ? 1 : 0) + (c.sink || c.window ? 1 : 0) + (c.pooled ? 1 : 0) + (c.adaptive ? 1 : 0) + (c.heads ? 1 : 0);
  const bool sinkish = c.sink || c.window;
  const int rc = (variants && (quant || c.batch || variants > 1))
                     ? EKV_E_UNSUPPORTED
                     : ekv_plan_step(bank, r->step, P, c.long_rows, c.capped || sinkish, quant || c.batch || sinkish || c.capped || c.heads, c.pooled || c.adaptive);
  P->heads = c.heads ? 1 : 0;
  P->capped = c.capped ? 1 : 0;
  P->sink = c.sink ? 1 : 0;
  P->window = c.window ? 1 : 0;
  P->pooled = c.pooled ? 1 : 0;
  P->adaptive = c.adaptive ? 1 : 0;
  P->ada_keys = P->ada_cls = -1;
  P->bf16 = c.dtype == EKV_DTYPE_BF16;
  P->rows = c.rows;
  P->batch = c.batch;
  if (quant || c.batch || sinkish) P->fused_order = 0;      // (the quantised, the batch and the sink instances keep order F, without resident rows)
  if (c.capped && P->fused_nw == 8) P->fused_order &= ~0xFFFF;      // (the soft-capped 8-wave instances keep order F; their resident rows stay)
  auto refuse = [&](int code) {
    if (P->long_rows) {      // (a long plan that is refused after all reports the layout of the plain call: nothing of the long scorer remains)
      EkvStepPlan plain;
      (void)ekv_plan_step(bank, r->step, &plain);
      P->bytes = plain.bytes, P->big_rows = plain.big_rows, P->key_rows = -1;
    }
    P->one_launch = P->n_launches = P->n_list = P->long_rows = P->long_tiles = 0;
    if (c.batch || c.capped || sinkish || c.pooled || c.adaptive || c.heads) P->bytes = 0;      // (nothing will run: ekv_batch_workspace_bytes of a refused table, ekv_cap_ / ekv_sink_ / ekv_pool_workspace_bytes of a refused step, is 0)
    return code;
  };
  const ekv_step* st = c.step;
  if (c.batch) {
    if (int e = check_bank(bank)) return refuse(e);
    // the forms a batch does not take, whatever else the step says: chunk steps, RoPE-on-read, phased / deferred / slot-indexed steps
    if (st->q_len != 1 || st->rope_on_read || st->phases != 0 || st->defer_layers != 0 || st->tova_head_mean) return refuse(EKV_E_UNSUPPORTED);
  }
  if (rc == EKV_OK && P->bf16 && st->rope_on_read) return refuse(EKV_E_UNSUPPORTED);
  if (rc != EKV_OK) return refuse(rc);
  if (c.capped && (st->rope_on_read || (bank->head_dim != 128 && bank->head_dim != kChunkNarrowD))) return refuse(EKV_E_UNSUPPORTED);
  if (c.sink && (st->rope_on_read || (bank->head_dim != 64 && bank->head_dim != 128))) return refuse(EKV_E_UNSUPPORTED);
  if (c.window && (st->rope_on_read || bank->head_dim != (c.sink ? 64 : 128))) return refuse(EKV_E_UNSUPPORTED);
  if ((c.pooled || c.adaptive) && (st->rope_on_read || st->tova_head_mean || (st->policy != EKV_POLICY_H2O_HEAD && st->policy != EKV_POLICY_TOVA)))
    return refuse(EKV_E_UNSUPPORTED);
  if (c.adaptive) {
    if (bank->n_kv_heads > 64) return refuse(EKV_E_UNSUPPORTED);
    plan_ada_layout(bank, st, P);
  }
  if (c.heads) {
    const int rep = bank->n_q_heads / bank->n_kv_heads;
    if (st->q_len != 1 || st->rope_on_read || (st->phases & EKV_PHASE_SLOT_ROWS) || st->tova_head_mean || st->n_evict > 1 || rep > 8) return refuse(EKV_E_UNSUPPORTED);
    // the shortest head: every argument check of the uniform step that reads T is monotone in it (T < q_len, n_evict >= T, score_off >= T,
    // a candidate range narrower than n_evict), and the envelope has passed them for the longest
    ekv_step one = *r->step;
    one.n_slots = heads_t_min, one.n_split = P->n_split;
    EkvStepPlan P1;
    if (ekv_plan_step(bank, &one, &P1) == EKV_E_ARG) return refuse(EKV_E_ARG);
    for (int i = 0; i < P->n_list; ++i) {
      const int kind = P->list[i].kind;
      if (kind != EKV_RUN_DECODE && kind != EKV_RUN_FOLD && kind != EKV_RUN_DECODE_SCORE) return refuse(EKV_E_UNSUPPORTED);
    }
  }
  if (quant && (st->q_len != 1 || st->rope_on_read || !ekv_rows_head_dim(c.rows, bank->head_dim) ||
                bank->n_q_heads / bank->n_kv_heads > kRowsRules[c.rows].max_rep))
    return refuse(EKV_E_UNSUPPORTED);
  if (c.batch) {
    for (int i = 0; i < c.n_seq; ++i) {      // per entry: the checks of the single-sequence step of that entry's geometry
      const ekv_seq& e = c.seqs[i];
      ekv_step one = *st;
      one.layer_begin = e.layer, one.layer_count = 1, one.n_split = P->n_split;
      one.n_slots = e.n_slots, one.score_off = e.score_off, one.n_evict = e.n_evict, one.win_lo = e.win_lo, one.win_tail = e.win_tail;
      one.roco_k1 = e.roco_k1, one.range_start = e.range_start, one.phys_extent = e.phys_extent;
      EkvStepPlan P1;
      if (ekv_plan_step(bank, &one, &P1) == EKV_E_ARG) return refuse(EKV_E_ARG);
    }
    // the kernels with a batch instance: the one-launch step, the split attention kernel (+ fold) and the fast scorer behind it, the
    // range compaction.  What is left to the generic scorer (GQA factors > 8, rows beyond 6144 slots, cap % 4 != 0) has none.
    for (int i = 0; i < P->n_list; ++i) {
      const int kind = P->list[i].kind;
      if (kind != EKV_RUN_FUSED_DECODE && kind != EKV_RUN_DECODE && kind != EKV_RUN_FOLD && kind != EKV_RUN_RANGE && kind != EKV_RUN_DECODE_SCORE)
        return refuse(EKV_E_UNSUPPORTED);
    }
  }
  return EKV_OK;
}

int call_check(const EkvCall& c) {
  EkvResolved r;
  return resolve_call(c, &r);
}

size_t call_workspace_bytes(const EkvCall& c) {
  EkvResolved r;
  (void)resolve_call(c, &r);
  return r.plan.bytes;      // (a batch: the table travels in the kernel arguments, nothing is staged)
}

int call_info(const EkvCall& c, int32_t* info, int32_t n_info) {
  EkvResolved r;
  const bool ok = resolve_call(c, &r) == EKV_OK;
  if (c.dtype != EKV_DTYPE_F16 && c.dtype != EKV_DTYPE_BF16) return EKV_E_ARG;
  if (c.capped && !(c.softcap > 0.f && c.softcap <= 3.0e38f)) return EKV_E_ARG;      // (a cap no step can be planned with)
  if (c.sink && c.sinks == nullptr) return EKV_E_ARG;
  if (c.window && !ekv_win_ok(c.win, r.bank)) return EKV_E_ARG;
  if (c.pooled && !(c.pool != nullptr && c.pool->radius >= 1 && (c.pool->op == EKV_POOL_MAX || c.pool->op == EKV_POOL_AVG))) return EKV_E_ARG;
  if (c.adaptive && !ekv_ada_ok(c.ada, c.step)) return EKV_E_ARG;
  if (c.heads) {
    int32_t t_max, t_min;
    if (int e = ekv_heads_envelope(r.bank, c.step, c.hd, &t_max, &t_min)) return e;
  }
  if (c.rows != EKV_ROWS_kv16 && !r.bank) return EKV_E_ARG;
  if (int e = check_bank(r.bank)) return e;
  if (!c.step || (c.batch && !c.seqs) || !info || n_info < 1) return EKV_E_ARG;
  const EkvStepPlan& P = r.plan;
  const int32_t v[EKV_STEP_INFO_N] = {P.n_split, ok ? P.one_launch : 0, P.two_pass, P.wide, P.n_qblocks, P.qb_rows, P.n_col_parts,
                                      P.fold_in_kernel, ok ? P.n_launches : 0, ok ? (P.fused_order & 3) : 0};
  for (int i = 0; i < n_info && i < EKV_STEP_INFO_N; ++i) info[i] = v[i];
  for (int i = EKV_STEP_INFO_N; i < n_info; ++i) info[i] = 0;
  if (c.long_rows) {      // ekv_long_step_info: does the step end in the long-row scorer, and the column tiles per head of its sweep
    if (n_info > 10) info[10] = ok ? P.long_rows : 0;
    if (n_info > 11) info[11] = ok ? P.long_tiles : 0;
  }
  return EKV_OK;
}

int call_resident_rows(const EkvCall& c) {
  EkvResolved r;
  const bool ok = resolve_call(c, &r) == EKV_OK;
  if (c.dtype != EKV_DTYPE_F16 && c.dtype != EKV_DTYPE_BF16) return EKV_E_ARG;
  if (c.rows != EKV_ROWS_kv16 && !r.bank) return EKV_E_ARG;
  if (int e = check_bank(r.bank)) return e;
  if (!c.step || (c.batch && !c.seqs)) return EKV_E_ARG;
  return ok && r.plan.one_launch ? EKV_RESIDENT_ROWS(r.plan.fused_order) : 0;
}

int call_plan(const ekv_bank* bank, const ekv_step* st, int32_t* n_split, int32_t* fused) {
  if (int e = check_bank(bank)) return e;
  if (!st || !n_split || !fused) return EKV_E_ARG;
  EkvResolved r;
  const int rc = resolve_call(step_call(bank, st, EKV_DTYPE_F16), &r);
  *n_split = r.plan.n_split;
  // one launch for the whole step: the fused decode kernel, the logits-in-LDS or logits-resident chunk kernel, or a chunk step whose
  // scorer runs as the tail of the attention kernel; a step the call would refuse plans as 0
  *fused = rc == EKV_OK ? r.plan.one_launch : 0;
  return EKV_OK;
}
