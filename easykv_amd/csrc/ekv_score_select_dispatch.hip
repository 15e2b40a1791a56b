// Block-size dispatch of the generic scorer: 256-thread workgroups when the grid alone fills the chip (more workgroups
// resident per CU, cheaper barriers), 512 threads when there are few (head, layer) pairs.
#include <cstdlib>
#include "ekv_common.h"
#include "ekv_kernels.h"

// ---- the instances (ekv_instances.def).  The head-mean row does not depend on the element type: the f16 instance of a block size
// exports it.  (LDS bytes of a block size: ekv_score_lds_bytes, ekv_geometry.h)
typedef hipError_t EkvSelectFn(const EkvScoreArgs&, int layer_count, hipStream_t);
#define EKV_SCORE_SELECT(nt, elem) EkvSelectFn EKV_FN_SCORE_SELECT(nt, elem), ekv_launch_tova_headmean_nt##nt;
#include "ekv_instances.def"

namespace {
struct SelectInstance {
  int threads;
  bool bf16;
  EkvSelectFn* fn;
};
const SelectInstance kSelect[] = {
#define EKV_SCORE_SELECT(nt, elem) {nt, EKV_IS_##elem, EKV_FN_SCORE_SELECT(nt, elem)},
#include "ekv_instances.def"
};
hipError_t launch_select(int threads, const EkvScoreArgs& a, int layer_count, hipStream_t s, bool bf16) {
  for (const SelectInstance& in : kSelect)
    if (in.threads == threads && in.bf16 == bf16) return in.fn(a, layer_count, s);
  return hipErrorInvalidValue;
}
}  // namespace

hipError_t ekv_launch_score_select(const EkvScoreArgs& a, int layer_count, hipStream_t s, bool bf16) {
  // (the bf16 instances differ only in how the folded output is rounded and stored)
  auto nt256 = [&](const EkvScoreArgs& x, int lc, hipStream_t st) { return launch_select(256, x, lc, st, bf16); };
  auto nt512 = [&](const EkvScoreArgs& x, int lc, hipStream_t st) { return launch_select(512, x, lc, st, bf16); };
  auto nt1024 = [&](const EkvScoreArgs& x, int lc, hipStream_t st) { return launch_select(1024, x, lc, st, bf16); };
  // 256 threads only while at least three such workgroups fit a CU's LDS; wide score rows (C4: W = 5098 -> 82 KB) leave
  // room for one workgroup per CU, which must then bring 512 threads
  if (a.big_rows != nullptr) return nt1024(a, layer_count, s);   // rows in global scratch, keys in LDS
  static const int force = [] { const char* e = std::getenv("EKV_SS_NT"); return e ? std::atoi(e) : 0; }();   // (A/B knob: 256 / 512 / 1024)
  if (force == 256 && ekv_score_lds_bytes(256, a) <= 160 * 1024) return nt256(a, layer_count, s);
  if (force == 512 && ekv_score_lds_bytes(512, a) <= 160 * 1024) return nt512(a, layer_count, s);
  if (force == 1024 && ekv_score_lds_bytes(1024, a) <= 160 * 1024) return nt1024(a, layer_count, s);
  // (the rule itself is ekv_score_select_threads, ekv_geometry.h: the long-row scorer asks it which build the plain call would run)
  // 256 threads where the grid alone fills the chip and three workgroups fit a CU's LDS.
  // one workgroup per CU either way (at most one (head, layer) pair per CU, or LDS rows too wide for two): give it all 16
  // wave slots — the logits sweep is VALU-bound on exact expf / IEEE div and 2 waves per SIMD do not fill the pipeline
  const bool scored = a.policy == EKV_POLICY_H2O_HEAD || a.policy == EKV_POLICY_ROCO || a.policy == EKV_POLICY_TOVA;
  const int64_t W = (int64_t)a.n_slots - (scored ? a.score_off : 0);
  const int64_t rows = a.colsum != nullptr ? 0 : (int64_t)(a.n_q_heads / a.n_kv_heads) * a.q_len;
  switch (ekv_score_select_threads((int64_t)a.n_kv_heads * layer_count, W, rows, false)) {
    case 256: return nt256(a, layer_count, s);
    case 1024: return nt1024(a, layer_count, s);
    default: return nt512(a, layer_count, s);
  }
}

// ---- the pooled instances (ekv_instances_later.def, EKV_SCORE_SELECT_POOL): 512 threads, or 1024 wherever the unpooled rule above
// picks them (rows in scratch; one workgroup per CU).  Where that rule picks 256 threads the pooled call runs 512.
typedef hipError_t EkvSelectPoolFn(const EkvScoreArgs&, const EkvPoolArgs&, int layer_count, hipStream_t);
#define EKV_SCORE_SELECT_POOL(nt, elem) EkvSelectPoolFn EKV_FN_SCORE_SELECT_POOL(nt, elem);
#include "ekv_instances.def"

namespace {
struct SelectPoolInstance {
  int threads;
  bool bf16;
  EkvSelectPoolFn* fn;
};
const SelectPoolInstance kSelectPool[] = {
#define EKV_SCORE_SELECT_POOL(nt, elem) {nt, EKV_IS_##elem, EKV_FN_SCORE_SELECT_POOL(nt, elem)},
#include "ekv_instances.def"
};
}  // namespace

hipError_t ekv_launch_score_select_pool(const EkvScoreArgs& a, const EkvPoolArgs& pool, int layer_count, hipStream_t s, bool bf16) {
  const int64_t W = (int64_t)a.n_slots - a.score_off;      // (a pooled step is scored: h2o_head / tova)
  const int64_t rows = a.colsum != nullptr ? 0 : (int64_t)(a.n_q_heads / a.n_kv_heads) * a.q_len;
  const int threads = ekv_score_pool_threads((int64_t)a.n_kv_heads * layer_count, W, rows, a.big_rows != nullptr);
  for (const SelectPoolInstance& in : kSelectPool)
    if (in.threads == threads && in.bf16 == bf16) return in.fn(a, pool, layer_count, s);
  return hipErrorInvalidValue;
}

// ---- the adaptive instances (ekv_instances_later.def, EKV_SCORE_SELECT_ADA): the block size of the pooled rule above, for both phases
typedef hipError_t EkvSelectAdaFn(const EkvScoreArgs&, const EkvAdaArgs&, int layer_count, hipStream_t);
#define EKV_SCORE_SELECT_ADA(nt, elem) EkvSelectAdaFn EKV_FN_SCORE_SELECT_ADA(nt, elem);
#include "ekv_instances.def"

namespace {
struct SelectAdaInstance {
  int threads;
  bool bf16;
  EkvSelectAdaFn* fn;
};
const SelectAdaInstance kSelectAda[] = {
#define EKV_SCORE_SELECT_ADA(nt, elem) {nt, EKV_IS_##elem, EKV_FN_SCORE_SELECT_ADA(nt, elem)},
#include "ekv_instances.def"
};
}  // namespace

hipError_t ekv_launch_score_select_ada(const EkvScoreArgs& a, const EkvAdaArgs& ada, int layer_count, hipStream_t s, bool bf16) {
  const int64_t W = (int64_t)a.n_slots - a.score_off;
  const int64_t rows = a.colsum != nullptr ? 0 : (int64_t)(a.n_q_heads / a.n_kv_heads) * a.q_len;
  const int threads = ekv_score_pool_threads((int64_t)a.n_kv_heads * layer_count, W, rows, a.big_rows != nullptr);
  for (const SelectAdaInstance& in : kSelectAda)
    if (in.threads == threads && in.bf16 == bf16) return in.fn(a, ada, layer_count, s);
  return hipErrorInvalidValue;
}

hipError_t ekv_launch_tova_headmean(const EkvScoreArgs& a, int layer_count, hipStream_t s) {
  return ekv_launch_tova_headmean_nt512(a, layer_count, s);
}
