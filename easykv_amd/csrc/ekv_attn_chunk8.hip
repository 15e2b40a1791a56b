// Launch code of the chunk step over FP8 code rows (ekv_attn_chunk8.inc; which steps run there: resolve_call, ekv_plan.cpp).
#include "ekv_common.h"
#include "ekv_kernels.h"

// ---- the instances (the EKV_CHUNK_CODES lines of the manifest): launcher declarations, then one table entry per line
typedef hipError_t EkvChunk8Fn(const EkvAttnArgs&, int layer_count, hipStream_t, const EkvScoreArgs*);
#define EKV_CHUNK_CODES(elem, d) EkvChunk8Fn EKV_FN_D_ELEM(ekv_launch_attn_chunk8, d, elem);
#include "ekv_instances.def"

namespace {
struct Chunk8Instance {
  int head_dim;
  bool bf16;
  EkvChunk8Fn* fn;
};
const Chunk8Instance kChunk8[] = {
#define EKV_CHUNK_CODES(elem, d) {d, EKV_IS_##elem, EKV_FN_D_ELEM(ekv_launch_attn_chunk8, d, elem)},
#include "ekv_instances.def"
};
}  // namespace

// fuse_sc != nullptr: an unsplit one-block step whose scorer runs as the tail of the kernel (one launch for the whole step)
hipError_t ekv_launch_attn_chunk8(const EkvAttnArgs& a, int head_dim, int layer_count, hipStream_t s, const EkvScoreArgs* fuse_sc, bool bf16) {
  int qb_rows, n_qblocks, qpw;
  ekv_chunk_blocks(a.n_q_heads / a.n_kv_heads, a.q_len, &qb_rows, &n_qblocks, &qpw, kChunkNarrowD);
  if (qb_rows != a.qb_rows || n_qblocks != a.n_qblocks || (a.n_q_heads / a.n_kv_heads) * qb_rows > kChunkNarrowRows) return hipErrorInvalidValue;
  for (const Chunk8Instance& in : kChunk8)
    if (in.head_dim == head_dim && in.bf16 == bf16) return in.fn(a, layer_count, s, fuse_sc);
  return hipErrorInvalidValue;
}
