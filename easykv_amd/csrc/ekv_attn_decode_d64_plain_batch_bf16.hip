// batch instance of ekv_attn_decode.inc (batched decode steps, ekv_seq): head_dim 64, plain keys, bf16
#define EKV_BATCH 1
#define EKV_BF16 1
#define EKV_D 64
#define EKV_ROPE false
#define EKV_ROPE_TAG plain
#include "ekv_attn_decode.inc"
