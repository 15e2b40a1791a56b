// bf16 instance of ekv_attn_decode.inc: head_dim 64, plain keys (RoPE-on-read has no bf16 build)
#define EKV_BF16 1
#define EKV_D 64
#define EKV_ROPE false
#define EKV_ROPE_TAG plain
#include "ekv_attn_decode.inc"
