// FP8-row ("kv8") instance of ekv_attn_decode.inc: head_dim 128, plain keys, fp16 queries / outputs
#define EKV_KV8 1
#define EKV_D 128
#define EKV_ROPE false
#define EKV_ROPE_TAG plain
#include "ekv_attn_decode.inc"
