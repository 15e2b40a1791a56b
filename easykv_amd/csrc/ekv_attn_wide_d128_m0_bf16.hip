// wide-query-block attention kernel (ekv_attn_wide.inc), head_dim 128, mode 0, bf16
#define EKV_BF16 1
#define EKV_D 128
#define EKV_WIDE_MODE 0
#include "ekv_attn_wide.inc"
