// logits-resident scored chunk step (ekv_attn_resident.inc), head_dim 128, bf16
#define EKV_BF16 1
#include "ekv_attn_resident.inc"
