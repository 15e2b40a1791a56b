// split-path decode scorer and fold (ekv_decode_score.inc), bf16 outputs
#define EKV_BF16 1
#include "ekv_decode_score.inc"
