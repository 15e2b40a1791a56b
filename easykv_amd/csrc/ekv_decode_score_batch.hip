// scorer of the split path of a batched decode step (ekv_decode_score.inc, EKV_BATCH), fp16 outputs
#define EKV_BATCH 1
#include "ekv_decode_score.inc"
