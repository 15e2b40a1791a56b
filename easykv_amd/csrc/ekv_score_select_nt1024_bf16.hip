// generic scorer, 1024 threads per workgroup, bf16 outputs
#define EKV_BF16 1
#define EKV_SS_NT 1024
#include "ekv_score_select.inc"
