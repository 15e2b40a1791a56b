// split-path decode scorer and fold (ekv_decode_score.inc), fp16 outputs
#include "ekv_decode_score.inc"
