// Explicit instantiations of the two-workgroups-per-CU wide GEMM with the rotary epilogue (the audio side's
// q / k projections, model.py:242-245, 198-214).
#define ASRX_P2_INSTANTIATE
#include "gemm_p2.h"

ASRX_P2_INST(3, BF16A, Rot)
ASRX_P2_INST(3, F32A, Rot)
