// Explicit instantiation of the tied-logits wide GEMM with the logits-free head epilogue (gemm_wr.h
// epilogue_head: per-tile max, sum exp and argmax, no logits store), 384-column tiles.
#define ASRX_WR_INSTANTIATE
#include "gemm_wr.h"

ASRX_WR_INST(3, ROWS, BF16A, Head)
