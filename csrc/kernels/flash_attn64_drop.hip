// Attention dropout inside the head-dim-64 flash kernels: the DROP instantiations of
// flash_attn64.hip's forward (one query group per wave), dQ and dK / dV kernels, each
// {causal, full} x {plain, lengths}, and their launchers.
//
// The mask is dropout.h's (index ((b H + h) S + q) S + k, a Philox call per 8 consecutive keys of
// one query, S % 8 == 0), regenerated in registers by all three kernels: no keep image in HBM, one
// Philox call per 8 scores, no barrier added. lse stays the undropped log-sum-exp; with
// M = keep / (1 - p_eff): O = (M P) V, dV = (M P)^T dO, dS = P (M dP - D), D = rowsum(dO * O).
// Where the bits come from is described at drop_keep64 / drop_keep_patch in flash_attn64.hip.
//
// This file compiles flash_attn64.hip a second time for those instantiations alone, with the same
// scalar-fp32 flags (_build.py SRC_FLAGS), and leaves the plain kernels' code as it was.
#define CML_F64_DROP_TU 1
#include "flash_attn64.hip"
