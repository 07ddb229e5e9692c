// tfg_layout.h -- what the per-cell kernels of different translation units share (tfg_mib.hip, cell_meas.hip): the grid's shape, the
// layout of a work item's cell_scratch, and how the kernels that walk port 0's reference rows split them over a workgroup.
#pragma once
#include "lcs_internal.h"

#define NSC 72
#define ROWS LCS_TFG_ROWS

// cell_scratch layout (doubles, per work item)
#define CS_N_OFDM 0
#define CS_KFACTOR 1
#define CS_OOB 2
#define CS_NRS 8         // 4 values: RS rows per port
#define CS_NPP 640       // [4 ports][CE_NCHUNK <= 8] partial sums of |filtered - raw|^2
#define CS_TF_RES 680    // tfoec: residual_f, k_factor_residual, delay
#define CS_TF_KRES 681
#define CS_TF_TOE 684     // 4 complex partial sums of the timing estimate (k_tfoec_est parts), summed in part order
#define CS_CAND 16       // 12 candidates x 4: ok, bits lo (24 bits as double), unused
#define CS_SHIFT 64      // [140][4] (-1 = no RS)
#define CS_RS 1024       // [140][12] complex
#define CS_SIZE LCS_CELL_SCRATCH

// k_tdd_config, k_cell_meas: 16 lanes (TDD_ROW_LANES, tdd_config.h) per reference row, a thread's rows TC_GROUPS apart
#define TC_THREADS 512
#define TC_GROUPS (TC_THREADS / 16)                         // rows per pass
#define TC_MAX_Q 288                                        // reference rows of 854 symbols with the extended CP: 285
#define TC_PASSES (TC_MAX_Q / TC_GROUPS)
