// press_rows.h -- launch of the kernel that turns the emission tables press_kernel.hip leaves in device memory into a
// profile's tables in the engine's pool (press_rows.hip): what dcp_setup_rows and dcp_cost_order_rows (host_logic.h)
// stage on the host from a pressed file, made where the tables already are.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#define DCP_ROWS_TILE 64 // positions and codes per LDS tile

// One profile of a batch.  Offsets are floats into the pool; the emission tables of its nodes are entries
// [src, src + K) of the emission kernel's output, its transitions trans[8][Kp] and the 16 floats of +inf that round
// the canonical tables up to 128 bytes lie at `trans_src` of the uploaded transition blocks.
struct DcpRowsDesc
{
  int64_t src;       // entry of node 0
  int64_t rows_off;  // rows[1364][stride]
  int64_t trans_off; // trans[8][Kp], then the padding up to copy_off's alignment
  int64_t trans_src; // where the block lies among the uploaded ones, in floats
  int64_t copy_off;  // cost-order copy [1364][DCP_COST_ORDER_HDR + 64 cQ]; unused when cQ == 0
  int32_t K, Kp;
  int32_t stride;    // DCP_ROW_HDR + Kp
  int32_t trans_floats; // 8 Kp + padding
  int32_t cQ;        // positions per lane of the cost kernel the copy is for (W' = 1), 0: no copy
  int32_t poison;    // DECIPHON_HIP_COST_ORDER=poison: the canonical match columns of a copied profile are 0
};

// For each of the n profiles of `desc` (device memory): rows, cost-order copy and transitions into `pool`, from
// em[entries][1364] (log-probabilities, node-major), null[1364] and bg[1364] (the same) and the transition blocks
// `trans`, all device memory.  max_Kp = the largest Kp among them.  Returns 0, or -1 when the launch failed.
int dcp_press_rows_launch(float const *em, float const *null, float const *bg, float const *trans,
                          DcpRowsDesc const *desc, int n, int max_Kp, float *pool, hipStream_t stream);
