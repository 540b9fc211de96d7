// press_rows.h -- launch of the kernel that turns the emission tables press_kernel.hip leaves in device memory into a
// profile's tables in the engine's pool (press_rows.hip): what dcp_setup_rows and dcp_cost_order_rows (host_logic.h)
// stage on the host from a pressed file, made where the tables already are.
#pragma once
#include "press_out.h"

#include <hip/hip_runtime_api.h>
#include <stdint.h>

#define DCP_ROWS_TILE 64 // positions and codes per LDS tile

// One profile of a batch.  Offsets are floats into the pool; the emission tables of its nodes are entries
// [out.src, out.src + K) of the emission kernel's output, its transitions trans[8][Kp] and the 16 floats of +inf that
// round the canonical tables up to 128 bytes lie at `trans_src` of the uploaded transition blocks.
struct DcpRowsDesc
{
  DcpRowsOut out;
  int64_t trans_off; // trans[8][Kp], then the padding up to out.copy_off's alignment
  int64_t trans_src; // where the block lies among the uploaded ones, in floats
  int32_t trans_floats; // 8 Kp + padding
};

// For each of the n profiles of `desc` (device memory): rows, cost-order copy and transitions into `pool`, from
// em[entries][1364] (log-probabilities, node-major), null[1364] and bg[1364] (the same) and the transition blocks
// `trans`, all device memory.  max_Kp = the largest Kp among them.  Returns 0, or -1 when the launch failed.
int dcp_press_rows_launch(float const *em, float const *null, float const *bg, float const *trans,
                          DcpRowsDesc const *desc, int n, int max_Kp, float *pool, hipStream_t stream);
