// press_out.h -- where the kernels that make a profile's emission rows on the device (press_rows.hip, press_reemit.hip)
// write them: the part of their descriptors that the two share, and on the device (press_out_dev.h) the code that
// stores a value and the rows' headers through it.
#pragma once
#include <stdint.h>

// One profile.  Offsets are floats into the pool; what `src` counts is the kernel's own (DcpRowsDesc, DcpReemitDesc).
struct DcpRowsOut
{
  int64_t src;      // entry of node 0 among the kernel's inputs
  int64_t rows_off; // rows[1364][stride]
  int64_t copy_off; // cost-order copy [1364][DCP_COST_ORDER_HDR + 64 cQ]; unused when cQ == 0
  int32_t K, Kp;
  int32_t stride; // DCP_ROW_HDR + Kp
  int32_t cQ;     // positions per lane of the cost kernel the copy is for (W' = 1), 0: no copy
  int32_t poison; // DECIPHON_HIP_COST_ORDER=poison: the canonical match columns of a copied profile are 0
};
