// press_reemit.h -- launch of the kernel that writes the emission rows of resident profiles again, at a new error rate,
// from their nodes' distributions in device memory (press_reemit.hip): what the emission kernel and the rows kernel of
// a load (press_kernel.hip, press_rows.hip) write between them, without the node-major tables in between and without
// the transitions, which do not depend on the error rate.
#pragma once
#include "press_out.h"

#include <hip/hip_runtime_api.h>
#include <stdint.h>

#define DCP_REEMIT_TILE 64 // positions and codes per workgroup: DCP_ROWS_TILE, and what dcp_reemit_tiles counts by

// One profile.  Its nodes' inputs are entries [out.src, out.src + K) of the distributions (press_kernel.h:
// DCP_PRESS_IN_STRIDE floats each), and the null and background tables under the new error rate are rows `null_row` and
// `bg_row` of the model tables, 1364 log-probabilities each.
struct DcpReemitDesc
{
  DcpRowsOut out;
  int32_t null_row, bg_row;
};

// For each of the n (profile, k0) pairs -- desc[pair_profile[i]], positions [pair_k0[i], pair_k0[i] + 64), k0 a multiple
// of 64 below the profile's Kp (dcp_reemit_tiles, include/deciphon_host.h) -- the 1364 x 64 emission costs of those
// positions under error rate epsilon into the profile's rows and cost-order copy, and with k0 = 0 the rows' headers.
// Everything but `pool` is read; all of it is device memory.  Returns 0, or -1 when a launch failed.
int dcp_press_reemit_launch(float const *dist, float const *models, DcpReemitDesc const *desc, int32_t const *pair_profile,
                            int32_t const *pair_k0, int64_t n, float epsilon, float *pool, hipStream_t stream);
