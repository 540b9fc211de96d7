// press_out_dev.h -- device side of press_out.h: how rows_kernel (press_rows.hip) and reemit_kernel (press_reemit.hip)
// put a cost and a tile's headers into a profile's canonical rows and its cost-order copy.  Both run 256 threads over
// tiles of 64 positions x 64 codes; the tile loops are their own.
#pragma once
#include "dcp_types.h"
#include "press_out.h"

#include <hip/hip_runtime.h>

namespace dcp_out
{

constexpr int TILE = 64;
constexpr int THREADS = 256;
static_assert(THREADS == TILE * DCP_ROW_HDR, "one thread per header float of a tile");

// the sign flip is exact (the sign bit: -inf becomes +inf, 0 becomes -0 as on the host)
__device__ inline float flip(float v) { return __uint_as_float(__float_as_uint(v) ^ 0x80000000u); }

// the column of position k in the cost-order copy (0 where k lies beyond it: no value goes there)
__device__ inline int copy_col(DcpRowsOut const &o, int k) { return k < TILE * o.cQ ? dcp_cost_order_col(o.cQ, 1, k) : 0; }

// cost v of code c at position k, col = copy_col(o, k): into the canonical row (+inf beyond K comes as v; 0 in the
// match columns of a poisoned profile) and into the cost-order copy
__device__ inline void store(float *pool, DcpRowsOut const &o, int c, int k, int col, float v)
{
  int const copy_cols = TILE * o.cQ, copy_stride = DCP_COST_ORDER_HDR + copy_cols;
  pool[o.rows_off + (int64_t)c * o.stride + DCP_ROW_HDR + k] = o.poison && k < o.K ? 0.0f : v;
  if (k < copy_cols) pool[o.copy_off + (int64_t)c * copy_stride + DCP_COST_ORDER_HDR + col] = v;
}

// the {null, bg, 0, 0} headers of codes [c0, c0 + TILE) in both layouts, from the log-probabilities null[1364] and
// bg[1364]; the copy's header is padded with +inf to DCP_COST_ORDER_HDR floats.  For the whole workgroup.
__device__ inline void headers(float *pool, DcpRowsOut const &o, int c0, int tid, float const *null, float const *bg)
{
  float const inf = __uint_as_float(0x7f800000u);
  int const copy_stride = DCP_COST_ORDER_HDR + TILE * o.cQ;
  {
    int const c = c0 + tid / DCP_ROW_HDR, j = tid % DCP_ROW_HDR; // THREADS = TILE * DCP_ROW_HDR
    if (c < DCP_TABLE_SIZE)
      pool[o.rows_off + (int64_t)c * o.stride + j] = j == 0 ? flip(null[c]) : j == 1 ? flip(bg[c]) : 0.0f;
  }
  if (o.cQ)
    for (int i = tid; i < TILE * DCP_COST_ORDER_HDR; i += THREADS)
    {
      int const c = c0 + i / DCP_COST_ORDER_HDR, j = i % DCP_COST_ORDER_HDR;
      if (c < DCP_TABLE_SIZE)
        pool[o.copy_off + (int64_t)c * copy_stride + j] =
            j == 0 ? flip(null[c]) : j == 1 ? flip(bg[c]) : j < DCP_ROW_HDR ? 0.0f : inf;
    }
}

} // namespace dcp_out
