// press_rows.hip -- from the emission tables in device memory to a profile's tables in the pool.
//
// The emission kernel (press_kernel.hip) leaves em[node][1364], log-probabilities, node-major.  The DP kernels read
// code-major rows of costs, rows[1364][DCP_ROW_HDR + Kp] = { -null[c], -bg[c], 0, 0, -em[0..K)[c], +inf .. } (dcp_types.h),
// and for some shapes a second copy of them in cost order.  From a pressed file the host makes both (host_logic.cpp:
// dcp_setup_rows, dcp_cost_order_rows); this kernel makes the same words from the tables where they lie.
//
// It is a transposition: reads are contiguous along the code, writes along the position.  A workgroup takes a tile of
// DCP_ROWS_TILE positions x DCP_ROWS_TILE codes of one profile through LDS (a pitch of 65 floats: the transposed reads
// of a 32-lane half then fall on 32 different banks), so both sides are 256-byte runs per wavefront.  The grid is
// (position tiles up to the largest Kp of the batch, code tiles and one more for the transitions, profile); a profile's
// descriptor (press_rows.h) is uniform over the workgroup.  Tiles beyond K write the +inf padding without reading.
// The sign flip is exact (the sign bit: -inf becomes +inf, 0 becomes -0 as on the host).  How a value and the headers go
// out to the two layouts is shared with the re-emission kernel (press_out_dev.h).
#include "press_rows.h"
#include "dcp_types.h"
#include "press_out_dev.h"

#include <hip/hip_runtime.h>

namespace
{

constexpr int TILE = DCP_ROWS_TILE;
constexpr int PITCH = TILE + 1;
constexpr int THREADS = 256;
constexpr int CODE_TILES = (DCP_TABLE_SIZE + TILE - 1) / TILE; // 22: 21 whole ones and one of 20 codes

using dcp_out::flip;

__global__ __launch_bounds__(THREADS) void rows_kernel(float const *__restrict__ em, float const *__restrict__ null,
                                                       float const *__restrict__ bg, float const *__restrict__ trans,
                                                       DcpRowsDesc const *__restrict__ desc, int first,
                                                       float *__restrict__ pool)
{
  __shared__ float tile[TILE][PITCH]; // [position][code]
  DcpRowsDesc const d = desc[first + (int)blockIdx.z];
  DcpRowsOut const &o = d.out;
  int const k0 = (int)blockIdx.x * TILE;
  if (k0 >= o.Kp) return; // (Kp is a multiple of the tile)
  int const tid = (int)threadIdx.x, tx = tid & (TILE - 1), ty = tid / TILE;
  float const inf = __uint_as_float(0x7f800000u);

  if ((int)blockIdx.y == CODE_TILES)
  {
    // the transitions, built on the host: columns k0 .. of the eight rows, and behind the last row the padding
    for (int i = tid; i < DCP_NUM_TRANS * TILE; i += THREADS)
    {
      int64_t const at = (int64_t)(i / TILE) * o.Kp + k0 + (i & (TILE - 1));
      pool[d.trans_off + at] = trans[d.trans_src + at];
    }
    if (k0 == 0)
      for (int i = DCP_NUM_TRANS * o.Kp + tid; i < d.trans_floats; i += THREADS)
        pool[d.trans_off + i] = trans[d.trans_src + i];
    return;
  }

  int const c0 = (int)blockIdx.y * TILE;
  for (int kk = ty; kk < TILE; kk += THREADS / TILE)
  {
    int const k = k0 + kk, c = c0 + tx;
    float v = inf;
    if (k < o.K && c < DCP_TABLE_SIZE) v = flip(em[(o.src + k) * DCP_TABLE_SIZE + c]);
    tile[kk][tx] = v;
  }
  __syncthreads();

  int const k = k0 + tx;
  int const col = dcp_out::copy_col(o, k);
  for (int cc = ty; cc < TILE; cc += THREADS / TILE)
  {
    int const c = c0 + cc;
    if (c >= DCP_TABLE_SIZE) break;
    dcp_out::store(pool, o, c, k, col, tile[tx][cc]);
  }

  if (k0 == 0) dcp_out::headers(pool, o, c0, tid, null, bg); // of this tile's codes
}

static_assert(TILE == dcp_out::TILE && THREADS == dcp_out::THREADS, "the tiles press_out_dev.h writes");

} // namespace

int dcp_press_rows_launch(float const *em, float const *null, float const *bg, float const *trans,
                          DcpRowsDesc const *desc, int n, int max_Kp, float *pool, hipStream_t stream)
{
  if (n <= 0 || max_Kp <= 0) return 0;
  unsigned const xtiles = (unsigned)((max_Kp + TILE - 1) / TILE);
  for (int first = 0; first < n; first += 65535) // gridDim.z
  {
    unsigned const z = (unsigned)(n - first < 65535 ? n - first : 65535);
    hipLaunchKernelGGL(rows_kernel, dim3(xtiles, CODE_TILES + 1, z), dim3(THREADS), 0, stream, em, null, bg, trans, desc,
                       first, pool);
    if (hipGetLastError() != hipSuccess) return -1;
  }
  return 0;
}
