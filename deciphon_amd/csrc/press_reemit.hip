// press_reemit.hip -- the emission rows of resident profiles at a new error rate, written where they lie.
//
// A load from a HMMER3 file makes a profile's rows in two kernels: emission_kernel (press_kernel.hip) writes
// em[node][1364] into a scratch buffer, rows_kernel (press_rows.hip) reads it back, transposes it into the code-major
// rows the DP kernels read and copies the transitions.  A change of the error rate alone needs neither the scratch
// buffer nor the transitions: the tables are a function of each node's 129 inputs and e, and the inputs have stayed in
// device memory since the load.  This kernel is the two fused, over the profiles of a whole pool in one launch.
//
// The grid is (pairs, 2): a pair is (profile, k0), one per 64 positions below the profile's Kp, listed on the host
// (dcp_reemit_tiles), so no workgroup is launched to find that it has nothing to do; blockIdx.y picks 11 of the 22
// tiles of 64 codes.  A workgroup takes its 64 positions in two halves.  The inputs of a half's 32 nodes are
// exponentiated into LDS as doubles (33 KB: with the tile, three workgroups fit a CU's 160 KB; all 64 nodes at once,
// 66 KB, would leave one), and are then shared by the 11 code tiles: per tile, wavefront w computes positions w, w + 4,
// ... of the half, lane = code, exactly as emission_kernel does for one node, into an LDS tile [position][code] of
// pitch 65, and the tile goes out transposed, position-major as rows_kernel writes -- a wavefront's store is two runs
// of 32 positions, 128 bytes each, of two codes -- into the canonical rows (+inf beyond K, 0 in the match columns of a
// poisoned profile) and through dcp_cost_order_col into the cost-order copy.  Pairs with k0 = 0 also write the
// {null, bg, 0, 0} headers of both layouts from the model tables of the new error rate.  Nothing else of a profile is
// touched: not the transitions, not the 16 floats behind them.
//
// Why 11 code tiles per workgroup and not one: the kernel is bound by double-precision arithmetic, not by memory (it
// writes at 0.6 TB/s), and exponentiating 32 x 129 inputs costs about as much as the 32 x 64 values of one code tile
// that are computed from them.  Measured on 2000 Pfam-shaped profiles, repeated calls on one engine
// (profiles/r17_set_epsilon.txt): one code tile per workgroup 7.5 ms, two 6.0 ms, eleven 4.7 ms, all 22 the same 4.7 ms
// with half as many workgroups.
//
// The arithmetic is press_emission.h's, shared with emission_kernel and built with the same flags: the words are the
// same as those of a load at that error rate.
#include "press_reemit.h"
#include "dcp_types.h"
#include "press_emission.h"
#include "press_kernel.h"
#include "press_out_dev.h"

#include <hip/hip_runtime.h>

namespace
{

using namespace dcp_emission;

constexpr int TILE = DCP_REEMIT_TILE;
constexpr int PITCH = TILE + 1;
constexpr int HALF = TILE / 2; // nodes whose inputs are in LDS at a time
constexpr int THREADS = 256;
constexpr int WAVES = THREADS / TILE;
constexpr int CODE_TILES = (DCP_TABLE_SIZE + TILE - 1) / TILE; // 22: 21 whole ones and one of 20 codes
constexpr int CT = 11;                                         // code tiles per workgroup
constexpr int64_t MAX_PAIRS = (int64_t)1 << 22;                // per launch: gridDim.x * THREADS stays below 2^32

using dcp_out::flip;

__global__ __launch_bounds__(THREADS) void reemit_kernel(float const *__restrict__ dist, float const *__restrict__ models,
                                                         DcpReemitDesc const *__restrict__ desc,
                                                         int32_t const *__restrict__ pair_profile,
                                                         int32_t const *__restrict__ pair_k0, int64_t first, float epsilon,
                                                         float *__restrict__ pool)
{
  __shared__ double prob[HALF][INPUTS];
  __shared__ float tile[HALF][PITCH]; // [position][code]
  int64_t const pair = first + (int64_t)blockIdx.x;
  DcpReemitDesc const d = desc[pair_profile[pair]];
  DcpRowsOut const &o = d.out;
  int const k0 = pair_k0[pair]; // (a multiple of the tile below Kp)
  int const tid = (int)threadIdx.x, tx = tid & (TILE - 1), ty = tid / TILE;
  float const inf = __uint_as_float(0x7f800000u);
  double const le = log((double)epsilon), lf = log1p(-(double)epsilon);

  for (int h = 0; h < TILE / HALF; ++h)
  {
    int const kh = k0 + h * HALF;
    int const nodes = o.K - kh < HALF ? o.K - kh : HALF; // of this half below K; may be <= 0
    for (int i = tid; i < nodes * INPUTS; i += THREADS)
    {
      int const node = i / INPUTS, j = i % INPUTS;
      prob[node][j] = input_prob(dist[(o.src + kh + node) * DCP_PRESS_IN_STRIDE + j]);
    }
    __syncthreads();
    int const k = kh + (tx & (HALF - 1)); // the position this lane writes
    int const col = dcp_out::copy_col(o, k);
    for (int ct = 0; ct < CT; ++ct)
    {
      int const c0 = ((int)blockIdx.y * CT + ct) * TILE;
      int z[5];
      int const code = c0 + tx;
      int const n = decode(code, z);
      for (int kk = ty; kk < HALF; kk += WAVES)
      {
        float v = inf;
        if (kk < nodes && code < DCP_TABLE_SIZE)
        {
          State const s{prob[kk], prob[kk] + 4, dist + (o.src + kh + kk) * DCP_PRESS_IN_STRIDE};
          v = flip(emission_lprob(s, le, lf, n, z));
        }
        tile[kk][tx] = v;
      }
      __syncthreads();
      for (int cc = 2 * ty + tx / HALF; cc < TILE; cc += 2 * WAVES)
      {
        int const c = c0 + cc;
        if (c >= DCP_TABLE_SIZE) continue;
        dcp_out::store(pool, o, c, k, col, tile[tx & (HALF - 1)][cc]);
      }
      __syncthreads(); // the tile has been read, and after the last code tile the half's inputs
    }
  }

  if (k0 != 0) return;
  // the headers of this workgroup's codes
  float const *null = models + (int64_t)d.null_row * DCP_PRESS_TABLE, *bg = models + (int64_t)d.bg_row * DCP_PRESS_TABLE;
  for (int ct = 0; ct < CT; ++ct) dcp_out::headers(pool, o, ((int)blockIdx.y * CT + ct) * TILE, tid, null, bg);
}

static_assert(TILE == dcp_out::TILE && THREADS == dcp_out::THREADS, "the tiles press_out_dev.h writes");
static_assert(CODE_TILES % CT == 0, "whole workgroups of code tiles");
static_assert(DCP_PRESS_TABLE == DCP_TABLE_SIZE, "the model tables are rows of the emission kernel");

} // namespace

int dcp_press_reemit_launch(float const *dist, float const *models, DcpReemitDesc const *desc, int32_t const *pair_profile,
                            int32_t const *pair_k0, int64_t n, float epsilon, float *pool, hipStream_t stream)
{
  for (int64_t first = 0; first < n; first += MAX_PAIRS) // gridDim.x
  {
    unsigned const x = (unsigned)(n - first < MAX_PAIRS ? n - first : MAX_PAIRS);
    hipLaunchKernelGGL(reemit_kernel, dim3(x, CODE_TILES / CT), dim3(THREADS), 0, stream, dist, models, desc, pair_profile,
                       pair_k0, first, epsilon, pool);
    if (hipGetLastError() != hipSuccess) return -1;
  }
  return 0;
}
