// viterbi_kernels.h -- launch interface of the HIP kernels (host side).
#pragma once
#include "dcp_types.h"
#include <hip/hip_runtime.h>

// kernel classes by padded size Kp (dcp_class_of; every class's kernel shapes: DCP_CLASS_TABLE, viterbi_kernels.hip):
//   0..3: Kp = 64..256, one wavefront, 1..4 positions per lane
//   4..10: Kp = 384, 512, 768, 1024, 1536, 2048, 4096, several wavefronts or more positions per lane
//   11:    4096 < K <= 16383, strip by strip
// (DCP_NUM_CLASSES, DCP_STRIP_CLASS and DCP_NUM_PACK_SHAPES: dcp_types.h, for the host-only units as well)
#define DCP_STRIP_POSITIONS 2048 // 64 lanes x 4 positions x 8 wavefronts
#define DCP_MAX_CORE_SIZE 16383 // state ids keep 14 bits for k + 1 (c-core/state.h:27-39)
// per-problem ring scratch of the strip class: rest[5][Kp] + Ipre[5][Kp] floats at the largest Kp
#define DCP_RING_FLOATS ((size_t)10 * DCP_MAX_STRIPS * DCP_STRIP_POSITIONS)
#define DCP_RING_SLOTS 1024 // workgroups of the strip kernel in flight (each takes problems in turn)
int dcp_class_of(int K);                      // -1 when K is not covered
void dcp_class_shape(int cls, int *Q, int *W);

// Several windows per wavefront (viterbi_pack.h), cost pass of short profiles: shape i runs groups of S lanes
// with Q positions per lane, (S - 1) * Q positions at most (DCP_PACK_TABLE, viterbi_kernels.hip: K <= 3 .. 124).
// The tables keep the layout of the class the profile belongs to.
int dcp_pack_shape_of(int K); // -1: no shape holds K
void dcp_pack_shape(int shape, int *Q, int *S);

struct DcpLaunch
{
  float const *pool;             // device: all profile arrays
  DcpProfileDev const *profiles; // device
  DcpProblem const *problems;    // device, all of one kernel class
  DcpCodeRow const *code_rows;   // device
  float const *xt_table;         // device, [rows][DCP_XT_STRIDE]
  float *out;                    // device: cost pass [2*slots] (null, alt); path pass [slots]
  unsigned char *arena;          // device: trellises (path pass only)
  float *ring = nullptr;         // device: strip class only, DCP_RING_SLOTS x DCP_RING_FLOATS
  int nprob;
  hipStream_t stream;
  // cost pass of a class (dcp_launch_cost, dcp_launch_cost_narrow): which windows share an XCD's L2 (dcp_types.h).
  // DCP_PLACE_AUTO: dcp_xcd_placement decides from windows_per_profile, the mean over the profiles of `problems`
  // (0: not known, the plain order); DCP_PLACE_PLAIN / DCP_PLACE_EIGHTHS: as told.  The other launches do not read them.
  int windows_per_profile = 0;
  int placement = DCP_PLACE_AUTO;
};

hipError_t dcp_launch_cost(int cls, DcpLaunch const &a);
// core sizes up to it have a cost kernel of their own on the class's layout (0: none): (5,1) below (6,1), (7,1) below
// (8,1), and K <= 640 as ONE wavefront of ten positions per lane instead of (6,2)'s two
int dcp_class_narrow_limit(int cls);
int dcp_class_narrow_q(int cls); // positions per lane of that one-wavefront kernel: 5, 7, 10 (0: none)
hipError_t dcp_launch_cost_narrow(int cls, DcpLaunch const &a); // cost pass of those windows
hipError_t dcp_launch_path(int cls, DcpLaunch const &a);
// trellis_unzip of every problem of a.problems (all classes): steps[step_off[out] .. step_off[out+1]) is the
// buffer of problem `out`; its steps end at the buffer's end
hipError_t dcp_launch_unzip(DcpLaunch const &a, uint32_t *steps, int64_t const *step_off, int32_t *nsteps);
// fast path pass: cost pass that stores each window's DP table at arena + problem.trellis, then the
// traceback of every problem of a.problems (all classes) into steps / nsteps (as dcp_launch_unzip)
// (in blocks, dcp_types.h: B rows between checkpoints, 0 = whole windows; ckpt_addr[out] = the window's checkpoints)
hipError_t dcp_launch_cost_ckpt(int cls, DcpLaunch const &a, int64_t const *ckpt_addr, int B);
// Launch `it` = 0, 1, .. of the groups of G >= 1 blocks (not the strip class): block dcp_group_block(L, B, G, it, g) of
// every window that has one, g = 0 .. G - 1, into table g of the window's G block tables (dcp_block_table_floats
// apart), one workgroup per (window, g); the traceback then walks those blocks, the highest first.  (B = 0, G = 1,
// it = 0: every window whole.)
hipError_t dcp_launch_cost_store(int cls, DcpLaunch const &a, int64_t const *ckpt_addr, int B, int G, int it);
// (ckpt_addr != NULL, strip class: a window with ckpt_addr[out] == 0 keeps its whole table -- one block, B = 0 -- whatever B)
hipError_t dcp_launch_traceback(DcpLaunch const &a, uint32_t *steps, int64_t const *step_off, int32_t *nsteps,
                                DcpTraceState *states, int B, int G, int it, int64_t const *ckpt_addr = nullptr);
// the strip class, per window: ckpt_addr[out] != 0 = the window's checkpoints (dcp_strip_ckpt_floats each), every B > 0
// rows, its G block tables at DcpProblem::trellis; 0 = the window keeps its whole table there and is one block, taken
// in launch 0.  _ckpt: the checkpoints of the former (not needed when there is none).  _store: launch `it` of the groups
// of G blocks of every window (as dcp_launch_cost_store; a.arena is not used), to be followed by
// dcp_launch_traceback(.., B, G, it, ckpt_addr) or dcp_launch_replay
hipError_t dcp_launch_strip_ckpt(DcpLaunch const &a, int64_t const *ckpt_addr, int B);
hipError_t dcp_launch_strip_store(DcpLaunch const &a, int64_t const *ckpt_addr, int B, int G, int it);
// the same for every window of a.problems (one class, not the strip class) in ONE launch: a workgroup takes its window
// through the checkpoints, then block by block through rows + traceback (DcpProblem::trellis = the table's address)
hipError_t dcp_launch_path_blocks(int cls, DcpLaunch const &a, int64_t const *ckpt_addr, int B, uint32_t *steps,
                                  int64_t const *step_off, int32_t *nsteps, DcpTraceState *states);
// strip class: the trellis replayed row by row (row_replay.h) from the tables dcp_launch_strip_store (launch `it` of the
// groups of G blocks) has just written at DcpProblem::trellis of a.problems.
// aux[4][a.nprob], indexed by DcpProblem::out: the window's trellis (device address), its scratch (3 K floats per row:
// L + 1 rows for a whole table, dcp_replay_block_rows(B) per block table), its checkpoints (0: whole table, as for
// dcp_launch_traceback) and the slot of a.out its score goes to.  A block serves the rows of the traceback's partition.
// max_rows: the most rows (threads) a window has in this launch.
hipError_t dcp_launch_replay(DcpLaunch const &a, int64_t const *aux, int B, int G, int it, int max_rows);
hipError_t dcp_launch_compact_steps(uint32_t const *steps, int64_t const *step_off, int64_t const *compact_off,
                                    uint32_t *out, int n, hipStream_t stream);
// packs of one shape: one wavefront each; a.problems is not used
hipError_t dcp_launch_cost_pack(int shape, DcpLaunch const &a, DcpPack const *packs, int npack, uint32_t ncode_rows);
// lrt of every window from out[2n] = (null, alt); hits[0] = number of windows with a finite lrt >= 0 (zeroed by
// the caller), then (window, lrt bits) pairs, unordered
hipError_t dcp_launch_lrt_filter(float const *out, int n, uint32_t *hits, hipStream_t stream);
// the same with the table rows of the short emission lengths in LDS (all five lengths for groups of four lanes):
// workgroups of dcp_pack_lds_waves(shape) wavefronts, groups[i] = {first pack, number of packs (<= that many,
// all of one profile)}
int dcp_pack_lds_waves(int shape); // 0: the shape reads every row from global memory
hipError_t dcp_launch_cost_pack_lds(int shape, DcpLaunch const &a, DcpPack const *packs, int2 const *groups, int ngroups,
                                    uint32_t ncode_rows);
// every problem of classes 0..3 (single-wave) in one launch
hipError_t dcp_launch_cost_fused(DcpLaunch const &a);

// ---- code_rows.hip ----
// the code rows (code_rows.h) of nreads reads, nt[seq_off[s] .. seq_off[s + 1]), max_len the longest: sequence s is read
// s, row_off[nreads + 1] the rows in front of each; or, on both strands, sequence 2s is read s and 2s + 1 its reverse
// complement, row_off[2 nreads + 1]
hipError_t dcp_launch_encode(unsigned char const *nt, int64_t const *seq_off, int64_t const *row_off, int nreads,
                             bool both, int64_t max_len, DcpCodeRow *rows, hipStream_t stream);
// the code rows of nseq random sequences of len nucleotides (calibrate.h states them), len + 1 rows each, back to back
// from rows[0]: no nt buffer, no loads
hipError_t dcp_launch_random_code_rows(int nseq, int len, uint64_t seed, uint32_t const t[3], DcpCodeRow *rows,
                                       hipStream_t stream);

// ---- calibrate.hip ----
// The scores of one chunk of a calibration's cost pass at one rung of its ladder: out holds the pairs {null, alt} of
// nprof profiles x nseq reads, profile-major; x = dcp_lrt(-null, -alt), as dcp_lrt_filter_kernel forms it, goes to
// scores[profile][nlen][nseq] at [.][rung][read] (scores: at the chunk's first profile).
hipError_t dcp_launch_calib_gather(float const *out, int nprof, int nseq, int nlen, int rung, float *scores, hipStream_t stream);
// Gumbel fit of nprof profiles by maximum likelihood, one wavefront per profile, over scores[nprof][nlen][n]; nlen in
// 1 .. DCP_CALIB_MAX_LENS.  Per rung j the non-finite scores are left out and counted in excluded[p][j]; over the n' kept
//   mu = m - (1 / lambda) * log((1 / n') * sum exp(-lambda * (x - m))),  m = min x,  summed in fp64 (every term <= 1),
// whose fp32 bits are mu_bits[p][j]; NaN when n' = 0.  lambda > 0: that lambda.  lambda == 0: the one lambda per profile
// that maximises the likelihood with a location of its own for every rung -- the root of
//   g(lambda) = sum_j n'_j (1 / lambda - mean_j(y) + T1_j / T0_j),  y = x - m_j,  Tk_j = sum y^k exp(-lambda y),
// over the rungs with n'_j >= 2 and not all scores equal, by Newton's method inside a bracket, to 1e-13 relative -- and
// mu of every rung at it; a profile without such a rung gets NaN for lambda and every mu.  lambda_bits[p]: the fp32 bits
// of the lambda used.  The order of every sum is fixed: the same scores give the same bits.
hipError_t dcp_launch_gumbel_ladder_fit(float const *scores, int nprof, int nlen, int n, float lambda, uint32_t *mu_bits,
                                        int32_t *excluded, uint32_t *lambda_bits, hipStream_t stream);
