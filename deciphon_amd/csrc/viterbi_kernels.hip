// viterbi_kernels.hip -- gfx950 kernels of the Viterbi scan path.
//
// One workgroup per (profile x window) problem: a single wavefront for K <= 256
// (Q = 1..4 positions per lane), W = 2..16 wavefronts of Q = 4 beyond that.
// Problems of one launch share the kernel class (Q, W), K <= 64*Q*W.
#include <stdlib.h>

#include "lane_ops_gpu.h"
#include "viterbi_body.h"
#include "viterbi_pack.h"
#include "traceback.h"
#include "viterbi_kernels.h"
#include "row_replay.h"

// A device address that reaches a kernel as an INTEGER (the table and checkpoint addresses in DcpProblem::trellis and
// ckpt_addr[]) would make every access through it a flat_* instruction: the compiler cannot know the address space,
// flat accesses may complete out of order, and each use of a loaded value then waits for ALL outstanding memory
// operations -- the emission prefetch of the next row and the stores of this one included (vmcnt(0) twice per row).
// Going through an address_space(1) pointer tells it the memory is global: global_load / global_store, counted waits.
template <class T> __device__ __forceinline__ T *dcp_global(uintptr_t address)
{
  return (T *)(__attribute__((address_space(1))) T *)address;
}

// Which list entry a workgroup takes (dcp_types.h, "which XCD's L2 serves which windows"): dcp_xcd_eighths_entry, under
// the names the kernels have always used.  The cost kernels of a class take the eighths or the plain order as the host
// decided for the launch (DcpLaunch::placement, dcp_xcd_placement).
__device__ __forceinline__ int dcp_xcd_remap_any(int b, int n) { return dcp_xcd_eighths_entry(b, n); }
// The fused kernel and the packs: a launch of about one generation of wavefronts keeps the plain order.  Their lists
// are not even in time (the fused kernel's windows belong to profiles of different classes, a shape's packs go
// longest first inside a profile), and in a small launch nothing is left to even the eighths out.
__device__ __forceinline__ int dcp_xcd_remap(int b, int n) { return n < 16384 ? b : dcp_xcd_remap_any(b, n); }
// The path pass's kernels take the eighths whatever the size of the launch: all their wavefronts are resident at once
// (nothing to even out), and what they wait for is memory -- the 2301 hit windows of the headline scan fetch 140 GB of
// emission rows and write 66 GB of tables in 50 ms (scripts/pmc_path.sh).  With the windows of a profile on one XCD
// instead of all eight, the pass takes 46.5 ms instead of 51 (profiles/r03_path_pass_pmc.txt).

// Wavefronts per SIMD the register allocator must leave room for.  A wavefront issues a VALU every ~7.5 cycles
// whatever its instruction-level parallelism (profiles/r02_valu_rates.txt), so two wavefronts per SIMD cap the
// issue rate at 640 G/s and three at 729.  Holding a shape to fewer registers by the bound alone spills into the row
// loop (Q = 3 / 4 to 96 / 128 VGPRs: 6-7 scratch reloads per row, 881 -> 620 GCUPS at K = 173, 1000 -> 878 at K = 256;
// (6,1), (7,1) to 168: 26-55 per row -- profiles/r02_exp_trans_stash_occupancy.txt).  Asking for the next row's
// emissions later in the row (DCP_COST_POLICY bit 1, viterbi_body.h) frees Q registers per emission length at the
// peak instead: (4,1) 147 -> 128 VGPRs = four wavefronts per SIMD instead of three (K = 256: 1102 -> 1199 GCUPS),
// (5,1) fits 168 with nothing spilled inside the loop (K = 300: 961 -> 1006), and ten positions per lane fit one
// wavefront at all ((10,1), 226 VGPRs: K = 513..640 run 32-38 % faster than as two wavefronts of five).  Where the
// wavefronts per SIMD stay what they were it brings nothing ((3,1), (6,1), (7,1): profiles/r03_exp_register_policy.txt).
#ifndef DCP_COST_WAVES
#define DCP_COST_WAVES(Q, W) ((W) == 1 && (Q) == 4 ? 4 : (W) == 1 && (Q) == 5 ? 3 : (Q) >= 8 ? 2 : 1)
#endif
template <int Q, int W, int POLICY = DCP_COST_POLICY(Q, W), int WAVES = DCP_COST_WAVES(Q, W)>
__global__ __launch_bounds__(64 * W, WAVES) void dcp_cost_kernel(float const *__restrict__ pool,
                                                      DcpProfileDev const *__restrict__ profiles,
                                                      DcpProblem const *__restrict__ problems,
                                                      DcpCodeRow const *__restrict__ code_rows,
                                                      float const *__restrict__ xt_table,
                                                      float *__restrict__ out, int nprob, int eighths)
{
  if ((int)blockIdx.x >= nprob) return;
#ifdef DCP_EXP_LDSPAD // timing experiment (profiles/r02_exp_*): LDS nobody uses holds the wavefronts per SIMD down
  __shared__ float pad[DCP_EXP_LDSPAD / 4];
  if (nprob < 0) out[0] = pad[threadIdx.x];
#endif
  int const p = eighths ? dcp_xcd_remap_any((int)blockIdx.x, nprob) : (int)blockIdx.x;
  DcpProblem const pb = problems[p];
  DcpProfileDev const pf = profiles[pb.profile];
  CostWave<Q, W, false, POLICY> w;
  w.init(pool, pf, code_rows + pb.code_row, xt_table + (size_t)pb.xt_row * DCP_XT_STRIDE);
  w.run(pb.L, out + 2 * (size_t)pb.out);
}

// Fast path pass in blocks (dcp_types.h).  First the checkpoints: the cost pass once more over the hit windows,
// leaving the folded ring of five rows every B rows (windows of a single block need none and leave at once).
template <int Q, int W>
__global__ __launch_bounds__(64 * W, (Q >= 8 ? 2 : 1)) void dcp_cost_ckpt_kernel(float const *__restrict__ pool,
                                                           DcpProfileDev const *__restrict__ profiles,
                                                           DcpProblem const *__restrict__ problems,
                                                           DcpCodeRow const *__restrict__ code_rows,
                                                           float const *__restrict__ xt_table,
                                                           int64_t const *__restrict__ ckpt_addr, int B,
                                                           float *__restrict__ out, int nprob)
{
  if ((int)blockIdx.x >= nprob) return;
  DcpProblem const pb = problems[dcp_xcd_remap_any((int)blockIdx.x, nprob)];
  if (dcp_num_blocks(pb.L, B) <= 1) return;
  DcpProfileDev const pf = profiles[pb.profile];
  CostWave<Q, W> w;
  w.ckpt_out = dcp_global<float>((uintptr_t)ckpt_addr[pb.out]);
  w.ckpt_every = B;
  w.init(pool, pf, code_rows + pb.code_row, xt_table + (size_t)pb.xt_row * DCP_XT_STRIDE);
  w.run(pb.L, out + 2 * (size_t)pb.out);
}

// Then the blocks (DcpBlock, dcp_types.h) from the last to the first, G of every window side by side, one workgroup
// each: every block of a window that has one in launch `it`, recomputed from its checkpoint into one of the window's G
// tables -- the blocks of a window are independent once its checkpoints exist, and a lone wavefront per window leaves
// the GPU empty and waits out every row's latency by itself (profiles/r03_scan_pipeline.txt).  Workgroup b takes window
// b / G and table b % G.  B = 0: the whole window is one block and its table holds all its rows.
template <int Q, int W>
__global__ __launch_bounds__(64 * W, (Q >= 8 ? 2 : 1)) void dcp_cost_store_kernel(float const *__restrict__ pool,
                                                            DcpProfileDev const *__restrict__ profiles,
                                                            DcpProblem const *__restrict__ problems,
                                                            DcpCodeRow const *__restrict__ code_rows,
                                                            float const *__restrict__ xt_table,
                                                            unsigned char *__restrict__ arena,
                                                            int64_t const *__restrict__ ckpt_addr, int B, int G, int it,
                                                            float *__restrict__ out, int nprob)
{
  if ((int)blockIdx.x >= nprob * G) return;
  int const b = dcp_xcd_remap_any((int)blockIdx.x, nprob * G); // (window, block) pairs in eighths: whole windows, mostly
  int const sub = b % G;
  DcpProblem const pb = problems[b / G];
  int const block = dcp_group_block(pb.L, B, G, it, sub);
  if (block < 0) return;
  DcpProfileDev const pf = profiles[pb.profile];
  DcpBlock const blk = dcp_block(pb.L, B, block);
  CostWave<Q, W, true> w;
  // integer arithmetic: the engine passes arena = 0 and absolute table addresses in pb.trellis
  dcp_bind_block(w, dcp_global<float>((uintptr_t)arena + (uintptr_t)pb.trellis) + dcp_group_table(pb.L, pf.Kp, B, sub),
                 dcp_global<float const>((uintptr_t)ckpt_addr[pb.out]), blk, pf.Kp);
  w.init(pool, pf, code_rows + pb.code_row, xt_table + (size_t)pb.xt_row * DCP_XT_STRIDE);
  w.run(pb.L, out + 2 * (size_t)pb.out, blk.last);
}

// Profiles beyond 4096 positions: one workgroup walks each row strip by strip (StripWave).
template <int Q, int W>
__global__ __launch_bounds__(64 * W) void dcp_strip_kernel(float const *__restrict__ pool,
                                                       DcpProfileDev const *__restrict__ profiles,
                                                       DcpProblem const *__restrict__ problems,
                                                       DcpCodeRow const *__restrict__ code_rows,
                                                       float const *__restrict__ xt_table,
                                                       unsigned char *__restrict__ /* arena: no table */,
                                                       float *__restrict__ ring, float *__restrict__ out, int nprob)
{
  // the grid is at most DCP_RING_SLOTS workgroups, each owning one ring and taking problems in turn
  for (int p = (int)blockIdx.x; p < nprob; p += (int)gridDim.x)
  {
    DcpProblem const pb = problems[p];
    DcpProfileDev const pf = profiles[pb.profile];
    StripWave<Q, W> w;
    w.ring = ring + (size_t)blockIdx.x * DCP_RING_FLOATS;
    w.init(pool, pf, code_rows + pb.code_row, xt_table + (size_t)pb.xt_row * DCP_XT_STRIDE);
    w.run(pb.L, out + 2 * (size_t)pb.out);
    __syncthreads(); // the next problem re-initialises the LDS records
  }
}

// The strip class in blocks (dcp_types.h), per window: ckpt_addr[out] != 0 is a window whose table is held a block at a
// time, 0 one that keeps its whole table (one block, B = 0) -- a request may mix the two.  First the checkpoints of the
// windows that go in blocks ...
template <int Q, int W>
__global__ __launch_bounds__(64 * W) void dcp_strip_ckpt_kernel(float const *__restrict__ pool,
                                                            DcpProfileDev const *__restrict__ profiles,
                                                            DcpProblem const *__restrict__ problems,
                                                            DcpCodeRow const *__restrict__ code_rows,
                                                            float const *__restrict__ xt_table,
                                                            int64_t const *__restrict__ ckpt_addr, int B,
                                                            float *__restrict__ ring, float *__restrict__ out, int nprob)
{
  for (int p = (int)blockIdx.x; p < nprob; p += (int)gridDim.x)
  {
    DcpProblem const pb = problems[p];
    int64_t const ck = ckpt_addr[pb.out];
    if (ck == 0 || dcp_num_blocks(pb.L, B) <= 1) continue; // (uniform: no barrier is skipped by a part of the workgroup)
    DcpProfileDev const pf = profiles[pb.profile];
    StripWave<Q, W, false> w;
    w.ring = ring + (size_t)blockIdx.x * DCP_RING_FLOATS;
    w.ckpt_out = dcp_global<float>((uintptr_t)ck);
    w.ckpt_every = B;
    w.init(pool, pf, code_rows + pb.code_row, xt_table + (size_t)pb.xt_row * DCP_XT_STRIDE);
    w.run(pb.L, out + 2 * (size_t)pb.out);
    __syncthreads(); // the next problem re-initialises the LDS records
  }
}

// ... then launch `it` of the groups of G blocks, as dcp_cost_store_kernel: item i = (window i / G, table i % G).  A
// workgroup owns one ring and takes items in turn.
template <int Q, int W>
__global__ __launch_bounds__(64 * W) void dcp_strip_store_kernel(float const *__restrict__ pool,
                                                             DcpProfileDev const *__restrict__ profiles,
                                                             DcpProblem const *__restrict__ problems,
                                                             DcpCodeRow const *__restrict__ code_rows,
                                                             float const *__restrict__ xt_table,
                                                             int64_t const *__restrict__ ckpt_addr, int B, int G, int it,
                                                             float *__restrict__ ring, float *__restrict__ out, int nprob)
{
  for (int i = (int)blockIdx.x; i < nprob * G; i += (int)gridDim.x)
  {
    int const sub = i % G;
    DcpProblem const pb = problems[i / G];
    int64_t const ck = ckpt_addr[pb.out];
    int const Bw = ck != 0 ? B : 0;
    int const block = dcp_group_block(pb.L, Bw, G, it, sub);
    if (block < 0) continue;
    DcpProfileDev const pf = profiles[pb.profile];
    DcpBlock const blk = dcp_block(pb.L, Bw, block);
    StripWave<Q, W, true> w;
    w.ring = ring + (size_t)blockIdx.x * DCP_RING_FLOATS;
    dcp_bind_block(w, dcp_global<float>((uintptr_t)pb.trellis) + dcp_group_table(pb.L, pf.Kp, Bw, sub),
                   dcp_global<float const>((uintptr_t)ck), blk, pf.Kp);
    w.init(pool, pf, code_rows + pb.code_row, xt_table + (size_t)pb.xt_row * DCP_XT_STRIDE);
    w.run(pb.L, out + 2 * (size_t)pb.out, blk.last);
    __syncthreads();
  }
}

// one row of one window's trellis: thread r of the window in launch `it` (dcp_launch_replay)
__device__ void dcp_replay_one(float const *__restrict__ pool, DcpProfileDev const *__restrict__ profiles,
                               DcpProblem const pb, DcpCodeRow const *__restrict__ code_rows,
                               float const *__restrict__ xt_table, int64_t const *__restrict__ aux, int naux, int B, int G,
                               int it, float *__restrict__ out)
{
  int const r = (int)(blockIdx.x * 64u + threadIdx.x);
  int const Bw = aux[2 * (size_t)naux + pb.out] != 0 ? B : 0; // no checkpoints: the whole table, one block
  DcpProfileDev const pf = profiles[pb.profile];
  // trellis of a problem: uint32 xnodes[L+1] then uint16 nodes[(L+1)*K]
  uint32_t *xnodes = dcp_global<uint32_t>((uintptr_t)aux[pb.out]);
  DcpTraceIn in = dcp_trace_in(pool, pf, code_rows + pb.code_row, xt_table + (size_t)pb.xt_row * DCP_XT_STRIDE, pb.L);
  int const l = dcp_replay_thread(in, dcp_global<float const>((uintptr_t)pb.trellis), Bw, G, it, r,
                                  dcp_global<float>((uintptr_t)aux[(size_t)naux + pb.out]), xnodes,
                                  reinterpret_cast<uint16_t *>(xnodes + (pb.L + 1)));
  if (l > 0 && l == pb.L) // T of the last row: the score viterbi_path returns (c-core/viterbi.c:585-586,599)
  {
    float const *last = in.sp + (size_t)(l - in.row_base) * DCP_SP_STRIDE;
    out[aux[3 * (size_t)naux + pb.out]] = __builtin_fminf(last[3] + in.xt[DCP_ET], last[4] + in.xt[DCP_CT]);
  }
}

// The pass-by-pass trellis of profiles beyond 4096 positions: every row replayed from the DP table
// by one thread (row_replay.h).  blockIdx.y (strided: the y extent of a grid stops at 65535) = problem,
// blockIdx.x * 64 + threadIdx.x = row of the window in this launch.
__global__ __launch_bounds__(64) void dcp_replay_kernel(
    float const *__restrict__ pool, DcpProfileDev const *__restrict__ profiles, DcpProblem const *__restrict__ problems,
    DcpCodeRow const *__restrict__ code_rows, float const *__restrict__ xt_table, int64_t const *__restrict__ aux, int B,
    int G, int it, float *__restrict__ out, int nprob)
{
  for (int p = (int)blockIdx.y; p < nprob; p += (int)gridDim.y)
    dcp_replay_one(pool, profiles, problems[p], code_rows, xt_table, aux, nprob, B, G, it, out);
}

hipError_t dcp_launch_replay(DcpLaunch const &a, int64_t const *aux, int B, int G, int it, int max_rows)
{
  if (a.nprob <= 0) return hipSuccess;
  if (!aux || B < 0 || B % 5 || G < 1 || it < 0 || max_rows < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(dcp_replay_kernel, dim3((unsigned)((max_rows + 63) / 64), (unsigned)(a.nprob < 65535 ? a.nprob : 65535)), dim3(64), 0, a.stream,
                     a.pool, a.profiles, a.problems, a.code_rows, a.xt_table, aux, B, G, it, a.out, a.nprob);
  return hipGetLastError();
}

// What a walk that came to its end (r != 0: finished, or given up) leaves for the host and for the launches after
// it; true when it did.
__device__ __forceinline__ bool dcp_trace_end(int r, DcpTraceState *st, int32_t *nsteps)
{
  if (r != 0 && DcpLanesWave::leader())
  {
    st->status = r > 0 ? 1 : r;
    *nsteps = r;
  }
  return r != 0;
}

// Fast path pass, step 2: one WAVEFRONT walks one window's DP table back from T to S (traceback.h).
__global__ __launch_bounds__(64) void dcp_traceback_kernel(
    float const *__restrict__ pool, DcpProfileDev const *__restrict__ profiles, DcpProblem const *__restrict__ problems,
    DcpCodeRow const *__restrict__ code_rows, float const *__restrict__ xt_table,
    unsigned char const *__restrict__ arena, uint32_t *__restrict__ steps, int64_t const *__restrict__ step_off,
    int32_t *__restrict__ nsteps, DcpTraceState *__restrict__ states, int B, int G, int it,
    int64_t const *__restrict__ ckpt_addr, int nprob)
{
  int const p = (int)blockIdx.x;
  if (p >= nprob) return;
  DcpProblem const pb = problems[p];
  if (ckpt_addr && ckpt_addr[pb.out] == 0) B = 0; // strip class: this window keeps its whole table (dcp_strip_store_kernel)
  DcpTraceState *st = states + pb.out;
  if (st->status != 0) return; // finished, or given up, in a later block
  DcpProfileDev const pf = profiles[pb.profile];
  DcpTraceIn in = dcp_trace_in(pool, pf, code_rows + pb.code_row, xt_table + (size_t)pb.xt_row * DCP_XT_STRIDE, pb.L);
  // through the (up to) G blocks that launch `it` of the store kernel has just written, the highest first
  int const r = dcp_traceback_group<DcpLanesWave>(in, dcp_global<float const>((uintptr_t)arena + (uintptr_t)pb.trellis), B, G, it,
                                                  steps + step_off[pb.out], step_off[pb.out + 1] - step_off[pb.out], st);
  dcp_trace_end(r, st, nsteps + pb.out);
}

// The fast path pass of ONE window from start to end in one workgroup (what dcp_cost_ckpt_kernel, then per block
// dcp_cost_store_kernel + dcp_traceback_kernel do in 1 + 2 x blocks launches): the checkpoints, then block by block
// from the last to the first the rows of the block into the window's table and the traceback through them by the
// workgroup's first wavefront.  Windows of one launch no longer wait for each other between blocks -- a window of
// two blocks is done after two -- and nothing returns to the host in between.  The table rows a traceback reads
// were written by wavefronts of its own workgroup: the workgroup barrier orders them (one CU, one vector L1).
template <int Q, int W>
__global__ __launch_bounds__(64 * W, (Q >= 8 ? 2 : 1)) void dcp_path_blocks_kernel(
    float const *__restrict__ pool, DcpProfileDev const *__restrict__ profiles, DcpProblem const *__restrict__ problems,
    DcpCodeRow const *__restrict__ code_rows, float const *__restrict__ xt_table, int64_t const *__restrict__ ckpt_addr,
    int B, float *__restrict__ out, uint32_t *__restrict__ steps, int64_t const *__restrict__ step_off,
    int32_t *__restrict__ nsteps, DcpTraceState *__restrict__ states, int nprob)
{
  if ((int)blockIdx.x >= nprob) return;
  __shared__ int walk_over;
  DcpProblem const pb = problems[dcp_xcd_remap_any((int)blockIdx.x, nprob)];
  DcpProfileDev const pf = profiles[pb.profile];
  DcpCodeRow const *codes = code_rows + pb.code_row;
  float const *xt = xt_table + (size_t)pb.xt_row * DCP_XT_STRIDE;
  int const nb = dcp_num_blocks(pb.L, B);
  float *ckpt = nb > 1 ? dcp_global<float>((uintptr_t)ckpt_addr[pb.out]) : nullptr;
  if (nb > 1)
  {
    CostWave<Q, W> w;
    w.ckpt_out = ckpt;
    w.ckpt_every = B;
    w.init(pool, pf, codes, xt);
    // the path pass runs beside the cost kernels of the batches in flight (dcp_scan_run): its few wavefronts are bound
    // by latency, so they go first wherever they share a SIMD -- what they take from the others is a few per cent
    wave_priority<3>();
    w.run(pb.L, out + 2 * (size_t)pb.out);
  }
  float *table = dcp_global<float>((uintptr_t)pb.trellis);
  for (int block = nb - 1; block >= 0; --block)
  {
    DcpBlock const blk = dcp_block(pb.L, B, block);
    __syncthreads(); // the checkpoints are written; the walk through the block above has left the table
    {
      CostWave<Q, W, true> w;
      dcp_bind_block(w, table, ckpt, blk, pf.Kp);
      w.init(pool, pf, codes, xt);
      wave_priority<3>();
      w.run(pb.L, out + 2 * (size_t)pb.out, blk.last);
    }
    __threadfence_block();
    __syncthreads();
    if (threadIdx.x < 64)
    {
      DcpTraceState *st = states + pb.out;
      DcpTraceIn in = dcp_trace_in(pool, pf, codes, xt, pb.L);
      dcp_trace_bind(in, table, blk);
      int const r = dcp_traceback<DcpLanesWave>(in, steps + step_off[pb.out], step_off[pb.out + 1] - step_off[pb.out], st);
      bool const over = dcp_trace_end(r, st, nsteps + pb.out);
      if (threadIdx.x == 0) walk_over = over;
    }
    __syncthreads();
    if (walk_over) break; // finished, or given up (a tie the values cannot resolve: the literal pass takes it)
  }
}

// All single-wave classes in one launch: small scans (a few thousand windows spread
// over several classes) would otherwise run their per-class kernels one after the
// other, each too small to fill 1024 SIMDs.  Costs the register budget of the
// largest class, so it is used only when the launch is small (engine.cpp).
__global__ __launch_bounds__(64) void dcp_cost_kernel_fused(float const *__restrict__ pool,
                                                            DcpProfileDev const *__restrict__ profiles,
                                                            DcpProblem const *__restrict__ problems,
                                                            DcpCodeRow const *__restrict__ code_rows,
                                                            float const *__restrict__ xt_table,
                                                            float *__restrict__ out, int nprob)
{
  if ((int)blockIdx.x >= nprob) return;
  int const p = dcp_xcd_remap((int)blockIdx.x, nprob);
  DcpProblem const pb = problems[p];
  DcpProfileDev const pf = profiles[pb.profile];
  DcpCodeRow const *codes = code_rows + pb.code_row;
  float const *xt = xt_table + (size_t)pb.xt_row * DCP_XT_STRIDE;
  float *o = out + 2 * (size_t)pb.out;
  switch (pf.Q)
  {
  case 1: { CostWave<1, 1> w; w.init(pool, pf, codes, xt); w.run(pb.L, o); break; }
  case 2: { CostWave<2, 1> w; w.init(pool, pf, codes, xt); w.run(pb.L, o); break; }
  case 3: { CostWave<3, 1> w; w.init(pool, pf, codes, xt); w.run(pb.L, o); break; }
  default: { CostWave<4, 1> w; w.init(pool, pf, codes, xt); w.run(pb.L, o); break; }
  }
}

// Several windows of one profile per wavefront (viterbi_pack.h): one workgroup = one wavefront = one DcpPack.
// (four positions per lane with the next row's operands asked for late: 180 -> 155 VGPRs, three wavefronts per SIMD)
#ifndef DCP_PACK_WAVES
#define DCP_PACK_WAVES(Q) ((Q) == 4 ? 3 : 1)
#endif
template <int Q, int S, bool LATE = DCP_PACK_LATE(Q), int WAVES = DCP_PACK_WAVES(Q)>
__global__ __launch_bounds__(64, WAVES) void dcp_cost_pack_kernel(float const *__restrict__ pool,
                                                           DcpProfileDev const *__restrict__ profiles,
                                                           DcpPack const *__restrict__ packs,
                                                           DcpCodeRow const *__restrict__ code_rows, uint32_t ncode_rows,
                                                           float const *__restrict__ xt_table, float *__restrict__ out,
                                                           int npack)
{
  if ((int)blockIdx.x >= npack) return;
  DcpPack const &pk = packs[dcp_xcd_remap((int)blockIdx.x, npack)];
  DcpProfileDev const pf = profiles[pk.profile];
  PackWave<Q, S, dcp_lazy_turns(Q), 0, LATE> w;
  w.init(pool, pf, code_rows, ncode_rows, xt_table, pk);
  w.run(pk.Lmax, out, pk, xt_table);
}

// The same with the rows of the short emission lengths in LDS (viterbi_pack.h, NLDS): a workgroup of WG
// wavefronts = WG packs of ONE profile (groups[blockIdx] = first pack, number of packs) copies the first
// DCP_PACK_LDS_ROWS(NLDS) rows of the profile's table -- header and position columns -- once, and every
// wavefront gathers those operands from there.
template <int Q, int S, int WG, int NLDS, bool LATE = DCP_PACK_LATE(Q)>
__global__ __launch_bounds__(64 * WG) void dcp_cost_pack_lds_kernel(float const *__restrict__ pool,
                                                                   DcpProfileDev const *__restrict__ profiles,
                                                                   DcpPack const *__restrict__ packs,
                                                                   int2 const *__restrict__ groups,
                                                                   DcpCodeRow const *__restrict__ code_rows,
                                                                   uint32_t ncode_rows, float const *__restrict__ xt_table,
                                                                   float *__restrict__ out, int ngroups)
{
  constexpr int RL = DCP_PACK_LDS_ROW(Q, S), NR = DCP_PACK_LDS_ROWS(NLDS);
  __shared__ __attribute__((aligned(16))) float table[NR * RL];
  if ((int)blockIdx.x >= ngroups) return;
  int2 const grp = groups[blockIdx.x];
  DcpProfileDev const pf = profiles[packs[grp.x].profile];
  float const *__restrict__ rows = pool + pf.rows_off;
  int const stride = pf.Kp + DCP_ROW_HDR;
  int const used = pf.K + DCP_ROW_HDR; // the columns behind it are the +inf padding: not fetched
  for (int i = (int)threadIdx.x; i < NR * RL; i += 64 * WG)
  {
    int const c = i / RL, j = i - c * RL;
    table[i] = j < used ? rows[(size_t)c * stride + j] : __builtin_inff();
  }
  __syncthreads();
  int const wave = (int)(threadIdx.x >> 6);
  if (wave >= grp.y) return; // no barrier follows
  DcpPack const &pk = packs[grp.x + wave];
  PackWave<Q, S, dcp_lazy_turns(Q), NLDS, LATE> w;
  w.init(pool, pf, code_rows, ncode_rows, xt_table, pk, (lds_float const *)table);
  w.run(pk.Lmax, out, pk, xt_table);
}

template <int Q, int W>
__global__ __launch_bounds__(64 * W) void dcp_path_kernel(float const *__restrict__ pool,
                                                      DcpProfileDev const *__restrict__ profiles,
                                                      DcpProblem const *__restrict__ problems,
                                                      DcpCodeRow const *__restrict__ code_rows,
                                                      float const *__restrict__ xt_table,
                                                      unsigned char *__restrict__ arena,
                                                      float *__restrict__ out, int nprob)
{
  int const p = (int)blockIdx.x;
  if (p >= nprob) return;
  DcpProblem const pb = problems[p];
  DcpProfileDev const pf = profiles[pb.profile];
  // trellis of a problem: uint32 xnodes[L+1] then uint16 nodes[(L+1)*K]
  uint32_t *xnodes = reinterpret_cast<uint32_t *>(arena + pb.trellis);
  uint16_t *nodes = reinterpret_cast<uint16_t *>(xnodes + (pb.L + 1));
  PathWave<Q, W> w;
  w.init(pool, pf, code_rows + pb.code_row, xt_table + (size_t)pb.xt_row * DCP_XT_STRIDE, xnodes, nodes);
  float const T = w.run(pb.L);
  store_f32_lane0(out + pb.out, w.g.lane, T);
}

// trellis_unzip on the device (dcp_trellis_step, dcp_states.h): one thread walks one problem's trellis from T at stage L
// back to S at stage 0 and writes the steps, packed as state_id | seqsize << 16, from
// the END of its buffer backwards, so that they read forwards in path order.
// nsteps[p] = number of steps, or -1 when the buffer was too small / the trellis is
// inconsistent (the host then unzips that one itself).
__global__ void dcp_unzip_kernel(DcpProfileDev const *__restrict__ profiles, DcpProblem const *__restrict__ problems,
                                 unsigned char const *__restrict__ arena, uint32_t *__restrict__ steps,
                                 int64_t const *__restrict__ step_off, int32_t *__restrict__ nsteps, int nprob)
{
  int const p = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (p >= nprob) return;
  DcpProblem const pb = problems[p];
  int const K = profiles[pb.profile].K;
  int const L = pb.L;
  uint32_t const *xnodes = reinterpret_cast<uint32_t const *>(arena + pb.trellis);
  uint16_t const *nodes = reinterpret_cast<uint16_t const *>(xnodes + (L + 1));
  uint32_t *buf = steps + step_off[pb.out];
  int64_t const cap = step_off[pb.out + 1] - step_off[pb.out];
  int state = ST_T, stage = L;
  int64_t n = 0;
  bool bad = false;
  while ((state != ST_S || stage) && !bad)
  {
    DcpStep const step = dcp_trellis_step(K, xnodes, nodes, state, stage);
    if (step.prev < 0 || n + 1 >= cap) { bad = true; break; }
    buf[cap - 1 - n] = (uint32_t)state | ((uint32_t)step.size << 16);
    ++n;
    state = step.prev;
    stage -= step.size;
    if (stage < 0) bad = true;
  }
  if (!bad && n < cap)
  {
    buf[cap - 1 - n] = (uint32_t)state; // the start state, no emission
    ++n;
  }
  else
    bad = true;
  nsteps[pb.out] = bad ? -1 : (int32_t)n;
}

// The filter of process_window (c-core/thread.c:118-121) on the device: dcp_lrt of every window (dcp_types.h), and the windows that go on to the path pass -- lrt finite and
// >= 0 -- appended to a list: hits[0] counts them, then (window, lrt bits) pairs, in no particular order (the
// host sorts the few that there are).
__global__ void dcp_lrt_filter_kernel(float const *__restrict__ out, int n, uint32_t *__restrict__ hits)
{
  int const i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  bool keep = false;
  float lrt = 0.0f;
  if (i < n)
  {
    float const null_loglik = -out[2 * (size_t)i], alt_loglik = -out[2 * (size_t)i + 1];
    lrt = dcp_lrt(null_loglik, alt_loglik);
    keep = lrt >= 0.0f && lrt < __builtin_inff(); // finite (not NaN, not +inf) and not negative
  }
  unsigned long long const mask = __ballot(keep);
  if (!mask) return;
  int const lane = (int)(threadIdx.x & 63);
  uint32_t base = 0;
  if (lane == __ffsll((long long)mask) - 1) base = atomicAdd(hits, (uint32_t)__popcll(mask));
  base = (uint32_t)__shfl((int)base, __ffsll((long long)mask) - 1);
  if (keep)
  {
    uint32_t const at = base + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
    hits[1 + 2 * (size_t)at] = (uint32_t)i;
    hits[2 + 2 * (size_t)at] = __float_as_uint(lrt);
  }
}

hipError_t dcp_launch_lrt_filter(float const *out, int n, uint32_t *hits, hipStream_t stream)
{
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(dcp_lrt_filter_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, out, n, hits);
  return hipGetLastError();
}

// Packs the steps of all windows back to back (window i: compact_off[i] .. compact_off[i+1])
// so that one small D2H copy carries every path: the per-window buffers are sized for the
// worst case and mostly empty.
__global__ void dcp_compact_steps_kernel(uint32_t const *__restrict__ steps, int64_t const *__restrict__ step_off,
                                         int64_t const *__restrict__ compact_off, uint32_t *__restrict__ out, int n)
{
  int const i = (int)blockIdx.x;
  if (i >= n) return;
  int64_t const count = compact_off[i + 1] - compact_off[i];
  uint32_t const *src = steps + step_off[i + 1] - count; // the steps end at the buffer's end
  uint32_t *dst = out + compact_off[i];
  for (int64_t j = threadIdx.x; j < count; j += blockDim.x) dst[j] = src[j];
}

hipError_t dcp_launch_compact_steps(uint32_t const *steps, int64_t const *step_off, int64_t const *compact_off,
                                    uint32_t *out, int n, hipStream_t stream)
{
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(dcp_compact_steps_kernel, dim3((unsigned)n), dim3(256), 0, stream, steps, step_off, compact_off,
                     out, n);
  return hipGetLastError();
}

hipError_t dcp_launch_unzip(DcpLaunch const &a, uint32_t *steps, int64_t const *step_off, int32_t *nsteps)
{
  if (a.nprob <= 0) return hipSuccess;
  unsigned const blocks = (unsigned)((a.nprob + 63) / 64);
  hipLaunchKernelGGL(dcp_unzip_kernel, dim3(blocks), dim3(64), 0, a.stream, a.profiles, a.problems, a.arena, steps,
                     step_off, nsteps, a.nprob);
  return hipGetLastError();
}

// Workgroups of dcp_cost_kernel<Q, W> that one XCD holds at the occupancy the kernel was compiled for (asked of the
// runtime once per kernel and device: registers and LDS decide it, not the launch bounds alone)
template <int Q, int W, int POLICY, int WAVES> static hipError_t cost_resident_per_xcd(int *resident)
{
  static thread_local int cached_dev = -1, cached = 0;
  int dev = 0, per_cu = 0, cus = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  if (dev != cached_dev)
  {
    if ((e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, dcp_cost_kernel<Q, W, POLICY, WAVES>, 64 * W, 0)) != hipSuccess)
      return e;
    if ((e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev)) != hipSuccess) return e;
    cached = per_cu * cus / DCP_NUM_XCDS;
    cached_dev = dev;
  }
  *resident = cached;
  return hipSuccess;
}

template <int Q, int W, int POLICY = DCP_COST_POLICY(Q, W), int WAVES = DCP_COST_WAVES(Q, W)>
static hipError_t launch_cost_qw(DcpLaunch const &a)
{
  int place = a.placement;
  if (place == DCP_PLACE_AUTO)
  {
    // the rows the kernel reads: the first 64 Q W columns behind the header, of each of the 1364 codes
    long long const table_bytes = (long long)DCP_TABLE_SIZE * (64 * Q * W + DCP_ROW_HDR) * 4;
    int resident = 0;
    hipError_t const e = cost_resident_per_xcd<Q, W, POLICY, WAVES>(&resident);
    if (e != hipSuccess) return e;
    place = dcp_xcd_placement(a.nprob, a.windows_per_profile, table_bytes, resident);
  }
  hipLaunchKernelGGL((dcp_cost_kernel<Q, W, POLICY, WAVES>), dim3((unsigned)a.nprob), dim3(64 * W), 0, a.stream, a.pool,
                     a.profiles, a.problems, a.code_rows, a.xt_table, a.out, a.nprob, place == DCP_PLACE_EIGHTHS ? 1 : 0);
  return hipGetLastError();
}

// ---- the kernel classes below the strip class, each written once: class, (Q, W) of the cost kernels (cost, cost +
// checkpoints, cost + store, blocked path), (Q, W) of the pass-by-pass path kernel on the same padded layout ----
// Classes 0..3 are one wavefront of 1..4 positions per lane.  The cost kernels run the padded sizes 384 .. 4096 with 6
// or 8 positions per lane, which halves or quarters the wavefronts that meet at the row barrier; 8 per lane fits 256
// VGPRs (two waves per SIMD) only with the transition arrays parked in LDS between their uses (CostWave::STASH).
// Measured against the 3/4-per-lane shapes on Pfam-structured tables: K=384 639 -> 857 GCUPS, 512 674 -> 884,
// 768 517 -> 691, 1536 328 -> 593, 2048 427 -> 548, 4096 190 -> 337; (8,2) for 1024 brought nothing over (4,4).  The
// pass-by-pass path kernel keeps at most 4 per lane: (3, 2W) / (4, 2W) where the cost kernels have (6, W) / (8, W).
#define DCP_CLASS_TABLE(X) \
  X(0, 1, 1, 1, 1) \
  X(1, 2, 1, 2, 1) \
  X(2, 3, 1, 3, 1) \
  X(3, 4, 1, 4, 1) \
  X(4, 6, 1, 3, 2) \
  X(5, 8, 1, 4, 2) \
  X(6, 6, 2, 3, 4) \
  X(7, 4, 4, 4, 4) \
  X(8, 6, 4, 3, 8) \
  X(9, 8, 4, 4, 8) \
  X(10, 8, 8, 4, 16)

template <int Q_, int W_> struct ClassShape
{
  static constexpr int Q = Q_, W = W_;
};

// f(cost ClassShape, path ClassShape) of class cls
template <class F> static hipError_t with_class(int cls, F f)
{
  switch (cls)
  {
#define X(cls, Q, W, PQ, PW) \
  case cls: return f(ClassShape<Q, W>{}, ClassShape<PQ, PW>{});
    DCP_CLASS_TABLE(X)
#undef X
  default: return hipErrorInvalidValue;
  }
}
#define X(...) +1
static_assert(0 DCP_CLASS_TABLE(X) == DCP_STRIP_CLASS, "one row of DCP_CLASS_TABLE per class below the strip class");
#undef X

static hipError_t launch_strip(DcpLaunch const &a)
{
  if (!a.ring) return hipErrorInvalidValue;
  unsigned const grid = (unsigned)(a.nprob < DCP_RING_SLOTS ? a.nprob : DCP_RING_SLOTS);
  hipLaunchKernelGGL((dcp_strip_kernel<4, 8>), dim3(grid), dim3(512), 0, a.stream, a.pool,
                     a.profiles, a.problems, a.code_rows, a.xt_table, a.arena, a.ring, a.out, a.nprob);
  return hipGetLastError();
}

int dcp_class_of(int K)
{
  if (K < 1) return -1;
  // classes 0..3: one wave, Q = 1..4.  K = 61..64 take the 128-column layout: the packed cost kernel that runs
  // them (32 lanes x 3 positions, viterbi_pack.h) reads 96 columns of a row
  if (K <= 256) return K > 60 && K <= 64 ? 1 : (K + 63) / 64 - 1;
  // padded sizes 384, 512, 768, 1024, 1536, 2048, 4096 (their kernels: DCP_CLASS_TABLE)
  if (K <= 384) return 4;
  if (K <= 512) return 5;
  if (K <= 768) return 6;
  if (K <= 1024) return 7;
  if (K <= 1536) return 8;
  if (K <= 2048) return 9;
  if (K <= 4096) return 10;
  if (K <= DCP_MAX_CORE_SIZE) return DCP_STRIP_CLASS;
  return -1;
}

void dcp_class_shape(int cls, int *Q, int *W)
{
  *Q = 4, *W = 8; // the strip class: per strip
  (void)with_class(cls, [&](auto cost, auto) { return *Q = cost.Q, *W = cost.W, hipSuccess; });
}

hipError_t dcp_launch_cost(int cls, DcpLaunch const &a)
{
  if (a.nprob <= 0) return hipSuccess;
  if (cls == DCP_STRIP_CLASS) return launch_strip(a);
  return with_class(cls, [&](auto cost, auto) { return launch_cost_qw<decltype(cost)::Q, decltype(cost)::W>(a); });
}

// The classes whose rows are padded to 384, 512 and 768 columns: a profile that fits with one position per lane
// less -- K <= 320 in (5,1) instead of (6,1), K <= 448 in (7,1) instead of (8,1) -- runs that way on the same
// tables (it reads the first 64 Q W columns of a row): a sixth or an eighth fewer instructions per row.  K <= 640 on
// the 768-column layout runs as ONE wavefront of ten positions per lane, (10,1), instead of two of five: no barrier
// and no exchange per row, 325 instead of 2 x 242 VALU instructions (K = 520 / 576 / 640: 530 / 585 / 651 -> 715 /
// 810 / 857 GCUPS).  The engine sorts those windows to the front of their class.
int dcp_class_narrow_limit(int cls) { return cls == 4 ? 320 : cls == 5 ? 448 : cls == 6 ? 640 : 0; }
int dcp_class_narrow_q(int cls) { return cls == 4 ? 5 : cls == 5 ? 7 : cls == 6 ? 10 : 0; }

hipError_t dcp_launch_cost_narrow(int cls, DcpLaunch const &a)
{
  if (a.nprob <= 0) return hipSuccess;
  switch (dcp_class_narrow_q(cls))
  {
  case 5: return launch_cost_qw<5, 1>(a);
  case 7: return launch_cost_qw<7, 1>(a);
  case 10: return launch_cost_qw<10, 1>(a); // one wavefront on the two-wave layout
  default: return hipErrorInvalidValue;
  }
}

hipError_t dcp_launch_cost_store(int cls, DcpLaunch const &a, int64_t const *ckpt_addr, int B, int G, int it)
{
  if (a.nprob <= 0) return hipSuccess;
  if (!ckpt_addr || B < 0 || B % 5 || G < 1 || it < 0) return hipErrorInvalidValue;
  return with_class(cls, [&](auto cost, auto) { // (the strip class: dcp_launch_strip_store)
    using C = decltype(cost);
    hipLaunchKernelGGL((dcp_cost_store_kernel<C::Q, C::W>), dim3((unsigned)a.nprob * (unsigned)G), dim3(64 * C::W), 0,
                       a.stream, a.pool, a.profiles, a.problems, a.code_rows, a.xt_table, a.arena, ckpt_addr, B, G, it, a.out,
                       a.nprob);
    return hipGetLastError();
  });
}

hipError_t dcp_launch_cost_ckpt(int cls, DcpLaunch const &a, int64_t const *ckpt_addr, int B)
{
  if (a.nprob <= 0) return hipSuccess;
  return with_class(cls, [&](auto cost, auto) {
    using C = decltype(cost);
    hipLaunchKernelGGL((dcp_cost_ckpt_kernel<C::Q, C::W>), dim3((unsigned)a.nprob), dim3(64 * C::W), 0, a.stream, a.pool,
                       a.profiles, a.problems, a.code_rows, a.xt_table, ckpt_addr, B, a.out, a.nprob);
    return hipGetLastError();
  });
}

hipError_t dcp_launch_path_blocks(int cls, DcpLaunch const &a, int64_t const *ckpt_addr, int B, uint32_t *steps,
                                  int64_t const *step_off, int32_t *nsteps, DcpTraceState *states)
{
  if (a.nprob <= 0) return hipSuccess;
  return with_class(cls, [&](auto cost, auto) {
    using C = decltype(cost);
    hipLaunchKernelGGL((dcp_path_blocks_kernel<C::Q, C::W>), dim3((unsigned)a.nprob), dim3(64 * C::W), 0, a.stream, a.pool,
                       a.profiles, a.problems, a.code_rows, a.xt_table, ckpt_addr, B, a.out, steps, step_off, nsteps, states,
                       a.nprob);
    return hipGetLastError();
  });
}

hipError_t dcp_launch_strip_ckpt(DcpLaunch const &a, int64_t const *ckpt_addr, int B)
{
  if (a.nprob <= 0) return hipSuccess;
  if (!a.ring || !ckpt_addr || B <= 0 || B % 5) return hipErrorInvalidValue;
  unsigned const grid = (unsigned)(a.nprob < DCP_RING_SLOTS ? a.nprob : DCP_RING_SLOTS);
  hipLaunchKernelGGL((dcp_strip_ckpt_kernel<4, 8>), dim3(grid), dim3(512), 0, a.stream, a.pool, a.profiles, a.problems,
                     a.code_rows, a.xt_table, ckpt_addr, B, a.ring, a.out, a.nprob);
  return hipGetLastError();
}

hipError_t dcp_launch_strip_store(DcpLaunch const &a, int64_t const *ckpt_addr, int B, int G, int it)
{
  if (a.nprob <= 0) return hipSuccess;
  if (!a.ring || !ckpt_addr || B < 0 || B % 5 || G < 1 || it < 0) return hipErrorInvalidValue;
  long long const items = (long long)a.nprob * G;
  unsigned const grid = (unsigned)(items < DCP_RING_SLOTS ? items : DCP_RING_SLOTS);
  hipLaunchKernelGGL((dcp_strip_store_kernel<4, 8>), dim3(grid), dim3(512), 0, a.stream, a.pool, a.profiles, a.problems,
                     a.code_rows, a.xt_table, ckpt_addr, B, G, it, a.ring, a.out, a.nprob);
  return hipGetLastError();
}

hipError_t dcp_launch_traceback(DcpLaunch const &a, uint32_t *steps, int64_t const *step_off, int32_t *nsteps,
                                DcpTraceState *states, int B, int G, int it, int64_t const *ckpt_addr)
{
  if (a.nprob <= 0) return hipSuccess;
  if (G < 1 || it < 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(dcp_traceback_kernel, dim3((unsigned)a.nprob), dim3(64), 0, a.stream, a.pool, a.profiles, a.problems,
                     a.code_rows, a.xt_table, a.arena, steps, step_off, nsteps, states, B, G, it, ckpt_addr, a.nprob);
  return hipGetLastError();
}

// ---- several windows per wavefront: the shapes by core size, each written once ----
// shape, positions per lane Q, lanes per group S, and for the LDS variant the wavefronts per workgroup (as many as the
// registers let a CU hold) and the emission lengths whose rows it keeps in LDS: LDS bytes
#define DCP_PACK_TABLE(X) \
  X(0, 1, 4, 16, 5)   /* 44 KB */ \
  X(1, 2, 4, 16, 5)   /* 65 KB */ \
  X(2, 4, 4, 12, 5)   /* 87 KB */ \
  X(3, 2, 8, 16, 4)   /* 27 KB */ \
  X(4, 4, 8, 12, 4)   /* 44 KB */ \
  X(5, 2, 16, 16, 4)  /* 49 KB */ \
  X(6, 3, 16, 12, 4)  /* 71 KB */ \
  X(7, 4, 16, 12, 4)  /* 87 KB */ \
  X(8, 2, 32, 16, 4)  /* 92 KB */ \
  X(9, 3, 32, 12, 4)  /* 136 KB */ \
  X(10, 4, 32, 8, 3)  /* 43 KB: lengths 1..3 only */

template <int Q_, int S_, int WG_, int NLDS_> struct PackShape
{
  static constexpr int Q = Q_, S = S_, WG = WG_, NLDS = NLDS_;
};

// f(PackShape of `shape`)
template <class F> static hipError_t with_pack_shape(int shape, F f)
{
  switch (shape)
  {
#define X(shape, Q, S, WG, NLDS) \
  case shape: return f(PackShape<Q, S, WG, NLDS>{});
    DCP_PACK_TABLE(X)
#undef X
  default: return hipErrorInvalidValue;
  }
}
#define X(...) +1
static_assert(0 DCP_PACK_TABLE(X) == DCP_NUM_PACK_SHAPES, "one row of DCP_PACK_TABLE per shape");
#undef X

void dcp_pack_shape(int shape, int *Q, int *S)
{
  *Q = *S = 0;
  (void)with_pack_shape(shape, [&](auto p) { return *Q = p.Q, *S = p.S, hipSuccess; });
}

int dcp_pack_shape_of(int K)
{
  auto const holds = [K](int shape) {
    int Q, S;
    dcp_pack_shape(shape, &Q, &S);
    return K <= (S - 1) * Q;
  };
  // DECIPHON_HIP_PACK_PREFER=<shape>: that shape for every profile it holds (throughput experiments)
  static int const prefer = getenv("DECIPHON_HIP_PACK_PREFER") ? atoi(getenv("DECIPHON_HIP_PACK_PREFER")) : -1;
  if (prefer >= 0 && prefer < DCP_NUM_PACK_SHAPES && holds(prefer)) return prefer;
  for (int i = 0; i < DCP_NUM_PACK_SHAPES; ++i)
    if (holds(i)) return i; // the first that holds it costs the fewest instructions per cell
  return -1;
}

hipError_t dcp_launch_cost_pack(int shape, DcpLaunch const &a, DcpPack const *packs, int npack, uint32_t ncode_rows)
{
  if (npack <= 0) return hipSuccess;
  return with_pack_shape(shape, [&](auto p) {
    using P = decltype(p);
    hipLaunchKernelGGL((dcp_cost_pack_kernel<P::Q, P::S>), dim3((unsigned)npack), dim3(64), 0, a.stream, a.pool, a.profiles,
                       packs, a.code_rows, ncode_rows, a.xt_table, a.out, npack);
    return hipGetLastError();
  });
}

// Groups of 32 lanes keep every row in L2: two rows per load are not what binds them, and the LDS variants measured
// 3-5 % slower there (K = 93: 711 against 745 GCUPS) while groups of 8 and 16 gained up to 27 % (K = 28: 580 -> 737).
int dcp_pack_lds_waves(int shape)
{
  int waves = 0;
  (void)with_pack_shape(shape, [&](auto p) { return waves = p.S < 32 ? p.WG : 0, hipSuccess; });
  return waves;
}

hipError_t dcp_launch_cost_pack_lds(int shape, DcpLaunch const &a, DcpPack const *packs, int2 const *groups, int ngroups,
                                    uint32_t ncode_rows)
{
  if (ngroups <= 0) return hipSuccess;
  return with_pack_shape(shape, [&](auto p) {
    using P = decltype(p);
    hipLaunchKernelGGL((dcp_cost_pack_lds_kernel<P::Q, P::S, P::WG, P::NLDS>), dim3((unsigned)ngroups), dim3(64 * P::WG), 0,
                       a.stream, a.pool, a.profiles, packs, groups, a.code_rows, ncode_rows, a.xt_table, a.out, ngroups);
    return hipGetLastError();
  });
}

hipError_t dcp_launch_cost_fused(DcpLaunch const &a)
{
  if (a.nprob <= 0) return hipSuccess;
  hipLaunchKernelGGL(dcp_cost_kernel_fused, dim3((unsigned)a.nprob), dim3(64), 0, a.stream, a.pool, a.profiles,
                     a.problems, a.code_rows, a.xt_table, a.out, a.nprob);
  return hipGetLastError();
}

hipError_t dcp_launch_path(int cls, DcpLaunch const &a)
{
  if (a.nprob <= 0) return hipSuccess;
  return with_class(cls, [&](auto, auto path) {
    using P = decltype(path);
    hipLaunchKernelGGL((dcp_path_kernel<P::Q, P::W>), dim3((unsigned)a.nprob), dim3(64 * P::W), 0, a.stream, a.pool,
                       a.profiles, a.problems, a.code_rows, a.xt_table, a.arena, a.out, a.nprob);
    return hipGetLastError();
  });
}
