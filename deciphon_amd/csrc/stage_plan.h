// stage_plan.h -- the plan of a window list: which windows are refused, the problems they become, where their
// trellises or tables lie, which leave the problem list for the packs of the short profiles, how packs share LDS
// workgroups, the order of both lists and whose share of them is whose; and, from those shares, the launches of a cost
// pass.  Host only: no GPU, no engine, no environment -- engine.cpp reads DECIPHON_HIP_PACK, _PACK_LDS and _NARROW
// on every call and passes the values in, with the tables of the kernels (viterbi_kernels.h) as plain numbers.
#pragma once
#include "../../include/deciphon_hip.h"
#include "dcp_errors.h"
#include "dcp_types.h"
#include "path_plan.h"
#include <stddef.h>
#include <vector>

namespace dcp_engine
{

// what the plan needs of a profile: core size, padded size, kernel class (outside 0 .. DCP_NUM_CLASSES - 1: none),
// shape of the packed cost kernel (-1: none), and whether it fits its class with one position per lane less
struct StageProfile
{
  int K = 0, Kp = 0, cls = -1;
  int pack = -1;
  bool narrow = false;
};

// a pack shape (viterbi_pack.h): windows that share a wavefront, 64 / S, and the wavefronts of a workgroup that shares
// a profile's table in LDS (dcp_pack_lds_waves; 0: the shape reads every row from global memory)
struct StageShape
{
  int windows, lds_waves;
};

enum ArenaKind { ARENA_NONE, ARENA_TRELLIS, ARENA_TABLE };

// trellis of one window: uint32 xnodes[L+1], uint16 nodes[(L+1)][K] (c-core/trellis.h:12-21); in the arena of a staged
// list (ARENA_TRELLIS) the windows follow each other in the order given, each from a multiple of 16 bytes
inline size_t trellis_bytes(int L, int K) { return ((size_t)L + 1) * 4 + ((size_t)L + 1) * (size_t)K * 2; }
inline size_t trellis_stride(int L, int K) { return (trellis_bytes(L, K) + 15) & ~(size_t)15; }
// that layout, for windows that passed check_window: off[i] = where window i's trellis starts, off[n] = the arena's bytes
std::vector<size_t> trellis_offsets(int n, dcp_hip_window const *w, StageProfile const *profiles);

// {first pack, count} of a workgroup of the LDS pack kernels, counted from the shape's first pack (int2 on the device)
struct PackGroup
{
  int32_t first, count;
};

// what the launch functions need of a staged window list: whose share of the lists on the device is whose
struct StagedPlan
{
  int c_begin[DCP_NUM_CLASSES + 1] = {0}; // problems of class c are [c_begin[c], c_begin[c+1])
  int c_wide[DCP_NUM_CLASSES] = {0};      // ... the narrow profiles' first: [c_begin[c], c_wide[c])
  int c_profiles[DCP_NUM_CLASSES][2] = {{0}}; // profiles with a window among the narrow ones, and among the rest
  int pk_begin[DCP_NUM_PACK_SHAPES + 1] = {0};
  int pg_begin[DCP_NUM_PACK_SHAPES + 1] = {0};
  double cells = 0;
};

struct Staged : StagedPlan
{
  std::vector<DcpProblem> problems;   // sorted by (class, narrow first, profile); cost pass: without the packed ones
  std::vector<DcpPack> packs;         // cost pass: sorted by (shape, profile), pk_begin[s] = the first of shape s
  std::vector<PackGroup> pack_groups; // shapes with an LDS variant: one per workgroup, from pg_begin[s]
  size_t arena_bytes = 0;
  int max_xt_row = 1; // the largest DcpProblem::xt_row of the list
  Staged() = default;
  Staged(Staged const &) = delete;
  Staged &operator=(Staged const &) = delete;
};

// why a window list is refused: a DCP_E* code and the engine's message; code 0: it is not
struct Refusal
{
  int code = 0;
  char const *what = nullptr;
};

// profile index, sequence index, range -- in that order, the first that fails.  seq_off[nseq + 1]: the reads' offsets.
inline Refusal check_window(dcp_hip_window const &w, int nprofiles, int nseq, int64_t const *seq_off)
{
  if (w.profile < 0 || w.profile >= nprofiles) return {DCP_EFUNCUSE, "bad profile index"};
  if (w.seq < 0 || w.seq >= nseq) return {DCP_EFUNCUSE, "bad sequence index"};
  if (w.start < 0 || w.stop < w.start || w.stop > seq_off[w.seq + 1] - seq_off[w.seq]) return {DCP_EFUNCUSE, "bad window range"};
  return {};
}

struct StageInput
{
  int n;
  dcp_hip_window const *w;
  StageProfile const *profiles; // [nprofiles]
  int nprofiles;
  int nseq;
  int64_t const *seq_off, *row_off; // [nseq + 1]: nucleotides and code rows in front of each read, and in all
  ArenaKind arena;
  int64_t const *table_addr;        // ARENA_TABLE: per window, the device address of its DP table
  bool pack, pack_lds;              // DECIPHON_HIP_PACK, DECIPHON_HIP_PACK_LDS
  StageShape const *shapes;         // [DCP_NUM_PACK_SHAPES]
};

// The plan.  A list is refused for its first offending window (check_window, then DCP_EZEROSEQ for an empty one), a
// list whose windows all pass for a profile outside every kernel class (DCP_ELARGECORESIZE); st is then of no use.
// Windows of profiles with a pack shape are packed when in.pack, no arena is asked for and the code rows stay below
// 2^32 (a pack addresses them by u32 index).
Refusal plan_stage(StageInput const &in, Staged &st);

// ---- the launches of a cost pass over a staged list, in launch order ----
enum CostKernel
{
  COST_NONE,    // nothing: a class whose windows all went to its narrow kernel still has its branch entered and left
  COST_CLASS,   // dcp_launch_cost(index, ..) over problems [first, first + count)
  COST_NARROW,  // dcp_launch_cost_narrow(index, ..) over problems [first, first + count)
  COST_FUSED,   // dcp_launch_cost_fused over the problems of classes 0..3
  COST_PACK,    // dcp_launch_cost_pack(index, ..) over packs [first, first + count)
  COST_PACK_LDS // dcp_launch_cost_pack_lds(index, ..) over groups [first, first + count), packs from pk_begin[index]
};
enum CostBranch { BRANCH_CLASS, BRANCH_NARROW, BRANCH_PACK }; // dcp_hip::cls_branch, narrow_branch, pack_branch
struct CostLaunch
{
  int32_t kernel;              // CostKernel
  int32_t index;               // class, or pack shape
  int32_t first, count;        // in the staged list the kernel reads
  int32_t windows_per_profile; // COST_CLASS, COST_NARROW: the mean over the profiles of its windows (0: not known)
  int32_t branch;              // CostBranch; the branch itself is that array's [index]
};
// Classes from the last to the first, a class's narrow part in front of the rest (narrow: DECIPHON_HIP_NARROW; off, the
// class kernel takes all); one fused kernel in place of classes 0..3 when at least two of them are present and hold
// 16384 windows at the most; then the pack shapes from the last to the first.  More than one entry: the pass forks.
std::vector<CostLaunch> cost_schedule(StagedPlan const &st, bool narrow);

} // namespace dcp_engine
