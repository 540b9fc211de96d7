// scan_walk.h -- the window walk of dcp_scan_run: which windows of which (profile, read) pairs are scored, kept or
// scored again.  Host only: no GPU, no engine, no environment.
//
// Windows of ONE (profile, read) pair form a chain -- where window w + 1 starts depends on the hit of window w
// (c-core/window.c:21-31, c-core/thread.c:162) -- but hits are rare, and while a pair has had none its chain is the
// same for every pair with that read length and core size.  So the pairs are scored SPECULATIVELY, chunk by chunk
// (dcp_plan_chunks): every window of every pair's no-hit chain (chunk_windows), cost pass + LRT filter on the device
// (c-core/thread.c:114-121).  Pairs of which no window passes the filter are done (chunk_scored).  The windows that
// passed go through the path pass (c-core/thread.c:123-166) in batches (take_path_batch / path_walked); a pair with a
// hit then walks its real chain, and last_hit_pos is sticky: the chain leaves the speculated one and may rejoin it.
// While the windows that follow a hit are still the speculated ones of the same index their scores stand; otherwise
// they are scored again in rounds (take_cost_round / cost_scored).  With nothing speculated (all_pairs) every pair goes
// round by round.
//
// Invariants:
//  * A pair's chain is never split across chunks (dcp_plan_chunks): when a pair hits, the speculated scores of all
//    its windows are in that chunk's results.
//  * kept_chains_ and kept_lrt_ are deques that only grow: a PairState points into their elements (spec, spec_lrt)
//    for the rest of the scan, so their elements must never move.  st_ only grows too, but the queued work names its
//    pairs by index: it is a deque merely so that growing it copies no PairState.
//  * Between take_X and X_scored / X_walked the batch taken belongs to the caller's GPU call; the walk may be asked
//    for the windows of further chunks meanwhile, and two chunks may be outstanding (their window lists and base
//    offsets are the caller's).
#pragma once
#include "../../include/deciphon_hip.h"
#include "../../include/deciphon_host.h"
#include "host_logic.h"
#include <deque>
#include <map>
#include <utility>
#include <vector>

class DcpScanWalk
{
public:
  DcpScanWalk(int nprof, int32_t const *core_sizes, int nreads, int32_t const *read_lengths);

  // The windows of a chunk, pair by pair in (profile, read) order: wins[chunk.windows], and base[pairs + 1], the first
  // window of pair (p - p0) * (s1 - s0) + (s - s0).  DCP_EFUNCUSE when the plan's count is not the chains'.
  int chunk_windows(DcpChunk const &chunk, dcp_hip_window *wins, int64_t *base);
  // The filter's verdict on those windows: nh of them passed, hit_index ascending.  The pairs that hit keep their
  // chain and its speculated scores and move to their first window that needs work; all other windows are final.
  void chunk_scored(DcpChunk const &chunk, int64_t const *base, int nh, int32_t const *hit_index, float const *lrts);
  // nothing speculated: every pair with a non-empty read starts its chain
  void all_pairs();

  size_t cost_waiting() const { return need_cost_.size(); }
  size_t path_waiting() const { return need_path_.size(); }
  // windows nobody has scored yet (c-core/thread.c:114-121); those that pass wait for a path pass, the others' pairs move on
  std::vector<dcp_hip_window> const &take_cost_round();
  void cost_scored(int nh, int32_t const *hit_index, float const *lrts);
  // windows that passed the filter.  path_walked: per window of the batch whether its path holds a hit, and that
  // hit's last_hit_pos (window_set_last_hit_position, c-core/thread.c:162).  Returns the hits as they stand before
  // their pairs move on, in batch order; then every pair of the batch moves on.
  std::vector<dcp_hip_window> const &take_path_batch();
  std::vector<dcp_walk_hit> const &path_walked(uint8_t const *is_hit, int32_t const *last_hit_pos);

  size_t windows_walked() const { return nwindows_; }
  // windows queued for a cost round since the last call: one progress callback each (c-core/thread.c:74)
  size_t take_queued() { return std::exchange(queued_, 0); }

private:
  typedef std::vector<std::pair<int, int>> Chain; // [start, stop) of the windows of a pair that never hits
  struct PairState
  {
    int profile, seq;
    DcpWindow win;
    Chain const *spec;     // the speculated chain, nullptr: nothing speculated
    float const *spec_lrt; // ... and per window of it: its lrt when it passed the filter, -1 otherwise
  };
  struct Work
  {
    size_t pair;
    dcp_hip_window w;
    float lrt;
  };
  void advance(size_t pair);
  std::vector<dcp_hip_window> const &take(std::vector<Work> &from, std::vector<Work> &taken);

  std::vector<int32_t> K_, len_;
  // The chains of ONE profile by read length, made as the reads ask for them and dropped with the profile: reads of a
  // batch often share a length (then this is one chain per profile), but real reads need not -- a cache over all
  // (length, core size) pairs of a Pfam-sized scan of 1e4 reads of 1e4 lengths would hold 2e8 chains.
  std::map<int, Chain> chains_of_profile_;
  std::deque<PairState> st_;                // pairs that need more than their speculated scores
  std::deque<Chain> kept_chains_;           // their chains (PairState::spec) ...
  std::deque<std::vector<float>> kept_lrt_; // ... and the speculated lrt of the chains' windows (PairState::spec_lrt)
  std::vector<Work> need_cost_, need_path_, cost_taken_, path_taken_; // waiting, and with the caller's GPU call
  std::vector<dcp_hip_window> taken_wins_;                            // the windows of the batch taken last
  std::vector<dcp_walk_hit> hits_;
  size_t nwindows_ = 0, queued_ = 0;
};
