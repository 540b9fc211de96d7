// scan_walk.cpp -- see scan_walk.h
#include "scan_walk.h"
#include "dcp_errors.h"
#include <algorithm>

namespace
{
void make_chain(int seq_size, int core_size, std::vector<std::pair<int, int>> &c)
{
  c.clear();
  DcpWindow w(seq_size, core_size);
  while (w.next()) c.emplace_back(w.start, w.stop);
}
} // namespace

DcpScanWalk::DcpScanWalk(int nprof, int32_t const *core_sizes, int nreads, int32_t const *read_lengths)
    : K_(core_sizes, core_sizes + std::max(nprof, 0)), len_(read_lengths, read_lengths + std::max(nreads, 0))
{
}

int DcpScanWalk::chunk_windows(DcpChunk const &chunk, dcp_hip_window *wins, int64_t *base)
{
  int64_t n = 0;
  for (int p = chunk.p0; p < chunk.p1; ++p)
  {
    int last_len = -1;
    Chain const *ch = nullptr; // reads of one length follow each other more often than not
    chains_of_profile_.clear();
    for (int s = chunk.s0; s < chunk.s1; ++s)
    {
      int const len = len_[(size_t)s];
      if (len != last_len)
      {
        ch = nullptr;
        if (len > 0)
        {
          auto it = chains_of_profile_.find(len);
          if (it == chains_of_profile_.end())
          {
            it = chains_of_profile_.emplace(len, Chain()).first;
            make_chain(len, K_[(size_t)p], it->second);
          }
          ch = &it->second;
        }
        last_len = len;
      }
      *base++ = n;
      if (ch)
      {
        if ((int64_t)ch->size() > chunk.windows - n) return DCP_EFUNCUSE;
        dcp_hip_window *w = wins + n;
        for (std::pair<int, int> const &r : *ch) *w++ = dcp_hip_window{p, s, r.first, r.second};
        n += (int64_t)ch->size();
      }
    }
  }
  *base = n;
  return n == chunk.windows ? 0 : DCP_EFUNCUSE;
}

void DcpScanWalk::chunk_scored(DcpChunk const &chunk, int64_t const *base, int nh, int32_t const *hit_index,
                               float const *lrts)
{
  int const ns = chunk.s1 - chunk.s0;
  int64_t const *base_end = base + (size_t)(chunk.p1 - chunk.p0) * (size_t)ns + 1;
  int64_t speculated_of_hit_pairs = 0;
  size_t const first_new = st_.size();
  size_t last_pi = (size_t)-1;
  for (int h = 0; h < nh; ++h) // hit_index ascends: the hits of a pair are neighbours
  {
    int64_t const wi = hit_index[h];
    size_t const pi = (size_t)(std::upper_bound(base, base_end, wi) - base) - 1;
    if (pi != last_pi) // a pair's first hit: its chain and the (so far hit-less) scores of the chain's windows
    {
      last_pi = pi;
      int const p = chunk.p0 + (int)(pi / (size_t)ns), sq = chunk.s0 + (int)(pi % (size_t)ns);
      int const len = len_[(size_t)sq], K = K_[(size_t)p];
      kept_chains_.emplace_back();
      make_chain(len, K, kept_chains_.back());
      kept_lrt_.emplace_back((size_t)(base[pi + 1] - base[pi]), -1.0f);
      st_.push_back(PairState{p, sq, DcpWindow(len, K), &kept_chains_.back(), kept_lrt_.back().data()});
      speculated_of_hit_pairs += base[pi + 1] - base[pi];
    }
    kept_lrt_.back()[(size_t)(wi - base[pi])] = lrts[h];
  }
  nwindows_ += (size_t)(base_end[-1] - speculated_of_hit_pairs); // the windows of the pairs without a hit are final
  for (size_t i = first_new; i < st_.size(); ++i) advance(i);
}

void DcpScanWalk::all_pairs()
{
  for (int p = 0; p < (int)K_.size(); ++p)
    for (int s = 0; s < (int)len_.size(); ++s)
      if (len_[(size_t)s] > 0)
        st_.push_back(PairState{p, s, DcpWindow(len_[(size_t)s], K_[(size_t)p]), nullptr, nullptr});
  for (size_t i = 0; i < st_.size(); ++i) advance(i);
}

// moves a pair to its next window that needs work: a path pass (a speculated window that passed the filter) or a
// cost pass (a window nobody has scored); nothing when its chain has ended
void DcpScanWalk::advance(size_t i)
{
  PairState &ps = st_[i];
  while (ps.win.next())
  {
    ++nwindows_;
    dcp_hip_window const w{ps.profile, ps.seq, ps.win.start, ps.win.stop};
    bool const as_speculated = ps.spec && (size_t)ps.win.idx < ps.spec->size() &&
                               (*ps.spec)[(size_t)ps.win.idx] == std::make_pair(ps.win.start, ps.win.stop);
    if (!as_speculated)
    {
      ++queued_;
      need_cost_.push_back(Work{i, w, 0.0f});
      return;
    }
    float const lrt = ps.spec_lrt[ps.win.idx];
    if (lrt >= 0.0f)
    {
      need_path_.push_back(Work{i, w, lrt});
      return;
    }
  }
}

std::vector<dcp_hip_window> const &DcpScanWalk::take(std::vector<Work> &from, std::vector<Work> &taken)
{
  taken.clear();
  taken.swap(from);
  taken_wins_.resize(taken.size());
  for (size_t k = 0; k < taken.size(); ++k) taken_wins_[k] = taken[k].w;
  return taken_wins_;
}

std::vector<dcp_hip_window> const &DcpScanWalk::take_cost_round() { return take(need_cost_, cost_taken_); }
std::vector<dcp_hip_window> const &DcpScanWalk::take_path_batch() { return take(need_path_, path_taken_); }

void DcpScanWalk::cost_scored(int nh, int32_t const *hit_index, float const *lrts)
{
  std::vector<char> is_hit(cost_taken_.size(), 0);
  for (int h = 0; h < nh; ++h)
  {
    size_t const k = (size_t)hit_index[h];
    is_hit[k] = 1;
    need_path_.push_back(Work{cost_taken_[k].pair, cost_taken_[k].w, lrts[h]});
  }
  for (size_t k = 0; k < cost_taken_.size(); ++k)
    if (!is_hit[k]) advance(cost_taken_[k].pair);
  cost_taken_.clear();
}

std::vector<dcp_walk_hit> const &DcpScanWalk::path_walked(uint8_t const *is_hit, int32_t const *last_hit_pos)
{
  hits_.clear();
  for (size_t k = 0; k < path_taken_.size(); ++k)
  {
    if (!is_hit[k]) continue;
    PairState &ps = st_[path_taken_[k].pair];
    ps.win.last_hit_pos = last_hit_pos[k];
    hits_.push_back(dcp_walk_hit{(int32_t)k, ps.profile, ps.seq, ps.win.idx, ps.win.start, ps.win.stop, path_taken_[k].lrt});
  }
  for (Work const &wk : path_taken_) advance(wk.pair);
  path_taken_.clear();
  return hits_;
}
