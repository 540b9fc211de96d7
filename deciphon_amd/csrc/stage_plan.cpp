// stage_plan.cpp -- the plan of a window list and the launches of its cost pass (stage_plan.h).
#include "stage_plan.h"

#include <algorithm>
#include <string.h>

namespace dcp_engine
{
namespace
{

// Either list is ordered by one of two algorithms that must agree (tests/test_stage_plan.py holds them to each other):
// a list that comes in ascending profile order -- all a scan ever sends -- by counting passes, which keep staging off
// the scan's critical path; any other by a stable comparison sort.

// v reordered by key(v[i]) in [0, nkeys), equal keys keeping their order: count, prefix, scatter
template <class Key> void bucket_stable(std::vector<DcpProblem> &v, int nkeys, Key key)
{
  std::vector<size_t> at((size_t)nkeys + 1, 0);
  std::vector<unsigned char> k(v.size());
  for (size_t i = 0; i < v.size(); ++i) ++at[(size_t)(k[i] = (unsigned char)key(v[i])) + 1];
  bool one = false;
  for (int j = 0; j < nkeys; ++j)
  {
    one = one || at[(size_t)j + 1] == v.size();
    at[(size_t)j + 1] += at[(size_t)j];
  }
  if (one) return; // a single key: already in order
  std::vector<DcpProblem> out(v.size());
  for (size_t i = 0; i < v.size(); ++i) out[at[k[i]]++] = v[i];
  v.swap(out);
}

// the n problems at p ordered by window length, longest first, equal lengths keeping their order
void longest_first(DcpProblem *p, size_t n)
{
  if (n < 2) return;
  int lens[32];
  int nl = 0;
  bool sorted = true;
  for (size_t i = 0; i < n && nl <= 32; ++i)
  {
    sorted = sorted && (i == 0 || p[i].L <= p[i - 1].L);
    int j = 0;
    while (j < nl && lens[j] != p[i].L) ++j;
    if (j == nl)
    {
      if (nl == 32)
      {
        nl = 33;
        break;
      }
      lens[nl++] = p[i].L;
    }
  }
  if (sorted && nl <= 32) return;
  if (nl > 32)
  {
    std::stable_sort(p, p + n, [](DcpProblem const &a, DcpProblem const &b) { return a.L > b.L; });
    return;
  }
  std::sort(lens, lens + nl, [](int a, int b) { return a > b; });
  size_t at[33] = {0};
  for (size_t i = 0; i < n; ++i)
  {
    int j = 0;
    while (lens[j] != p[i].L) ++j;
    ++at[j + 1];
  }
  for (int j = 0; j < nl; ++j) at[j + 1] += at[j];
  std::vector<DcpProblem> out(n);
  for (size_t i = 0; i < n; ++i)
  {
    int j = 0;
    while (lens[j] != p[i].L) ++j;
    out[at[j]++] = p[i];
  }
  std::copy(out.begin(), out.end(), p);
}

// Cost pass: the windows of short profiles go several to a wavefront (viterbi_pack.h).  They leave the problem list
// and come back as packs: up to StageShape::windows windows of ONE profile each, longest first, so that the windows of a
// pack are of similar length (a pack runs as many rows as its longest window).
void pack_short_profiles(StageInput const &in, bool by_profile, Staged &st)
{
  StageProfile const *const prof = in.profiles;
  std::vector<DcpProblem> packed, rest;
  for (DcpProblem const &p : st.problems) (prof[p.profile].pack >= 0 ? packed : rest).push_back(p);
  if (by_profile)
  {
    // order (shape, profile, longest first) without a comparison sort over everything: a stable scatter by shape
    // keeps the profiles ascending, then each profile's run is ordered by length -- a counting pass when the run
    // holds few distinct lengths (the windows of a chain: whole windows and one tail)
    bucket_stable(packed, DCP_NUM_PACK_SHAPES, [&](DcpProblem const &a) { return prof[a.profile].pack; });
    for (size_t b = 0; b < packed.size();)
    {
      size_t e = b + 1;
      while (e < packed.size() && packed[e].profile == packed[b].profile) ++e;
      longest_first(packed.data() + b, e - b);
      b = e;
    }
  }
  else
    std::stable_sort(packed.begin(), packed.end(), [&](DcpProblem const &a, DcpProblem const &b) {
      int sa = prof[a.profile].pack, sb = prof[b.profile].pack;
      if (sa != sb) return sa < sb;
      if (a.profile != b.profile) return a.profile < b.profile;
      return a.L > b.L;
    });
  int shape = 0;
  for (size_t i = 0; i < packed.size();)
  {
    int const sh = prof[packed[i].profile].pack;
    while (shape < sh) st.pk_begin[++shape] = (int)st.packs.size();
    int const G = in.shapes[sh].windows;
    DcpPack pk;
    memset(&pk, 0, sizeof pk);
    pk.profile = packed[i].profile;
    pk.Lmax = packed[i].L;
    int g = 0;
    for (; g < G && i < packed.size() && packed[i].profile == pk.profile; ++g, ++i)
    {
      pk.L[g] = packed[i].L;
      pk.xt_row[g] = packed[i].xt_row;
      pk.out[g] = packed[i].out;
      pk.code_row[g] = (uint32_t)packed[i].code_row;
    }
    st.packs.push_back(pk);
  }
  while (shape < DCP_NUM_PACK_SHAPES) st.pk_begin[++shape] = (int)st.packs.size();
  st.problems.swap(rest);
  // four-lane groups: the packs of one profile go lds_waves to a workgroup, which shares the profile's table in LDS
  for (int s = 0; s < DCP_NUM_PACK_SHAPES; ++s)
  {
    st.pg_begin[s] = (int)st.pack_groups.size();
    int const wg = in.pack_lds ? in.shapes[s].lds_waves : 0;
    if (!wg) continue;
    for (int i = st.pk_begin[s]; i < st.pk_begin[s + 1];)
    {
      int j = i;
      while (j < st.pk_begin[s + 1] && j - i < wg && st.packs[(size_t)j].profile == st.packs[(size_t)i].profile) ++j;
      st.pack_groups.push_back(PackGroup{i - st.pk_begin[s], j - i});
      i = j;
    }
  }
  st.pg_begin[DCP_NUM_PACK_SHAPES] = (int)st.pack_groups.size();
}

} // namespace

std::vector<size_t> trellis_offsets(int n, dcp_hip_window const *w, StageProfile const *profiles)
{
  std::vector<size_t> off((size_t)std::max(n, 0) + 1, 0);
  for (int i = 0; i < n; ++i) off[(size_t)i + 1] = off[(size_t)i] + trellis_stride(w[i].stop - w[i].start, profiles[w[i].profile].K);
  return off;
}

Refusal plan_stage(StageInput const &in, Staged &st)
{
  int const n = in.n;
  dcp_hip_window const *const w = in.w;
  StageProfile const *const prof = in.profiles;
  static_cast<StagedPlan &>(st) = StagedPlan();
  st.problems.resize((size_t)n);
  st.packs.clear();
  st.pack_groups.clear();
  int64_t const *const seq_off = in.seq_off, *const row_off = in.row_off;
  int const nseq = in.nseq;
  ArenaKind const kind = in.arena;
  int max_xt_row = 1;
  size_t arena = 0;
  bool by_profile = true; // the windows come in ascending profile order (dcp_scan_run's do): no sort needed below
  bool classless = false;
  for (int i = 0; i < n; ++i)
  {
    by_profile = by_profile && (i == 0 || w[i].profile >= w[i - 1].profile);
    Refusal const bad = check_window(w[i], in.nprofiles, nseq, seq_off);
    if (bad.code) return bad;
    int const L = w[i].stop - w[i].start;
    if (L < 1) return {DCP_EZEROSEQ, "empty window"};
    StageProfile const &hp = prof[w[i].profile];
    classless = classless || hp.cls < 0 || hp.cls >= DCP_NUM_CLASSES;
    DcpProblem &p = st.problems[(size_t)i];
    p.profile = w[i].profile;
    p.L = L;
    p.code_row = row_off[w[i].seq] + w[i].start;
    p.xt_row = std::max(L / 3, 1); // c-core/thread.c:112
    p.out = i;
    p.trellis = 0;
    max_xt_row = std::max(max_xt_row, p.xt_row);
    st.cells += (double)hp.K * (double)L;
    if (kind != ARENA_NONE)
    {
      // trellises: offsets into the arena, as trellis_offsets has them; DP tables: addresses the caller placed
      p.trellis = kind == ARENA_TRELLIS ? (int64_t)arena : in.table_addr[i];
      arena += kind == ARENA_TRELLIS ? trellis_stride(L, hp.K) : (dcp_table_bytes(L, hp.Kp) + 15) & ~(size_t)15;
    }
  }
  st.arena_bytes = arena;
  st.max_xt_row = max_xt_row;
  // (no engine describes such a profile: refused here, in front of the orderings that index by class)
  if (classless) return {DCP_ELARGECORESIZE, "profile outside every kernel class"};
  // in.pack off keeps every window on the one-window-per-wavefront kernels (tests compare the two)
  if (in.pack && kind == ARENA_NONE && (uint64_t)row_off[nseq] < ((uint64_t)1 << 32)) // code rows by u32 index
    pack_short_profiles(in, by_profile, st);
  int const nu = (int)st.problems.size(); // windows that keep a wavefront (or a workgroup) to themselves
  // by (class, the narrow profiles of a class first -- one position per lane less: their own launch of the cost pass --,
  // profile)
  if (by_profile)
    bucket_stable(st.problems, 2 * DCP_NUM_CLASSES, [&](DcpProblem const &a) {
      StageProfile const &hp = prof[a.profile];
      return 2 * hp.cls + (hp.narrow ? 0 : 1);
    });
  else
    std::stable_sort(st.problems.begin(), st.problems.end(), [&](DcpProblem const &a, DcpProblem const &b) {
      StageProfile const &pa = prof[a.profile], &pb = prof[b.profile];
      if (pa.cls != pb.cls) return pa.cls < pb.cls;
      if (pa.narrow != pb.narrow) return pa.narrow;
      return a.profile < b.profile;
    });
  int i = 0;
  for (int c = 0; c < DCP_NUM_CLASSES; ++c)
  {
    st.c_begin[c] = i;
    // (the list is in profile order inside either part: a profile is one run of it)
    auto const starts_run = [&](int j) { return j == st.c_begin[c] || st.problems[(size_t)j].profile != st.problems[(size_t)j - 1].profile; };
    while (i < nu && prof[st.problems[(size_t)i].profile].cls == c && prof[st.problems[(size_t)i].profile].narrow)
      st.c_profiles[c][0] += starts_run(i), ++i;
    st.c_wide[c] = i;
    while (i < nu && prof[st.problems[(size_t)i].profile].cls == c) st.c_profiles[c][1] += starts_run(i), ++i;
  }
  st.c_begin[DCP_NUM_CLASSES] = i;
  return {};
}

// Launch order = start order (the hardware runs a few queues side by side and takes kernels as they come):
// the classes with the fewest, longest-running workgroups go first -- multi-wave groups, then 8, 6, 4, 3
// positions per lane -- and the packed kernels with their many short wavefronts last, where they fill what
// the tails of the others leave idle.  (The other way round the K > 384 classes ran alone at the end of a
// Pfam-shaped step: 33 + 50 ms of 456, profiles/r02_b.)
// Of the one-window kernels, a small launch that mixes single-wave classes goes out as ONE fused kernel (classes 0..3
// are contiguous in the sorted problem list); large launches keep one kernel per class, which fills the GPU by itself
// and has its own register budget.
std::vector<CostLaunch> cost_schedule(StagedPlan const &st, bool narrow)
{
  std::vector<CostLaunch> s;
  auto const per_profile = [](int windows, int profiles) { return profiles > 0 ? windows / profiles : 0; };
  int const single_wave = st.c_begin[4] - st.c_begin[0];
  int mixed = 0;
  for (int c = 0; c < 4; ++c) mixed += st.c_begin[c + 1] > st.c_begin[c];
  bool const fused = mixed >= 2 && single_wave <= 16384;
  for (int c = DCP_NUM_CLASSES - 1; c >= (fused ? 4 : 0); --c)
  {
    int const all = st.c_begin[c + 1] - st.c_begin[c];
    if (all <= 0) continue;
    // the windows that fit with one position per lane less (dcp_class_narrow_limit) lead the class's list and have
    // their own kernel, on its own stream
    int const nn = narrow ? st.c_wide[c] - st.c_begin[c] : 0;
    if (nn > 0) s.push_back({COST_NARROW, c, st.c_begin[c], nn, per_profile(nn, st.c_profiles[c][0]), BRANCH_NARROW});
    // the rest in one launch; with no narrow kernel (or none wanted) that is all of them: both parts' profiles
    int const np = st.c_profiles[c][1] + (nn > 0 ? 0 : st.c_profiles[c][0]);
    s.push_back({all > nn ? COST_CLASS : COST_NONE, c, st.c_begin[c] + nn, all - nn, per_profile(all - nn, np), BRANCH_CLASS});
  }
  if (fused) s.push_back({COST_FUSED, 0, st.c_begin[0], single_wave, 0, BRANCH_CLASS});
  for (int p = DCP_NUM_PACK_SHAPES - 1; p >= 0; --p)
  {
    int const np = st.pk_begin[p + 1] - st.pk_begin[p], ng = st.pg_begin[p + 1] - st.pg_begin[p];
    if (np <= 0) continue;
    if (ng > 0) s.push_back({COST_PACK_LDS, p, st.pg_begin[p], ng, 0, BRANCH_PACK});
    else s.push_back({COST_PACK, p, st.pk_begin[p], np, 0, BRANCH_PACK});
  }
  return s;
}

} // namespace dcp_engine
