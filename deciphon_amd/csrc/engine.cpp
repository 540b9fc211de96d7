// engine.cpp -- device-resident state and the C ABI of include/deciphon_hip.h: the engine itself, its sequences and
// mode, staging and launching of window lists.  Profiles: engine_profiles.cpp, engine_hmm.cpp; cost passes: engine_cost.cpp; path pass:
// engine_path.cpp; the state they share: engine_internal.h.
//
// HBM layout (one engine = one GPU):
//   pool      float[]          all profiles back to back; per profile
//                              rows[1364][4+Kp] = {null, bg, 0, 0, match[0..Kp)} | trans[8][Kp],
//                              Kp = 64*Q*W, padding = +inf (DcpProfileDev holds the offsets)
//   profiles  DcpProfileDev[]
//   code_rows DcpCodeRow[]     per sequence len+1 rows of 32 B (built on the GPU
//                              from 1 B/nt by dcp_encode_kernel)
//   xt_table  float[S+1][16]   special transitions per amino length S (host-computed:
//                              they need double-precision log, c-core/xtrans.c:26-45)
//   problems  DcpProblem[]     sorted by (Q, profile) so that neighbouring
//                              workgroups hit the same emission table in L2
//   out       float[]          (null, alt) per window
//   arena     bytes            trellises of the path pass
#include "engine_internal.h"

namespace dcp_engine
{
namespace
{

int ensure_xt(dcp_hip *x, int rows_needed)
{
  if (!x->mode_set) return fail(x, DCP_EFUNCUSE, "dcp_hip_set_mode has not been called");
  if (rows_needed <= x->xt_rows) return 0;
  // a window of the scan has at most 100 000 nucleotides (c-core/window.c:13), i.e. 33 333 amino acids: one table
  // covers them all, so that the table is never replaced while kernels that read it are in flight
  int rows = std::max(rows_needed, 33336);
  std::vector<float> tab((size_t)rows * DCP_XT_STRIDE, 0.0f);
  for (int s = 1; s < rows; ++s) dcp_xtrans(s, x->multi_hits, x->hmmer3_compat, tab.data() + (size_t)s * DCP_XT_STRIDE);
  if (!x->xt_override.empty())
    memcpy(tab.data(), x->xt_override.data(), std::min(tab.size(), x->xt_override.size()) * sizeof(float));
  HIP_TRY(x, hipDeviceSynchronize(), DCP_EFUNCUSE); // nothing may still be reading the old table
  HIP_TRY(x, x->d_xt.reserve(tab.size()), DCP_ENOMEM);
  HIP_TRY(x, hipMemcpy(x->d_xt.p, tab.data(), tab.size() * sizeof(float), hipMemcpyHostToDevice), DCP_EFUNCUSE);
  x->xt_rows = rows;
  return 0;
}

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

// a staged list goes up from pinned memory (see dcp_hip::Bank); dev has been reserved
template <class T> int upload(dcp_hip *x, DevBuf<T> &dev, PinBuf<T> &pinned, std::vector<T> const &v, hipStream_t stream)
{
  if (v.empty()) return 0;
  HIP_TRY(x, pinned.reserve(v.size()), DCP_ENOMEM);
  memcpy(pinned.p, v.data(), v.size() * sizeof(T));
  HIP_TRY(x, hipMemcpyAsync(dev.p, pinned.p, v.size() * sizeof(T), hipMemcpyHostToDevice, stream), DCP_EFUNCUSE);
  return 0;
}

} // namespace

int stage(dcp_hip *x, int n, dcp_hip_window const *w, ArenaKind arena_kind, Staged &st, hipStream_t origin)
{
  if (!origin) origin = x->stream;
  if (n < 0 || (n > 0 && !w)) return fail(x, DCP_EFUNCUSE, "bad window array");
  if (BK(x).n >= 0) return fail(x, DCP_EFUNCUSE, "a dcp_hip_cost_hits_begin is outstanding on these buffers: call dcp_hip_cost_hits_end first");
  if (x->committed != x->profiles.size()) return fail(x, DCP_EFUNCUSE, "profiles not committed");
  int const nseq = (int)x->seq_off.size() - 1;
  int max_s = 1;
  st.problems.resize((size_t)n);
  size_t arena = 0;
  bool by_profile = true; // the windows come in ascending profile order (dcp_scan_run's do): no sort needed below
  for (int i = 0; i < n; ++i)
  {
    by_profile = by_profile && (i == 0 || w[i].profile >= w[i - 1].profile);
    if (w[i].profile < 0 || w[i].profile >= (int)x->profiles.size()) return fail(x, DCP_EFUNCUSE, "bad profile index");
    if (w[i].seq < 0 || w[i].seq >= nseq) return fail(x, DCP_EFUNCUSE, "bad sequence index");
    int64_t const len = x->seq_off[(size_t)w[i].seq + 1] - x->seq_off[(size_t)w[i].seq];
    if (w[i].start < 0 || w[i].stop < w[i].start || w[i].stop > len) return fail(x, DCP_EFUNCUSE, "bad window range");
    int const L = w[i].stop - w[i].start;
    if (L < 1) return fail(x, DCP_EZEROSEQ, "empty window");
    HostProfile const &hp = x->profiles[(size_t)w[i].profile];
    DcpProblem &p = st.problems[(size_t)i];
    p.profile = w[i].profile;
    p.L = L;
    p.code_row = x->row_off[(size_t)w[i].seq] + w[i].start;
    p.xt_row = std::max(L / 3, 1); // c-core/thread.c:112
    p.out = i;
    p.trellis = 0;
    max_s = std::max(max_s, p.xt_row);
    st.cells += (double)hp.K * (double)L;
    if (arena_kind != ARENA_NONE)
    {
      size_t const bytes = arena_kind == ARENA_TRELLIS ? trellis_bytes(L, hp.K) : dcp_table_bytes(L, hp.Kp);
      // trellises: offsets into d_trellis; DP tables: addresses the caller placed in x->tables
      p.trellis = arena_kind == ARENA_TRELLIS ? (int64_t)arena : x->table_addr[(size_t)i];
      arena += (bytes + 15) & ~(size_t)15;
    }
  }
  st.arena_bytes = arena;
  // Cost pass: the windows of short profiles go several to a wavefront (viterbi_pack.h).  They leave the
  // problem list and come back as packs: up to G windows of ONE profile each, longest first, so that the
  // windows of a pack are of similar length (a pack runs as many rows as its longest window).
  // DECIPHON_HIP_PACK=0 keeps every window on the one-window-per-wavefront kernels (tests compare the two).
  st.packs.clear();
  for (int s = 0; s <= DCP_NUM_PACK_SHAPES; ++s) st.pk_begin[s] = 0;
  char const *pack_env = getenv("DECIPHON_HIP_PACK");
  bool const packing = arena_kind == ARENA_NONE && !(pack_env && pack_env[0] == '0') &&
                       (uint64_t)x->row_off.back() < ((uint64_t)1 << 32); // code rows are addressed by u32 index
  if (packing)
  {
    std::vector<DcpProblem> packed, rest;
    for (DcpProblem const &p : st.problems)
      (x->profiles[(size_t)p.profile].pack >= 0 ? packed : rest).push_back(p);
    if (by_profile)
    {
      // order (shape, profile, longest first) without a comparison sort over everything: a stable scatter by shape
      // keeps the profiles ascending, then each profile's run is ordered by length -- a counting pass when the run
      // holds few distinct lengths (the windows of a chain: whole windows and one tail)
      bucket_stable(packed, DCP_NUM_PACK_SHAPES, [&](DcpProblem const &a) { return x->profiles[(size_t)a.profile].pack; });
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
        int sa = x->profiles[(size_t)a.profile].pack, sb = x->profiles[(size_t)b.profile].pack;
        if (sa != sb) return sa < sb;
        if (a.profile != b.profile) return a.profile < b.profile;
        return a.L > b.L;
      });
    int shape = 0;
    for (size_t i = 0; i < packed.size();)
    {
      int const sh = x->profiles[(size_t)packed[i].profile].pack;
      while (shape < sh) st.pk_begin[++shape] = (int)st.packs.size();
      int pq = 0, ps = 0;
      dcp_pack_shape(sh, &pq, &ps);
      int const G = 64 / ps;
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
    // four-lane groups: the packs of one profile go WG to a workgroup, which shares the profile's table in LDS
    st.pack_groups.clear();
    char const *lds_env = getenv("DECIPHON_HIP_PACK_LDS");
    bool const lds_tables = !(lds_env && lds_env[0] == '0');
    for (int s = 0; s < DCP_NUM_PACK_SHAPES; ++s)
    {
      st.pg_begin[s] = (int)st.pack_groups.size();
      int const wg = lds_tables ? dcp_pack_lds_waves(s) : 0;
      if (!wg) continue;
      for (int i = st.pk_begin[s]; i < st.pk_begin[s + 1];)
      {
        int j = i;
        while (j < st.pk_begin[s + 1] && j - i < wg && st.packs[(size_t)j].profile == st.packs[(size_t)i].profile) ++j;
        st.pack_groups.push_back(make_int2(i - st.pk_begin[s], j - i));
        i = j;
      }
    }
    st.pg_begin[DCP_NUM_PACK_SHAPES] = (int)st.pack_groups.size();
  }
  int const nu = (int)st.problems.size(); // windows that keep a wavefront (or a workgroup) to themselves
  // by (class, the narrow profiles of a class first -- one position per lane less: their own launch of the cost pass --,
  // profile)
  if (by_profile)
    bucket_stable(st.problems, 2 * DCP_NUM_CLASSES, [&](DcpProblem const &a) {
      HostProfile const &hp = x->profiles[(size_t)a.profile];
      return 2 * hp.cls + (hp.narrow ? 0 : 1);
    });
  else
    std::stable_sort(st.problems.begin(), st.problems.end(), [&](DcpProblem const &a, DcpProblem const &b) {
      HostProfile const &pa = x->profiles[(size_t)a.profile], &pb = x->profiles[(size_t)b.profile];
      if (pa.cls != pb.cls) return pa.cls < pb.cls;
      if (pa.narrow != pb.narrow) return pa.narrow;
      return a.profile < b.profile;
    });
  int i = 0;
  for (int c = 0; c < DCP_NUM_CLASSES; ++c)
  {
    st.c_begin[c] = i;
    st.c_profiles[c][0] = st.c_profiles[c][1] = 0;
    // (the list is in profile order inside either part: a profile is one run of it)
    auto const starts_run = [&](int j) { return j == st.c_begin[c] || st.problems[(size_t)j].profile != st.problems[(size_t)j - 1].profile; };
    while (i < nu && x->profiles[(size_t)st.problems[(size_t)i].profile].cls == c &&
           x->profiles[(size_t)st.problems[(size_t)i].profile].narrow)
      st.c_profiles[c][0] += starts_run(i), ++i;
    st.c_wide[c] = i;
    while (i < nu && x->profiles[(size_t)st.problems[(size_t)i].profile].cls == c) st.c_profiles[c][1] += starts_run(i), ++i;
  }
  st.c_begin[DCP_NUM_CLASSES] = i;
  if (i != nu) return fail(x, DCP_ELARGECORESIZE, "profile outside every kernel class");
  if (st.c_begin[DCP_STRIP_CLASS + 1] > st.c_begin[DCP_STRIP_CLASS])
    HIP_TRY(x, BK(x).d_ring.reserve((size_t)DCP_RING_SLOTS * DCP_RING_FLOATS), DCP_ENOMEM);
  int rc = ensure_xt(x, max_s + 1);
  if (rc) return rc;
  if (x->cur != 2) x->staged_n = -1; // a cost bank's problem list and results are about to be replaced
  // every allocation first: after the first copy is enqueued nothing below can fail but a copy itself
  HIP_TRY(x, BK(x).d_problems.reserve((size_t)std::max(nu, 1)), DCP_ENOMEM);
  if (!st.packs.empty()) HIP_TRY(x, BK(x).d_packs.reserve(st.packs.size()), DCP_ENOMEM);
  if (!st.pack_groups.empty()) HIP_TRY(x, BK(x).d_pack_groups.reserve(st.pack_groups.size()), DCP_ENOMEM);
  dcp_hip::Bank &B = BK(x);
  if (B.up_pending) HIP_TRY(x, hipEventSynchronize(B.up_ev), DCP_EFUNCUSE); // the previous lists have gone up
  B.up_pending = false;
  if ((rc = upload(x, B.d_problems, B.h_problems, st.problems, origin))) return rc;
  if ((rc = upload(x, B.d_packs, B.h_packs, st.packs, origin))) return rc;
  if ((rc = upload(x, B.d_pack_groups, B.h_groups, st.pack_groups, origin))) return rc;
  HIP_TRY(x, hipEventRecord(B.up_ev, origin), DCP_EFUNCUSE);
  B.up_pending = true;
  return 0;
}

DcpLaunch launch_args(dcp_hip *x, StagedPlan const &st, int c)
{
  DcpLaunch a;
  a.pool = x->d_pool.p;
  a.profiles = x->d_profiles.p;
  a.problems = BK(x).d_problems.p + st.c_begin[c];
  a.code_rows = x->d_rows.p;
  a.xt_table = x->d_xt.p;
  a.out = BK(x).d_out.p;
  a.arena = x->d_trellis.p;
  a.nprob = st.c_begin[c + 1] - st.c_begin[c];
  a.stream = x->stream;
  a.ring = BK(x).d_ring.p;
  return a;
}

// Launches the path (or cost) kernels of every class present: the classes run
// concurrently on their own streams, forked from and joined back into x->stream.
int launch_all(dcp_hip *x, StagedPlan const &st, bool path)
{
  int classes = 0;
  for (int c = 0; c < DCP_NUM_CLASSES; ++c) classes += st.c_begin[c + 1] > st.c_begin[c];
  Fork fk(x, classes > 1);
  int rc = fk.begin(x->stream);
  if (rc) return rc;
  for (int c = 0; c < DCP_NUM_CLASSES; ++c)
  {
    DcpLaunch a = launch_args(x, st, c);
    if (a.nprob <= 0) continue;
    if (path && c == DCP_STRIP_CLASS) continue; // replayed from the DP table instead (path_literal)
    if ((rc = fk.enter(x->cls_branch[c], a))) return rc;
    HIP_TRY(x, path ? dcp_launch_path(c, a) : dcp_launch_cost(c, a), DCP_EFUNCUSE);
    if ((rc = fk.leave(x->cls_branch[c]))) return rc;
  }
  return fk.join();
}

// Cost pass.  The packed kernels (short profiles, several windows per wavefront) have one stream per shape.
// Of the rest, a small launch that mixes single-wave classes goes out as ONE fused kernel (classes 0..3
// are contiguous in the sorted problem list); large launches keep one kernel per class, which fills the GPU
// by itself and has its own register budget.  Everything is forked from `origin` (the stream the window lists were
// uploaded on; x->stream by default) and joined into x->stream.
// reps > 1 (measurement): every kernel `reps` times in its own stream before the join -- the passes of a kernel class
// follow each other without waiting for the other classes, exactly as the batches of a scan do when a second batch is
// begun while the first is in flight (dcp_hip_cost_hits_begin): no kernel's tail leaves the GPU idle but the last's.
int launch_cost_all(dcp_hip *x, StagedPlan const &st, hipStream_t origin, int reps)
{
  if (!origin) origin = x->stream;
  int const single_wave = st.c_begin[4] - st.c_begin[0];
  int mixed = 0;
  for (int c = 0; c < 4; ++c) mixed += st.c_begin[c + 1] > st.c_begin[c];
  bool const fused = mixed >= 2 && single_wave <= 16384;
  int kernels = fused ? 1 : 0;
  for (int c = fused ? 4 : 0; c < DCP_NUM_CLASSES; ++c) kernels += st.c_begin[c + 1] > st.c_begin[c];
  for (int s = 0; s < DCP_NUM_PACK_SHAPES; ++s) kernels += st.pk_begin[s + 1] > st.pk_begin[s];
  char const *narrow_env = getenv("DECIPHON_HIP_NARROW");
  bool const narrow = !(narrow_env && narrow_env[0] == '0');
  // DECIPHON_HIP_XCD_PLACEMENT=plain | eighths: every class's cost kernel that way (measurements, tests); auto, or
  // not set: dcp_xcd_placement decides per launch
  int placement = DCP_PLACE_AUTO;
  if (char const *e = getenv("DECIPHON_HIP_XCD_PLACEMENT"))
  {
    if (!strcmp(e, "plain")) placement = DCP_PLACE_PLAIN;
    else if (!strcmp(e, "eighths")) placement = DCP_PLACE_EIGHTHS;
    else if (strcmp(e, "auto")) return fail(x, DCP_EFUNCUSE, "DECIPHON_HIP_XCD_PLACEMENT is not plain, eighths or auto");
  }
  for (int c = 4; narrow && c < DCP_NUM_CLASSES; ++c) kernels += st.c_wide[c] > st.c_begin[c];
  // x->stream joins the kernels only after the last launch (Fork::join): a wait is a barrier in x->stream's hardware
  // queue, and a stream that shares that queue would start its kernel behind every barrier issued before
  // (profiles/r02_step_timeline.txt)
  Fork fk(x, kernels > 1 || origin != x->stream);
  int rc = fk.begin(origin);
  if (rc) return rc;
  // Launch order = start order (the hardware runs a few queues side by side and takes kernels as they come):
  // the classes with the fewest, longest-running workgroups go first -- multi-wave groups, then 8, 6, 4, 3
  // positions per lane -- and the packed kernels with their many short wavefronts last, where they fill what
  // the tails of the others leave idle.  (The other way round the K > 384 classes ran alone at the end of a
  // Pfam-shaped step: 33 + 50 ms of 456, profiles/r02_b.)
  for (int c = DCP_NUM_CLASSES - 1; c >= (fused ? 4 : 0); --c)
  {
    DcpLaunch b = launch_args(x, st, c);
    if (b.nprob <= 0) continue;
    if ((rc = fk.enter(x->cls_branch[c], b))) return rc;
    b.placement = placement;
    // the windows that fit with one position per lane less (dcp_class_narrow_limit) lead the class's list and have
    // their own kernel, on its own stream.  DECIPHON_HIP_NARROW=0: the class's kernel for all (tests compare).
    int const nn = narrow ? st.c_wide[c] - st.c_begin[c] : 0;
    if (nn > 0)
    {
      DcpLaunch n = b;
      n.nprob = nn;
      n.windows_per_profile = nn / st.c_profiles[c][0];
      if ((rc = fk.enter(x->narrow_branch[c], n))) return rc;
      for (int r = 0; r < reps; ++r) HIP_TRY(x, dcp_launch_cost_narrow(c, n), DCP_EFUNCUSE);
      if ((rc = fk.leave(x->narrow_branch[c]))) return rc;
      b.problems += nn;
      b.nprob -= nn;
    }
    if (b.nprob > 0)
    {
      // all of the class's windows in one launch (no narrow kernel, or none wanted): both parts' profiles
      int const np = st.c_profiles[c][1] + (nn > 0 ? 0 : st.c_profiles[c][0]);
      b.windows_per_profile = b.nprob / np;
      for (int r = 0; r < reps; ++r) HIP_TRY(x, dcp_launch_cost(c, b), DCP_EFUNCUSE);
    }
    if ((rc = fk.leave(x->cls_branch[c]))) return rc;
  }
  if (fused)
  {
    DcpLaunch a = launch_args(x, st, 0);
    a.nprob = single_wave;
    if ((rc = fk.enter(x->cls_branch[0], a))) return rc;
    for (int r = 0; r < reps; ++r) HIP_TRY(x, dcp_launch_cost_fused(a), DCP_EFUNCUSE);
    if ((rc = fk.leave(x->cls_branch[0]))) return rc;
  }
  for (int s = DCP_NUM_PACK_SHAPES - 1; s >= 0; --s)
  {
    int const np = st.pk_begin[s + 1] - st.pk_begin[s];
    if (np <= 0) continue;
    DcpLaunch a = launch_args(x, st, 0);
    if ((rc = fk.enter(x->pack_branch[s], a))) return rc;
    int const ng = st.pg_begin[s + 1] - st.pg_begin[s];
    for (int r = 0; r < reps; ++r)
    {
      if (ng > 0)
        HIP_TRY(x, dcp_launch_cost_pack_lds(s, a, BK(x).d_packs.p + st.pk_begin[s], BK(x).d_pack_groups.p + st.pg_begin[s], ng,
                                            (uint32_t)x->row_off.back()),
                DCP_EFUNCUSE);
      else
        HIP_TRY(x, dcp_launch_cost_pack(s, a, BK(x).d_packs.p + st.pk_begin[s], np, (uint32_t)x->row_off.back()), DCP_EFUNCUSE);
    }
    if ((rc = fk.leave(x->pack_branch[s]))) return rc;
  }
  return fk.join();
}

} // namespace dcp_engine

namespace
{

// priority 0: the default, what a stream created without one has
bool create_branch(Branch &b, int priority)
{
  return hipStreamCreateWithPriority(&b.stream, hipStreamNonBlocking, priority) == hipSuccess &&
         hipEventCreateWithFlags(&b.joined, hipEventDisableTiming) == hipSuccess;
}

void destroy_branch(Branch &b)
{
  if (b.stream) (void)hipStreamDestroy(b.stream);
  if (b.joined) (void)hipEventDestroy(b.joined);
}

} // namespace

extern "C" {

int dcp_hip_device_count(void)
{
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

struct dcp_hip *dcp_hip_new(int device)
{
  int n = dcp_hip_device_count();
  if (device < 0 || device >= n) return nullptr;
  if (hipSetDevice(device) != hipSuccess) return nullptr;
  dcp_hip *x = new dcp_hip;
  x->device = device;
  bool ok = hipStreamCreateWithFlags(&x->stream, hipStreamNonBlocking) == hipSuccess;
  ok = ok && hipEventCreateWithFlags(&x->fork_ev, hipEventDisableTiming) == hipSuccess;
  int prio_low = 0, prio_high = 0;
  ok = ok && hipDeviceGetStreamPriorityRange(&prio_low, &prio_high) == hipSuccess;
  // The multi-wave classes (K > 640) run on high-priority streams.  A workgroup of several wavefronts of 160-256
  // registers each is placed only where that much is free at once, and beside kernels of small wavefronts (the packed
  // kernels, 3 or 4 positions per lane) every slot that frees is taken by one of those first: on the headline workload
  // (6,2) -- 1 % of the cells -- then lasted 317 of the pass's 364 ms and held up the kernel behind it in its hardware
  // queue (the 32-lane packs, 11 % of the cells, which ran alone at the end).  A high-priority queue is served first.
  // DECIPHON_HIP_PRIO_FROM: first class (viterbi_kernels.h) that gets one; 99 = none (experiments).
  int prio_from = 6;
  if (char const *e = getenv("DECIPHON_HIP_PRIO_FROM")) prio_from = atoi(e);
  for (int c = 0; ok && c < DCP_NUM_CLASSES; ++c) ok = create_branch(x->cls_branch[c], c >= prio_from ? prio_high : 0);
  for (int s = 0; ok && s < DCP_NUM_PACK_SHAPES; ++s) ok = create_branch(x->pack_branch[s], 0);
  for (int c = 4; ok && c <= 6; ++c) ok = create_branch(x->narrow_branch[c], 0);
  // The path pass: streams of its own, alternately of high and of normal priority.  The runtime feeds four hardware
  // queues per priority level and a queue runs its kernels one after the other; a path pass is one chain of kernels per
  // class (checkpoints, then blocks and traceback in turns), few wavefronts each, bound by latency: on one level the
  // fifth to seventh chain started only when one of the first four had ended (the pass of 2301 hits of the headline scan:
  // 55-57 ms, on two levels 48-50).  dcp_scan_run calls it with no cost batch in flight; beside one, the chains on the
  // normal level queue behind the cost kernels.
  if (char const *e = getenv("DECIPHON_HIP_PATH_STREAM_PRIORITY")) // experiment: 0 = the same priority as the cost streams
    if (e[0] == '0') prio_high = 0;
  ok = ok && hipStreamCreateWithPriority(&x->path_set.stream, hipStreamNonBlocking, prio_high) == hipSuccess;
  ok = ok && hipEventCreateWithFlags(&x->path_set.fork_ev, hipEventDisableTiming) == hipSuccess;
  for (int c = 0; ok && c < DCP_NUM_CLASSES; ++c) ok = create_branch(x->path_set.cls_branch[c], c % 2 ? prio_high : 0);
  ok = ok && hipStreamCreateWithFlags(&x->upload_stream, hipStreamNonBlocking) == hipSuccess;
  for (int b = 0; ok && b < 3; ++b)
  {
    if (b < 2) ok = ok && hipEventCreateWithFlags(&x->bank[b].done_ev, hipEventDisableTiming) == hipSuccess;
    ok = ok && hipEventCreateWithFlags(&x->bank[b].up_ev, hipEventDisableTiming) == hipSuccess;
  }
  if (!ok)
  {
    dcp_hip_del(x);
    return nullptr;
  }
  x->seq_off.assign(1, 0);
  x->row_off.assign(1, 0);
  return x;
}

void dcp_hip_del(struct dcp_hip *x)
{
  if (!x) return;
  (void)hipSetDevice(x->device);
  (void)hipDeviceSynchronize(); // batches begun and never ended included
  for (int c = 0; c < DCP_NUM_CLASSES; ++c)
  {
    destroy_branch(x->cls_branch[c]);
    destroy_branch(x->narrow_branch[c]);
    destroy_branch(x->path_set.cls_branch[c]);
  }
  for (int s = 0; s < DCP_NUM_PACK_SHAPES; ++s) destroy_branch(x->pack_branch[s]);
  if (x->path_set.stream) (void)hipStreamDestroy(x->path_set.stream);
  if (x->path_set.fork_ev) (void)hipEventDestroy(x->path_set.fork_ev);
  if (x->upload_stream) (void)hipStreamDestroy(x->upload_stream);
  for (int b = 0; b < 3; ++b)
  {
    if (x->bank[b].done_ev) (void)hipEventDestroy(x->bank[b].done_ev);
    if (x->bank[b].up_ev) (void)hipEventDestroy(x->bank[b].up_ev);
  }
  if (x->fork_ev) (void)hipEventDestroy(x->fork_ev);
  if (x->stream) (void)hipStreamDestroy(x->stream);
  delete x;
}

char const *dcp_hip_strerror(struct dcp_hip const *x) { return x ? x->err.c_str() : "no engine"; }

int dcp_hip_encode(char const *data, int64_t n, uint8_t *out)
{
  if (n < 0 || (n > 0 && (!data || !out))) return DCP_EFUNCUSE;
  return dcp_encode_sequence(data, n, out);
}

int dcp_hip_set_sequences(struct dcp_hip *x, int nseq, uint8_t const *nt, int64_t const *offsets)
{
  if (!x || nseq < 0 || !offsets || (nseq > 0 && !nt)) return DCP_EFUNCUSE;
  if (outstanding_batches(x)) return refuse_outstanding(x);
  HIP_TRY(x, hipSetDevice(x->device), DCP_EFUNCUSE);
  // everything is checked before anything is replaced: a refused call leaves the previous reads in force
  std::vector<int64_t> row_off((size_t)nseq + 1);
  int64_t max_len = 0, rows = 0;
  if (offsets[0] != 0) return fail(x, DCP_EFUNCUSE, "offsets[0] must be 0");
  for (int i = 0; i < nseq; ++i)
  {
    int64_t len = offsets[i + 1] - offsets[i];
    if (len < 0) return fail(x, DCP_EFUNCUSE, "offsets must not decrease");
    max_len = std::max(max_len, len);
    row_off[(size_t)i] = rows;
    rows += len + 1;
  }
  row_off[(size_t)nseq] = rows;
  int64_t const total = offsets[nseq];
  for (int64_t i = 0; i < total; ++i)
    if (nt[i] > 3) return fail(x, DCP_ESEQABC, "nucleotide index above 3");
  ++x->gen;
  x->seq_off.assign(offsets, offsets + nseq + 1);
  x->row_off = std::move(row_off);
  HIP_TRY(x, hipStreamSynchronize(x->stream), DCP_EFUNCUSE);
  HIP_TRY(x, x->d_nt.reserve((size_t)std::max<int64_t>(total, 1)), DCP_ENOMEM);
  HIP_TRY(x, x->d_seq_off.reserve((size_t)nseq + 1), DCP_ENOMEM);
  HIP_TRY(x, x->d_row_off.reserve((size_t)nseq + 1), DCP_ENOMEM);
  HIP_TRY(x, x->d_rows.reserve((size_t)std::max<int64_t>(rows, 1)), DCP_ENOMEM);
  if (total)
    HIP_TRY(x, hipMemcpyAsync(x->d_nt.p, nt, (size_t)total, hipMemcpyHostToDevice, x->stream), DCP_EFUNCUSE);
  HIP_TRY(x, hipMemcpyAsync(x->d_seq_off.p, x->seq_off.data(), ((size_t)nseq + 1) * sizeof(int64_t),
                            hipMemcpyHostToDevice, x->stream),
          DCP_EFUNCUSE);
  HIP_TRY(x, hipMemcpyAsync(x->d_row_off.p, x->row_off.data(), ((size_t)nseq + 1) * sizeof(int64_t),
                            hipMemcpyHostToDevice, x->stream),
          DCP_EFUNCUSE);
  HIP_TRY(x, dcp_launch_encode(x->d_nt.p, x->d_seq_off.p, x->d_row_off.p, nseq, max_len, x->d_rows.p, x->stream),
          DCP_EFUNCUSE);
  HIP_TRY(x, hipStreamSynchronize(x->stream), DCP_EFUNCUSE);
  return 0;
}

int dcp_hip_set_mode(struct dcp_hip *x, int multi_hits, int hmmer3_compat)
{
  if (!x) return DCP_EFUNCUSE;
  if (outstanding_batches(x)) return refuse_outstanding(x);
  bool mh = multi_hits != 0, h3 = hmmer3_compat != 0;
  ++x->gen;
  if (x->mode_set && (mh != x->multi_hits || h3 != x->hmmer3_compat)) x->xt_rows = 0;
  x->multi_hits = mh;
  x->hmmer3_compat = h3;
  x->mode_set = true;
  return 0;
}

int dcp_hip_set_xtrans_table(struct dcp_hip *x, int rows, float const *xt)
{
  if (!x || rows < 0 || (rows > 0 && !xt)) return DCP_EFUNCUSE;
  if (outstanding_batches(x)) return refuse_outstanding(x);
  ++x->gen;
  x->xt_override.assign((size_t)rows * DCP_XT_STRIDE, 0.0f);
  for (int r = 0; r < rows; ++r)
    memcpy(x->xt_override.data() + (size_t)r * DCP_XT_STRIDE, xt + (size_t)r * DCP_NUM_XTRANS,
           sizeof(float) * DCP_NUM_XTRANS);
  x->xt_rows = 0; // rebuild the device table at the next launch
  return 0;
}

void dcp_hip_xtrans(int seq_size, int multi_hits, int hmmer3_compat, float xt[DCP_HIP_NUM_XTRANS])
{
  dcp_xtrans(seq_size, multi_hits != 0, hmmer3_compat != 0, xt);
}

} // extern "C"
