// engine_path.cpp -- the path pass of the C ABI: the fast pass over DP tables in blocks, the literal pass, the results.
#include "engine_internal.h"

namespace
{

// The fast path pass in blocks (dcp_types.h): rows between checkpoints.  DECIPHON_HIP_CKPT_ROWS overrides (tests
// use small blocks; 0 = whole windows, the tables of round 1); always a multiple of 5.
int ckpt_rows()
{
  int B = DCP_CKPT_ROWS_DEFAULT;
  if (char const *e = getenv("DECIPHON_HIP_CKPT_ROWS")) B = atoi(e);
  if (B < 0) B = 0;
  return B - B % 5;
}

// step buffers: a path has at most L emitting steps; mute steps (S, B, E, T, D runs) are few
// in practice.  DECIPHON_HIP_UNZIP_CAP (steps) overrides the capacity: a test hook for the
// overflow fallbacks.
// step_off (the caller keeps it until the stream has passed the copy) goes to the device with the buffers it describes.
int stage_steps(Pass const &ps, Staged const &st, int n, std::vector<int64_t> &step_off)
{
  dcp_hip *const x = ps.x;
  int64_t cap_override = 0;
  if (char const *e = getenv("DECIPHON_HIP_UNZIP_CAP")) cap_override = atoll(e);
  step_off.assign((size_t)n + 1, 0);
  for (DcpProblem const &p : st.problems)
    step_off[(size_t)p.out + 1] =
        cap_override > 0 ? cap_override : 2 * (int64_t)p.L + 2 * (int64_t)x->profiles[(size_t)p.profile].K + 64;
  for (int i = 0; i < n; ++i) step_off[(size_t)i + 1] += step_off[(size_t)i];
  HIP_TRY(x, x->d_steps.reserve((size_t)step_off[(size_t)n]), DCP_ENOMEM);
  HIP_TRY(x, x->d_step_off.reserve((size_t)n + 1), DCP_ENOMEM);
  HIP_TRY(x, x->d_nsteps.reserve((size_t)n), DCP_ENOMEM);
  HIP_TRY(x, hipMemcpyAsync(x->d_step_off.p, step_off.data(), ((size_t)n + 1) * sizeof(int64_t),
                            hipMemcpyHostToDevice, ps.on.stream),
          DCP_EFUNCUSE);
  return 0;
}

// what a path pass left on the device, on the host (pinned buffers of x)
struct PathFetched
{
  float const *out = nullptr;      // the first nout floats of d_out
  int32_t const *nsteps = nullptr; // per window; negative: no steps came back for it
  std::vector<int64_t> compact;    // steps[compact[i] .. compact[i+1]) are window i's (empty where nsteps[i] < 0)
  uint32_t const *steps = nullptr;
  size_t total_steps = 0;
};

// Brings the scores, the step counts and then only the steps actually written to the host.
int fetch_results(Pass const &ps, int n, size_t nout, PathFetched &f)
{
  dcp_hip *const x = ps.x;
  HIP_TRY(x, x->h_out.reserve(nout), DCP_ENOMEM);
  HIP_TRY(x, hipMemcpyAsync(x->h_out.p, ps.lists.d_out.p, nout * sizeof(float), hipMemcpyDeviceToHost, ps.on.stream), DCP_EFUNCUSE);
  f.out = x->h_out.p;
  HIP_TRY(x, x->h_nsteps.reserve((size_t)std::max(n, 1)), DCP_ENOMEM);
  HIP_TRY(x, hipMemcpyAsync(x->h_nsteps.p, x->d_nsteps.p, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, ps.on.stream),
          DCP_EFUNCUSE);
  HIP_TRY(x, hipStreamSynchronize(ps.on.stream), DCP_EFUNCUSE);
  int32_t const *const nsteps = f.nsteps = x->h_nsteps.p;
  std::vector<int64_t> &compact = f.compact;
  compact.assign((size_t)n + 1, 0);
  for (int i = 0; i < n; ++i) compact[(size_t)i + 1] = compact[(size_t)i] + (nsteps[i] > 0 ? nsteps[i] : 0);
  size_t const total = f.total_steps = (size_t)compact[(size_t)n];
  f.steps = nullptr;
  if (!total) return 0;
  HIP_TRY(x, x->d_compact_off.reserve((size_t)n + 1), DCP_ENOMEM);
  HIP_TRY(x, x->d_compact.reserve(total), DCP_ENOMEM);
  if (x->h_steps_used == x->h_steps.size()) x->h_steps.emplace_back();
  PinBuf<uint32_t> &h_steps = x->h_steps[x->h_steps_used++];
  HIP_TRY(x, h_steps.reserve(total), DCP_ENOMEM);
  HIP_TRY(x, hipMemcpyAsync(x->d_compact_off.p, compact.data(), ((size_t)n + 1) * sizeof(int64_t), hipMemcpyHostToDevice,
                            ps.on.stream),
          DCP_EFUNCUSE);
  HIP_TRY(x, dcp_launch_compact_steps(x->d_steps.p, x->d_step_off.p, x->d_compact_off.p, x->d_compact.p, n, ps.on.stream),
          DCP_EFUNCUSE);
  HIP_TRY(x, hipMemcpyAsync(h_steps.p, x->d_compact.p, total * sizeof(uint32_t), hipMemcpyDeviceToHost, ps.on.stream),
          DCP_EFUNCUSE);
  HIP_TRY(x, hipStreamSynchronize(ps.on.stream), DCP_EFUNCUSE);
  f.steps = h_steps.p;
  return 0;
}

int fetch_trellis(Pass const &ps, int i)
{
  dcp_hip *const x = ps.x;
  PathResult &r = x->paths[(size_t)i];
  if (r.trellis_on_host) return 0;
  std::vector<unsigned char> &buf = x->host_trellis[(size_t)i];
  size_t const bytes = trellis_bytes(r.L, r.K);
  buf.resize(bytes);
  HIP_TRY(x, hipMemcpyAsync(buf.data(), x->d_trellis.p + r.trellis_off, bytes, hipMemcpyDeviceToHost, ps.on.stream),
          DCP_EFUNCUSE);
  HIP_TRY(x, hipStreamSynchronize(ps.on.stream), DCP_EFUNCUSE);
  r.trellis_on_host = true;
  return 0;
}

// The kernels of every class of a staged list but `skip`: the classes of a slice are each too small to fill the GPU and
// each lasts as long as its longest window, so they go out on their own streams, forked from and joined back into the
// pass's.  launch(c, a) queues class c's on a.stream.
template <class Launch> int each_class(Pass const &ps, StagedPlan const &st, int skip, Launch launch)
{
  int classes = 0;
  for (int c = 0; c < DCP_NUM_CLASSES; ++c) classes += st.c_begin[c + 1] > st.c_begin[c];
  Fork fk(ps, classes > 1);
  int rc = fk.begin(ps.on.stream);
  if (rc) return rc;
  for (int c = 0; c < DCP_NUM_CLASSES; ++c)
  {
    DcpLaunch a = launch_args(ps, st, c);
    if (a.nprob <= 0 || c == skip) continue;
    if ((rc = fk.enter(ps.on.cls_branch[c], a))) return rc;
    if ((rc = launch(c, a))) return rc;
    if ((rc = fk.leave(ps.on.cls_branch[c]))) return rc;
  }
  return fk.join();
}

// The literal pass's path kernels; the strip class is replayed from the DP table instead (literal_strips)
int launch_all(Pass const &ps, StagedPlan const &st)
{
  return each_class(ps, st, DCP_STRIP_CLASS, [&](int c, DcpLaunch const &a) {
    HIP_TRY(ps.x, dcp_launch_path(c, a), DCP_EFUNCUSE);
    return 0;
  });
}

// HBM the fast pass fills with DP tables.  A slice takes as long as its longest window however
// few windows it holds, so more memory means fewer, fuller slices -- but VRAM is cleared when it
// is allocated (35 GB/s, scripts/alloc_timing.py), so an arena sized for the whole request costs
// more than the slices it saves unless the engine lives long.  Default: what dcp_hip_path_reserve
// set aside, at least 4 GB -- enough for thousands of windows since the tables are held a block at a time
// (12 B per cell of 505 rows plus 40 B per position and 500 rows of checkpoints, about a fifteenth of a 10 kb
// window's whole table).  DECIPHON_HIP_PATH_BUDGET_MB overrides.
size_t path_budget(dcp_hip *x)
{
  if (char const *e = getenv("DECIPHON_HIP_PATH_BUDGET_MB")) return (size_t)std::max(atol(e), 1L) << 20;
  size_t const want = std::max(x->tables.held, 2 * TableArena::CHUNK);
  size_t free_b = 0, total_b = 0;
  if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return want;
  size_t const margin = (size_t)6 << 30; // steps, trellis redo's, the caller's own buffers
  size_t const avail = free_b + x->tables.held;
  return std::max(std::min(want, avail > 2 * margin ? avail - margin : avail / 2), (size_t)256 << 20);
}

// The memory plan (path_plan.h) of these windows under the engine's settings: rows between checkpoints, budget and its
// strictness, the chunks the arena holds, DECIPHON_HIP_PATH_GROUP (blocks side by side, at least 1).
DcpPathPlan plan_path(dcp_hip *x, DcpPathKind kind, std::vector<dcp_hip_window> const &w, size_t budget)
{
  std::vector<DcpPathWindow> pw;
  for (dcp_hip_window const &v : w)
  {
    HostProfile const &hp = x->profiles[(size_t)v.profile];
    pw.push_back(DcpPathWindow{v.stop - v.start, hp.K, hp.Kp, hp.W, hp.cls == DCP_STRIP_CLASS});
  }
  char const *group = getenv("DECIPHON_HIP_PATH_GROUP");
  return dcp_plan_path(kind, (int)pw.size(), pw.data(), ckpt_rows(), budget, path_budget_strict(), x->tables.largest_chunk(),
                       group ? std::max(atoi(group), 1) : 0);
}

// A slice: the placements of windows [b, e) of a plan, until the arena refuses one (e == b: not even the first).  Their
// addresses go to x->table_addr, where stage() looks for them.
size_t place_slice(dcp_hip *x, DcpPathPlan const &plan, size_t b, size_t budget)
{
  x->tables.reset();
  x->table_addr.clear();
  size_t e = b;
  for (; e < plan.place.size(); ++e)
  {
    unsigned char *at = x->tables.place(plan.place[e].bytes, budget);
    if (!at) break;
    x->table_addr.push_back((int64_t)(uintptr_t)at);
  }
  x->path_table_bytes = std::max(x->path_table_bytes, (int64_t)x->tables.placed);
  return e;
}

// The literal pass of the profiles beyond 4096 positions (strip class): the register-resident path kernel does not
// reach them; their trellis is replayed row by row from the DP table (row_replay.h), into d_trellis at trel_off[j] for
// window w[sl[..]] = j, its score into slot j of d_out.  The tables are placed slice by slice within the budget like
// the fast pass's.  A window keeps its whole table, with (L + 1) * 3 * K floats of scratch, where the two fit the
// budget; where they do not -- and the budget is not strict -- the table comes a block at a time from checkpoints, G
// blocks side by side, and a block serves the rows of the traceback's partition (dcp_types.h): DCP_PATH_LITERAL.
// count_blocked: the windows taken in blocks go into x->path_blocked (a dcp_hip_path whose fast pass was skipped).
int literal_strips(Pass const &ps, std::vector<dcp_hip_window> const &w, std::vector<int> const &sl,
                   std::vector<size_t> const &trel_off, bool count_blocked)
{
  dcp_hip *const x = ps.x;
  int const n = (int)w.size();
  size_t const budget = path_budget(x);
  std::vector<dcp_hip_window> strips;
  for (int j : sl)
  {
    if (w[(size_t)j].stop - w[(size_t)j].start < 1) return fail(x, DCP_EZEROSEQ, "empty window");
    strips.push_back(w[(size_t)j]);
  }
  DcpPathPlan const plan = plan_path(x, DCP_PATH_LITERAL, strips, budget);
  int const B = plan.B, G = plan.G;
  if (count_blocked) x->path_blocked += plan.blocked;
  HIP_TRY(x, x->d_aux.reserve(4 * sl.size()), DCP_ENOMEM);
  for (size_t sb = 0; sb < sl.size();)
  {
    size_t const se = place_slice(x, plan, sb, budget);
    if (se == sb) return fail(x, DCP_ENOMEM, "no device memory for the DP table of a long profile's path pass");
    int const ns = (int)(se - sb);
    Staged ss;
    int rc = stage(ps, ns, strips.data() + sb, ARENA_TABLE, ss);
    if (rc) return rc;
    std::vector<int64_t> aux(4 * (size_t)ns); // [4][windows of the slice]: trellis, scratch, checkpoints, score slot
    int max_rows = 0, max_blocks = 0;
    for (int i = 0; i < ns; ++i)
    {
      int const j = sl[sb + (size_t)i];
      DcpPathPlace const &p = plan.place[sb + (size_t)i];
      aux[(size_t)i] = (int64_t)(uintptr_t)(x->d_trellis.p + trel_off[(size_t)j]);
      aux[(size_t)ns + i] = x->table_addr[(size_t)i] + (int64_t)p.scratch_off;
      aux[2 * (size_t)ns + i] = p.in_blocks ? x->table_addr[(size_t)i] + (int64_t)p.ckpt_off : 0;
      aux[3 * (size_t)ns + i] = j;
      max_rows = std::max(max_rows, p.replay_rows);
      if (p.in_blocks) max_blocks = std::max(max_blocks, p.blocks);
    }
    HIP_TRY(x, hipMemcpyAsync(x->d_aux.p, aux.data(), aux.size() * sizeof(int64_t), hipMemcpyHostToDevice, ps.on.stream),
            DCP_EFUNCUSE);
    DcpLaunch a = launch_args(ps, ss, DCP_STRIP_CLASS);
    a.arena = nullptr;
    // (null, alt) of the slice's windows go behind the n scores of the pass
    DcpLaunch store = a;
    store.out = a.out + n;
    // the checkpoints of the windows in blocks, then G blocks at a time; a window that keeps its whole table is one
    // block of the first round
    int64_t const *d_ckpt = x->d_aux.p + 2 * (size_t)ns;
    if (max_blocks > 0) HIP_TRY(x, dcp_launch_strip_ckpt(store, d_ckpt, B), DCP_EFUNCUSE);
    for (int it = 0; it == 0 || it * G < max_blocks; ++it)
    {
      HIP_TRY(x, dcp_launch_strip_store(store, d_ckpt, B, G, it), DCP_EFUNCUSE);
      HIP_TRY(x, dcp_launch_replay(a, x->d_aux.p, B, G, it, max_rows), DCP_EFUNCUSE);
    }
    HIP_TRY(x, hipStreamSynchronize(ps.on.stream), DCP_EFUNCUSE); // aux is read by the copy above; the next slice reuses the tables
    sb = se;
  }
  return 0;
}

// The literal path pass (viterbi_path as the reference runs it, pass by pass, with the
// trellis in HBM) + trellis_unzip on the device, for the windows path_wins[idx[..]].
int path_literal(Pass const &ps, std::vector<int> const &idx, bool count_blocked = false)
{
  dcp_hip *const x = ps.x;
  int const n = (int)idx.size();
  if (n == 0) return 0;
  std::vector<dcp_hip_window> w((size_t)n);
  for (int j = 0; j < n; ++j) w[(size_t)j] = x->path_wins[(size_t)idx[(size_t)j]];
  // where the plan of the list below puts every window's trellis (ARENA_TRELLIS)
  std::vector<size_t> const trel_off = trellis_offsets(n, w.data(), x->plan_profiles.data());
  std::vector<int> sl; // the windows of the strip class
  for (int j = 0; j < n; ++j)
    if (x->profiles[(size_t)w[(size_t)j].profile].cls == DCP_STRIP_CLASS) sl.push_back(j);
  HIP_TRY(x, ps.lists.d_out.reserve(3 * (size_t)n), DCP_ENOMEM);
  HIP_TRY(x, x->d_trellis.reserve(trel_off[(size_t)n]), DCP_ENOMEM);
  int rc = 0;
  // the strip class first: the problem list below replaces its lists on the device
  if (!sl.empty() && (rc = literal_strips(ps, w, sl, trel_off, count_blocked))) return rc;
  Staged st;
  if ((rc = stage(ps, n, w.data(), ARENA_TRELLIS, st))) return rc;
  if ((rc = launch_all(ps, st))) return rc; // (not the strip class)

  std::vector<int64_t> step_off;
  if ((rc = stage_steps(ps, st, n, step_off))) return rc;
  {
    DcpLaunch a = launch_args(ps, st, 0);
    a.problems = ps.lists.d_problems.p;
    a.nprob = n;
    HIP_TRY(x, dcp_launch_unzip(a, x->d_steps.p, x->d_step_off.p, x->d_nsteps.p), DCP_EFUNCUSE);
  }
  PathFetched f;
  if ((rc = fetch_results(ps, n, (size_t)n, f))) return rc;
  // every earlier trellis offset pointed into the arena that was just rewritten
  for (PathResult &r : x->paths) r.has_trellis = r.trellis_on_host = false;
  for (DcpProblem const &p : st.problems)
  {
    int const i = idx[(size_t)p.out];
    PathResult &r = x->paths[(size_t)i];
    r.K = x->profiles[(size_t)p.profile].K;
    r.L = p.L;
    r.score = f.out[(size_t)p.out];
    r.trellis_off = (size_t)p.trellis;
    r.has_trellis = true;
    r.trellis_on_host = false;
    r.steps = nullptr;
    r.nsteps = 0;
    r.owned.clear();
    int32_t const ns = f.nsteps[(size_t)p.out];
    // a window with no finite path at all (score +inf) has no steps: the reference never walks such
    // a trellis (process_window stops at a non-finite lrt, c-core/thread.c:118-121)
    if (!(r.score < INFINITY)) continue;
    if (ns >= 0)
    {
      r.steps = f.steps + f.compact[(size_t)p.out];
      r.nsteps = ns;
    }
    else
    {
      // the device buffer was too small for this path: fetch the trellis and unzip here
      if ((rc = fetch_trellis(ps, i))) return rc;
      uint32_t const *xn = reinterpret_cast<uint32_t const *>(x->host_trellis[(size_t)i].data());
      uint16_t const *nd = reinterpret_cast<uint16_t const *>(xn + (r.L + 1));
      std::vector<int32_t> ids, sizes;
      if ((rc = dcp_unzip(r.K, r.L, xn, nd, ids, sizes))) return fail(x, rc, "trellis_unzip failed");
      r.owned.resize(ids.size());
      for (size_t k = 0; k < ids.size(); ++k) r.owned[k] = (uint32_t)ids[k] | ((uint32_t)sizes[k] << 16);
      r.steps = r.owned.data();
      r.nsteps = (int32_t)r.owned.size();
    }
  }
  return 0;
}

// The fast path pass: the cost pass once more with every row's values kept in HBM, then a
// traceback that reads the back-pointers off those values (traceback.h).  Windows whose
// traceback meets an exact tie the values alone cannot resolve come back in `redo`.
// DECIPHON_HIP_TIMING=1: phase times of the path pass on stderr (synchronises between phases)
// windows [b, e) of x->path_sorted (window i there is window x->path_order[i] of the request)
int path_fast(Pass const &ps, int b, int e, std::vector<int> &redo)
{
  dcp_hip *const x = ps.x;
  int const n = e - b;
  Stopwatch tm(ps.on.stream);
  Staged st;
  int rc = stage(ps, n, x->path_sorted.data() + b, ARENA_TABLE, st);
  if (rc) return rc;
  tm.lap("stage");
  HIP_TRY(x, ps.lists.d_out.reserve(2 * (size_t)n), DCP_ENOMEM);
  int const B = x->path_plan.B, G = x->path_plan.G;
  // checkpoints sit behind each window's block tables (DcpPathPlace::ckpt_off)
  std::vector<int64_t> ckpt_addr((size_t)n, 0), step_off;
  StreamDrain drain{ps.on.stream}; // destroyed before the two: an early return does not pull them from under a copy
  int max_blocks = 1, strip_blocks = 0; // strip_blocks > 0: windows of the strip class that go in blocks
  for (DcpProblem const &p : st.problems)
  {
    DcpPathPlace const &pl = x->path_plan.place[(size_t)(b + p.out)];
    if (!pl.in_blocks) continue; // a window of the strip class that keeps its whole table has no checkpoints: address 0
    ckpt_addr[(size_t)p.out] = p.trellis + (int64_t)pl.ckpt_off;
    int &most = x->profiles[(size_t)p.profile].cls == DCP_STRIP_CLASS ? strip_blocks : max_blocks;
    most = std::max(most, pl.blocks);
  }
  HIP_TRY(x, x->d_ckpt_addr.reserve((size_t)n), DCP_ENOMEM);
  HIP_TRY(x, hipMemcpyAsync(x->d_ckpt_addr.p, ckpt_addr.data(), (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice, ps.on.stream),
          DCP_EFUNCUSE);
  HIP_TRY(x, x->d_trace.reserve((size_t)n), DCP_ENOMEM);
  HIP_TRY(x, hipMemsetAsync(x->d_trace.p, 0, (size_t)n * sizeof(DcpTraceState), ps.on.stream), DCP_EFUNCUSE);
  if ((rc = stage_steps(ps, st, n, step_off))) return rc;
  // The checkpoints of the windows that have more than one block, then the blocks from the last to the first.
  // Every class does that on its own stream (each_class) -- checkpoints, then per block its rows and the traceback
  // through it -- without waiting for the others: a class's windows are done when ITS slowest is, and the store kernel
  // of one class runs beside the traceback of another (one join at the end).
  char const *fused_env = getenv("DECIPHON_HIP_PATH_FUSED");
  bool const fused = !(fused_env && fused_env[0] == '0');
  rc = each_class(ps, st, -1, [&](int c, DcpLaunch a) {
    a.arena = nullptr; // DcpProblem::trellis holds the table's address
    if (c == DCP_STRIP_CLASS)
    {
      // the checkpoints of those that go in blocks, then G blocks at a time; a window that keeps its whole table (no
      // checkpoint address) is one block of the first round
      if (strip_blocks > 0) HIP_TRY(x, dcp_launch_strip_ckpt(a, x->d_ckpt_addr.p, B), DCP_EFUNCUSE);
      for (int it = 0; it == 0 || it * G < strip_blocks; ++it)
      {
        HIP_TRY(x, dcp_launch_strip_store(a, x->d_ckpt_addr.p, B, G, it), DCP_EFUNCUSE);
        HIP_TRY(x, dcp_launch_traceback(a, x->d_steps.p, x->d_step_off.p, x->d_nsteps.p, x->d_trace.p, B, G, it,
                                        x->d_ckpt_addr.p),
                DCP_EFUNCUSE);
      }
    }
    else if (G <= 1 && fused) // one launch: every window walks its own blocks (dcp_path_blocks_kernel)
      HIP_TRY(x, dcp_launch_path_blocks(c, a, x->d_ckpt_addr.p, B, x->d_steps.p, x->d_step_off.p, x->d_nsteps.p, x->d_trace.p),
              DCP_EFUNCUSE);
    else
    {
      // The checkpoints; then, G blocks at a time from the last to the first, the rows of those blocks of every
      // window -- a workgroup per (window, block): G times the wavefronts, each walking 1 / blocks of the rows --
      // and the traceback through them.  (G = 1 with DECIPHON_HIP_PATH_FUSED=0: a launch per block and phase.)
      if (max_blocks > 1) HIP_TRY(x, dcp_launch_cost_ckpt(c, a, x->d_ckpt_addr.p, B), DCP_EFUNCUSE);
      for (int it = 0; it * G < max_blocks; ++it)
      {
        HIP_TRY(x, dcp_launch_cost_store(c, a, x->d_ckpt_addr.p, B, G, it), DCP_EFUNCUSE);
        HIP_TRY(x, dcp_launch_traceback(a, x->d_steps.p, x->d_step_off.p, x->d_nsteps.p, x->d_trace.p, B, G, it), DCP_EFUNCUSE);
      }
    }
    return 0;
  });
  if (rc) return rc;
  tm.lap("traceback");
  PathFetched f;
  if ((rc = fetch_results(ps, n, 2 * (size_t)n, f))) return rc;
  tm.lap("fetch");
  for (DcpProblem const &p : st.problems)
  {
    PathResult &r = x->paths[(size_t)x->path_order[(size_t)(b + p.out)]];
    r.K = x->profiles[(size_t)p.profile].K;
    r.L = p.L;
    r.score = f.out[2 * (size_t)p.out + 1]; // the alt score of the same DP
    r.has_trellis = r.trellis_on_host = false;
    r.owned.clear();
    int32_t const ns = f.nsteps[(size_t)p.out];
    r.steps = ns >= 0 ? f.steps + f.compact[(size_t)p.out] : nullptr;
    r.nsteps = ns >= 0 ? ns : 0;
    if (ns < 0) redo.push_back(x->path_order[(size_t)(b + p.out)]);
  }
  tm.lap("results");
  if (tm.on)
    fprintf(stderr, "dcp_hip_path: %d windows, tables %.2f GB of %.2f GB held (hipMalloc %.1f ms), %zu steps, %zu to redo;%s\n",
            n, (double)x->tables.placed / 1e9, (double)x->tables.held / 1e9, x->tables.alloc_ms, f.total_steps,
            redo.size(), tm.line.c_str());
  return 0;
}

int path_run(Pass const &ps, int n, dcp_hip_window const *w)
{
  dcp_hip *const x = ps.x;
  HIP_TRY(x, hipSetDevice(x->device), DCP_EFUNCUSE);
  // (as stage() would: the literal pass lays its trellises out by the committed profiles before it stages)
  if (x->committed != x->profiles.size()) return fail(x, DCP_EFUNCUSE, "profiles not committed");
  // every window is checked here, whichever pass takes it (path_literal indexes x->profiles before stage() looks)
  for (int i = 0; i < n; ++i)
  {
    Refusal const bad = check_window(w[i], (int)x->profiles.size(), x->seqs.count(), x->seqs.seq_off.data());
    if (bad.code) return fail(x, bad.code, bad.what);
  }
  x->path_wins.assign(w, w + n);
  x->paths.resize((size_t)n);
  x->host_trellis.assign((size_t)n, std::vector<unsigned char>());
  if (n == 0) return 0;
  std::vector<int> redo;
  char const *mode = getenv("DECIPHON_HIP_PATH"); // "literal": skip the fast pass (tests, debugging)
  bool const literal_only = mode && strcmp(mode, "literal") == 0;
  if (literal_only)
    for (int i = 0; i < n; ++i) redo.push_back(i);
  else
  {
    // slowest windows first, so that the slices of quick windows do not each wait for a slow one
    // (a window's time is its rows times its class's time per row)
    std::vector<double> cost((size_t)n);
    for (int i = 0; i < n; ++i)
    {
      int const W = x->profiles[(size_t)w[i].profile].W;
      cost[(size_t)i] = (double)(w[i].stop - w[i].start) * (W == 1 ? 1.0 : W == 2 ? 2.0 : W == 4 ? 2.5 : W == 8 ? 3.0 : 4.0);
    }
    x->path_order.resize((size_t)n);
    for (int i = 0; i < n; ++i) x->path_order[(size_t)i] = i;
    std::stable_sort(x->path_order.begin(), x->path_order.end(),
                     [&](int a, int b) { return cost[(size_t)a] > cost[(size_t)b]; });
    x->path_sorted.resize((size_t)n);
    for (int i = 0; i < n; ++i) x->path_sorted[(size_t)i] = w[x->path_order[(size_t)i]];
    // slices bounded by the HBM their DP tables take
    size_t const budget = path_budget(x);
    x->path_plan = plan_path(x, DCP_PATH_FAST, x->path_sorted, budget);
    x->path_blocked += x->path_plan.blocked;
    for (int b = 0; b < n;)
    {
      int const e = (int)place_slice(x, x->path_plan, (size_t)b, budget);
      if (e == b) return fail(x, DCP_ENOMEM, "a window's DP table does not fit the device memory left");
      int rc = path_fast(ps, b, e, redo);
      if (rc) return rc;
      b = e;
    }
    std::sort(redo.begin(), redo.end());
  }
  x->path_redone = (int)redo.size();
  return path_literal(ps, redo, literal_only);
}

} // namespace

extern "C" {

int dcp_hip_path(struct dcp_hip *x, int n, struct dcp_hip_window const *w)
{
  if (!x || n < 0 || (n > 0 && !w)) return DCP_EFUNCUSE;
  // the previous results end here, whether or not this call succeeds; a failed call leaves none
  x->path_gen = UINT64_MAX;
  x->h_steps_used = 0;
  x->paths.clear();
  x->path_wins.clear();
  x->host_trellis.clear();
  x->path_table_bytes = 0;
  x->path_blocked = 0;
  // its own window lists, result buffers and streams: cost batches may be in flight
  int const rc = path_run(path_pass(x), n, w);
  if (rc)
  {
    x->paths.clear();
    x->path_wins.clear();
    x->host_trellis.clear();
    return rc;
  }
  x->path_gen = x->gen;
  return 0;
}

int dcp_hip_path_reserve(struct dcp_hip *x, int64_t bytes)
{
  if (!x || bytes < 0) return DCP_EFUNCUSE;
  HIP_TRY(x, hipSetDevice(x->device), DCP_EFUNCUSE);
  {
    // never more than a quarter of what is free right now: several scans may share the device
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && (size_t)bytes > x->tables.held + free_b / 4)
      bytes = (int64_t)(x->tables.held + free_b / 4);
  }
  if (!x->tables.hold((size_t)bytes)) return fail(x, DCP_ENOMEM, "dcp_hip_path_reserve: hipMalloc failed");
  return 0;
}

int dcp_hip_path_nsteps(struct dcp_hip const *x, int i)
{
  if (!x || i < 0 || i >= (int)x->paths.size()) return -1;
  return (int)x->paths[(size_t)i].nsteps;
}

int dcp_hip_path_steps(struct dcp_hip const *x, int i, int32_t *state_ids, int32_t *seqsizes)
{
  if (!x || i < 0 || i >= (int)x->paths.size() || !state_ids || !seqsizes) return DCP_EFUNCUSE;
  PathResult const &r = x->paths[(size_t)i];
  for (int32_t k = 0; k < r.nsteps; ++k)
  {
    state_ids[k] = (int32_t)(r.steps[k] & 0xffffu);
    seqsizes[k] = (int32_t)(r.steps[k] >> 16);
  }
  return 0;
}

int dcp_hip_path_steps_packed(struct dcp_hip const *x, int i, uint32_t const **steps, int32_t *nsteps)
{
  if (!x || i < 0 || i >= (int)x->paths.size() || !steps || !nsteps) return DCP_EFUNCUSE;
  *steps = x->paths[(size_t)i].steps;
  *nsteps = x->paths[(size_t)i].nsteps;
  return 0;
}

int dcp_hip_path_trellis(struct dcp_hip const *cx, int i, uint32_t const **xnodes, uint16_t const **nodes)
{
  dcp_hip *x = const_cast<dcp_hip *>(cx);
  if (!x || i < 0 || i >= (int)x->paths.size() || !xnodes || !nodes) return DCP_EFUNCUSE;
  // the trellis is (re)computed from the engine's inputs: they must still be those of the dcp_hip_path
  if (x->path_gen != x->gen)
    return fail(x, DCP_EFUNCUSE, x->path_gen == UINT64_MAX ? "the last dcp_hip_path failed"
                                                            : "the profiles, sequences, mode or xtrans table changed since "
                                                              "dcp_hip_path: call it again");
  HIP_TRY(x, hipSetDevice(x->device), DCP_EFUNCUSE);
  Pass const ps = path_pass(x);
  if (!x->paths[(size_t)i].has_trellis)
  {
    // The fast path pass keeps no trellis.  Somebody wants one: run the literal pass for the
    // whole batch once (its paths replace the fast ones; they are the same steps).
    std::vector<int> all((size_t)x->paths.size());
    for (size_t j = 0; j < all.size(); ++j) all[j] = (int)j;
    int rc = path_literal(ps, all);
    if (rc) return rc;
  }
  int rc = fetch_trellis(ps, i);
  if (rc) return rc;
  uint32_t const *xn = reinterpret_cast<uint32_t const *>(x->host_trellis[(size_t)i].data());
  *xnodes = xn;
  *nodes = reinterpret_cast<uint16_t const *>(xn + (x->paths[(size_t)i].L + 1));
  return 0;
}

int dcp_hip_path_redone(struct dcp_hip const *x) { return x ? x->path_redone : 0; }

int64_t dcp_hip_path_table_bytes(struct dcp_hip const *x) { return x ? x->path_table_bytes : 0; }

int dcp_hip_path_blocked(struct dcp_hip const *x) { return x ? x->path_blocked : 0; }

float dcp_hip_path_score(struct dcp_hip const *x, int i)
{
  if (!x || i < 0 || i >= (int)x->paths.size()) return NAN;
  return x->paths[(size_t)i].score;
}

} // extern "C"
