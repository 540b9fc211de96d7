// engine_path.cpp -- the path pass of the C ABI: the fast pass over DP tables in blocks, the literal pass, the results.
#include "engine_internal.h"

namespace
{

// for functions that enqueue copies from vectors of their own: whichever way they leave, the stream has passed the
// copies before the vectors go (a no-op when the function has synchronised already)
struct StreamDrain
{
  hipStream_t s;
  ~StreamDrain() { (void)hipStreamSynchronize(s); }
};

// The fast path pass in blocks (dcp_types.h): rows between checkpoints.  DECIPHON_HIP_CKPT_ROWS overrides (tests
// use small blocks; 0 = whole windows, the tables of round 1); always a multiple of 5.
int ckpt_rows()
{
  int B = DCP_CKPT_ROWS_DEFAULT;
  if (char const *e = getenv("DECIPHON_HIP_CKPT_ROWS")) B = atoi(e);
  if (B < 0) B = 0;
  return B - B % 5;
}
// one block's table, then the window's checkpoints (16-byte aligned)
size_t block_table_bytes(int L, int Kp, int B) { return (size_t)dcp_block_slots(L, B) * (DCP_SP_STRIDE + 3 * (size_t)Kp) * 4; }
// (strip: a window of the strip class, whose checkpoints carry B of five rows as well)
size_t ckpt_bytes(int L, int Kp, int W, int B, bool strip = false)
{
  return (size_t)(dcp_num_blocks(L, B) - 1) * (size_t)(strip ? dcp_strip_ckpt_floats(Kp, W) : dcp_ckpt_floats(Kp, W)) * 4;
}
// the G tables of a window whose G blocks are computed at once (dcp_cost_store_kernel); its checkpoints come behind them
size_t group_tables_bytes(int L, int Kp, int B, int G)
{
  return ((size_t)std::min(G, dcp_num_blocks(L, B)) * block_table_bytes(L, Kp, B) + 15) & ~(size_t)15;
}
size_t fast_bytes(int L, int Kp, int W, int B, int G = 1, bool strip = false)
{
  return group_tables_bytes(L, Kp, B, G) + ckpt_bytes(L, Kp, W, B, strip);
}

// Does this window of the strip class go in blocks?  `whole` = what it takes otherwise: its whole table (fast pass),
// or that and the replay scratch of all its rows (literal pass).  Where that fits the budget the window keeps it: its
// rows are walked once instead of twice.  Where it does not the window is taken a block at a time like every other
// class -- unless the budget is strict: DECIPHON_HIP_PATH_STRICT=1 refuses a strip window whose WHOLE table exceeds the
// budget, as it always has (its block table might fit; the rule is kept because callers and tests rely on it).
bool strip_in_blocks(size_t whole, int B, size_t budget) { return B > 0 && whole > budget && !path_budget_strict(); }

// The G block tables, the checkpoints and (literal pass) the replay scratch of a window are ONE placement, and a
// placement lies in one chunk of the arena.  Once the arena holds chunks -- dcp_hip_path_reserve sets the whole budget
// aside in chunks of TableArena::CHUNK -- a placement beyond the largest of them would be allocated on top of what is
// held, outside the budget: G is held to what a chunk takes.  per_block, fixed: bytes of one more block, of the rest.
int group_chunk_cap(dcp_hip const *x, size_t per_block, size_t fixed)
{
  size_t const chunk = x->tables.largest_chunk();
  if (chunk == 0 || per_block == 0) return INT32_MAX; // nothing held yet: the first chunk is made to measure
  size_t const slack = 1024; // the alignments of group_tables_bytes and TableArena::place
  return chunk > fixed + slack + per_block ? (int)std::min<size_t>((chunk - fixed - slack) / per_block, (size_t)INT32_MAX) : 1;
}

// How many blocks of a window go side by side: what 90 % of the budget holds of them at `one` bytes each beside
// `fixed`, no more than the window with the most blocks has (`most`) or a chunk takes (`cap`, group_chunk_cap).
// DECIPHON_HIP_PATH_GROUP overrides.
int group_size(size_t budget, double fixed, double one, int most, int cap)
{
  double const room = 0.9 * (double)budget - fixed;
  int G = one > 0 && room > one ? (int)std::min<double>(room / one, (double)most) : 1;
  G = std::min(G, cap);
  if (char const *e = getenv("DECIPHON_HIP_PATH_GROUP")) G = std::max(atoi(e), 1);
  return std::max(1, std::min(G, most));
}

void note_placed(dcp_hip *x) { x->path_table_bytes = std::max(x->path_table_bytes, (int64_t)x->tables.placed); }

// the path pass works on its own bank and streams (see dcp_hip::bank): swapped in for the duration of a call
struct PathContext
{
  dcp_hip *x;
  int saved_cur;
  static void swap_streams(dcp_hip *x)
  {
    std::swap(x->stream, x->path_set.stream);
    std::swap(x->fork_ev, x->path_set.fork_ev);
    std::swap(x->cls_branch, x->path_set.cls_branch);
  }
  explicit PathContext(dcp_hip *x_) : x(x_), saved_cur(x_->cur)
  {
    swap_streams(x);
    x->cur = 2;
  }
  ~PathContext()
  {
    swap_streams(x);
    x->cur = saved_cur;
  }
};

// step buffers: a path has at most L emitting steps; mute steps (S, B, E, T, D runs) are few
// in practice.  DECIPHON_HIP_UNZIP_CAP (steps) overrides the capacity: a test hook for the
// overflow fallbacks.
// step_off (the caller keeps it until the stream has passed the copy) goes to the device with the buffers it describes.
int stage_steps(dcp_hip *x, Staged const &st, int n, std::vector<int64_t> &step_off)
{
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
                            hipMemcpyHostToDevice, x->stream),
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
int fetch_results(dcp_hip *x, int n, size_t nout, PathFetched &f)
{
  HIP_TRY(x, x->h_out.reserve(nout), DCP_ENOMEM);
  HIP_TRY(x, hipMemcpyAsync(x->h_out.p, BK(x).d_out.p, nout * sizeof(float), hipMemcpyDeviceToHost, x->stream), DCP_EFUNCUSE);
  f.out = x->h_out.p;
  HIP_TRY(x, x->h_nsteps.reserve((size_t)std::max(n, 1)), DCP_ENOMEM);
  HIP_TRY(x, hipMemcpyAsync(x->h_nsteps.p, x->d_nsteps.p, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, x->stream),
          DCP_EFUNCUSE);
  HIP_TRY(x, hipStreamSynchronize(x->stream), DCP_EFUNCUSE);
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
                            x->stream),
          DCP_EFUNCUSE);
  HIP_TRY(x, dcp_launch_compact_steps(x->d_steps.p, x->d_step_off.p, x->d_compact_off.p, x->d_compact.p, n, x->stream),
          DCP_EFUNCUSE);
  HIP_TRY(x, hipMemcpyAsync(h_steps.p, x->d_compact.p, total * sizeof(uint32_t), hipMemcpyDeviceToHost, x->stream),
          DCP_EFUNCUSE);
  HIP_TRY(x, hipStreamSynchronize(x->stream), DCP_EFUNCUSE);
  f.steps = h_steps.p;
  return 0;
}

int fetch_trellis(dcp_hip *x, int i)
{
  PathResult &r = x->paths[(size_t)i];
  if (r.trellis_on_host) return 0;
  std::vector<unsigned char> &buf = x->host_trellis[(size_t)i];
  size_t const bytes = ((size_t)r.L + 1) * 4 + ((size_t)r.L + 1) * (size_t)r.K * 2;
  buf.resize(bytes);
  HIP_TRY(x, hipMemcpyAsync(buf.data(), x->d_trellis.p + r.trellis_off, bytes, hipMemcpyDeviceToHost, x->stream),
          DCP_EFUNCUSE);
  HIP_TRY(x, hipStreamSynchronize(x->stream), DCP_EFUNCUSE);
  r.trellis_on_host = true;
  return 0;
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

// The literal pass of the profiles beyond 4096 positions (strip class): the register-resident path kernel does not
// reach them; their trellis is replayed row by row from the DP table (row_replay.h), into d_trellis at trel_off[j] for
// window w[sl[..]] = j, its score into slot j of d_out.  The tables are placed slice by slice within the budget like
// the fast pass's.  A window keeps its whole table, with (L + 1) * 3 * K floats of scratch, where the two fit the
// budget; where they do not -- and the budget is not strict, see strip_in_blocks -- the table comes a block at a time
// from checkpoints, G blocks side by side, and a block serves the rows of the traceback's partition (dcp_types.h).
// count_blocked: the windows taken in blocks go into x->path_blocked (a dcp_hip_path whose fast pass was skipped).
int literal_strips(dcp_hip *x, std::vector<dcp_hip_window> const &w, std::vector<int> const &sl,
                   std::vector<size_t> const &trel_off, bool count_blocked)
{
  int const n = (int)w.size();
  size_t const budget = path_budget(x);
  int const B = ckpt_rows();
  auto const scratch_bytes = [](int rows, int K) { return (size_t)rows * 3 * (size_t)K * sizeof(float); };
  auto const aligned = [](size_t bytes) { return (bytes + 255) & ~(size_t)255; };
  std::vector<char> blocked(sl.size(), 0);
  int G = 1;
  {
    // as many blocks side by side as the budget holds for the window that needs the most
    double fixed = 0, one = 0;
    int most = 1, cap = INT32_MAX;
    for (size_t i = 0; i < sl.size(); ++i)
    {
      dcp_hip_window const &v = w[(size_t)sl[i]];
      HostProfile const &hp = x->profiles[(size_t)v.profile];
      int const L = v.stop - v.start;
      if (L < 1) return fail(x, DCP_EZEROSEQ, "empty window");
      blocked[i] = strip_in_blocks(aligned(table_bytes(L, hp.Kp)) + scratch_bytes(L + 1, hp.K), B, budget);
      if (!blocked[i]) continue;
      size_t const per_block = block_table_bytes(L, hp.Kp, B) + scratch_bytes(dcp_replay_block_rows(B), hp.K);
      fixed = std::max(fixed, (double)ckpt_bytes(L, hp.Kp, hp.W, B, true));
      one = std::max(one, (double)per_block);
      most = std::max(most, dcp_num_blocks(L, B));
      cap = std::min(cap, group_chunk_cap(x, per_block, ckpt_bytes(L, hp.Kp, hp.W, B, true)));
      if (count_blocked) ++x->path_blocked;
    }
    G = group_size(budget, fixed, one, most, cap);
  }
  HIP_TRY(x, x->d_aux.reserve(4 * sl.size()), DCP_ENOMEM);
  for (size_t sb = 0; sb < sl.size();)
  {
    size_t se = sb;
    x->tables.reset();
    x->table_addr.clear();
    std::vector<dcp_hip_window> ws;
    std::vector<int64_t> aux; // [4][windows of the slice]: trellis, scratch, checkpoints, score slot
    std::vector<int64_t> scr, ckp;
    int max_rows = 0, max_blocks = 0;
    for (; se < sl.size(); ++se)
    {
      dcp_hip_window const &v = w[(size_t)sl[se]];
      HostProfile const &hp = x->profiles[(size_t)v.profile];
      int const L = v.stop - v.start;
      // one placement per window: its table(s), then the checkpoints, then the scratch
      size_t const tables = aligned(blocked[se] ? fast_bytes(L, hp.Kp, hp.W, B, G, true) : table_bytes(L, hp.Kp));
      int const nb = blocked[se] ? dcp_num_blocks(L, B) : 1;
      int const rows = blocked[se] ? std::min(G, nb) * dcp_replay_block_rows(B) : L + 1;
      unsigned char *t = x->tables.place(tables + scratch_bytes(rows, hp.K), budget);
      if (!t) break;
      x->table_addr.push_back((int64_t)(uintptr_t)t);
      ws.push_back(v);
      scr.push_back((int64_t)(uintptr_t)(t + tables));
      ckp.push_back(blocked[se] ? (int64_t)(uintptr_t)t + (int64_t)group_tables_bytes(L, hp.Kp, B, G) : 0);
      max_rows = std::max(max_rows, rows);
      if (blocked[se]) max_blocks = std::max(max_blocks, nb);
    }
    if (se == sb) return fail(x, DCP_ENOMEM, "no device memory for the DP table of a long profile's path pass");
    note_placed(x);
    int const ns = (int)ws.size();
    Staged ss;
    int rc = stage(x, ns, ws.data(), ARENA_TABLE, ss);
    if (rc) return rc;
    aux.resize(4 * (size_t)ns);
    for (int i = 0; i < ns; ++i)
    {
      int const j = sl[sb + (size_t)i];
      aux[(size_t)i] = (int64_t)(uintptr_t)(x->d_trellis.p + trel_off[(size_t)j]);
      aux[(size_t)ns + i] = scr[(size_t)i];
      aux[2 * (size_t)ns + i] = ckp[(size_t)i];
      aux[3 * (size_t)ns + i] = j;
    }
    HIP_TRY(x, hipMemcpyAsync(x->d_aux.p, aux.data(), aux.size() * sizeof(int64_t), hipMemcpyHostToDevice, x->stream),
            DCP_EFUNCUSE);
    DcpLaunch a = launch_args(x, ss, DCP_STRIP_CLASS);
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
    HIP_TRY(x, hipStreamSynchronize(x->stream), DCP_EFUNCUSE); // aux is read by the copy above; the next slice reuses the tables
    sb = se;
  }
  return 0;
}

// The literal path pass (viterbi_path as the reference runs it, pass by pass, with the
// trellis in HBM) + trellis_unzip on the device, for the windows path_wins[idx[..]].
int path_literal(dcp_hip *x, std::vector<int> const &idx, bool count_blocked = false)
{
  int const n = (int)idx.size();
  if (n == 0) return 0;
  std::vector<dcp_hip_window> w((size_t)n);
  for (int j = 0; j < n; ++j) w[(size_t)j] = x->path_wins[(size_t)idx[(size_t)j]];
  // where stage() will put every window's trellis (ARENA_TRELLIS)
  std::vector<size_t> trel_off((size_t)n + 1, 0);
  std::vector<int> sl; // the windows of the strip class
  for (int j = 0; j < n; ++j)
  {
    HostProfile const &hp = x->profiles[(size_t)w[(size_t)j].profile];
    int const L = w[(size_t)j].stop - w[(size_t)j].start;
    trel_off[(size_t)j + 1] = trel_off[(size_t)j] + trellis_stride(std::max(L, 0), hp.K);
    if (hp.cls == DCP_STRIP_CLASS) sl.push_back(j);
  }
  HIP_TRY(x, BK(x).d_out.reserve(3 * (size_t)n), DCP_ENOMEM);
  HIP_TRY(x, x->d_trellis.reserve(trel_off[(size_t)n]), DCP_ENOMEM);
  int rc = 0;
  // the strip class first: the problem list below replaces its lists on the device
  if (!sl.empty() && (rc = literal_strips(x, w, sl, trel_off, count_blocked))) return rc;
  Staged st;
  if ((rc = stage(x, n, w.data(), ARENA_TRELLIS, st))) return rc;
  if (st.arena_bytes != trel_off[(size_t)n]) return fail(x, DCP_EFUNCUSE, "trellis arena laid out otherwise than expected");
  if ((rc = launch_all(x, st, true))) return rc; // (not the strip class)

  std::vector<int64_t> step_off;
  if ((rc = stage_steps(x, st, n, step_off))) return rc;
  {
    DcpLaunch a = launch_args(x, st, 0);
    a.problems = BK(x).d_problems.p;
    a.nprob = n;
    HIP_TRY(x, dcp_launch_unzip(a, x->d_steps.p, x->d_step_off.p, x->d_nsteps.p), DCP_EFUNCUSE);
  }
  PathFetched f;
  if ((rc = fetch_results(x, n, (size_t)n, f))) return rc;
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
      if ((rc = fetch_trellis(x, i))) return rc;
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
int path_fast(dcp_hip *x, int b, int e, std::vector<int> &redo)
{
  int const n = e - b;
  Stopwatch tm(x->stream);
  Staged st;
  int rc = stage(x, n, x->path_sorted.data() + b, ARENA_TABLE, st);
  if (rc) return rc;
  tm.lap("stage");
  HIP_TRY(x, BK(x).d_out.reserve(2 * (size_t)n), DCP_ENOMEM);
  int const B = ckpt_rows();
  // checkpoints sit behind each window's block table (dcp_hip_path placed fast_bytes per window)
  std::vector<int64_t> ckpt_addr((size_t)n, 0), step_off;
  StreamDrain drain{x->stream}; // destroyed before the two: an early return does not pull them from under a copy
  int max_blocks = 1, strip_blocks = 0; // strip_blocks > 0: windows of the strip class that go in blocks
  for (DcpProblem const &p : st.problems)
  {
    HostProfile const &hp = x->profiles[(size_t)p.profile];
    // (a window of the strip class that keeps its whole table has no checkpoints: address 0, dcp_hip_path placed
    // table_bytes for it)
    if (hp.cls == DCP_STRIP_CLASS && !x->path_in_blocks[(size_t)(b + p.out)]) continue;
    int const nb = dcp_num_blocks(p.L, B);
    ckpt_addr[(size_t)p.out] = p.trellis + (int64_t)group_tables_bytes(p.L, hp.Kp, B, x->path_group);
    int &most = hp.cls == DCP_STRIP_CLASS ? strip_blocks : max_blocks;
    most = std::max(most, nb);
  }
  HIP_TRY(x, x->d_ckpt_addr.reserve((size_t)n), DCP_ENOMEM);
  HIP_TRY(x, hipMemcpyAsync(x->d_ckpt_addr.p, ckpt_addr.data(), (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice, x->stream),
          DCP_EFUNCUSE);
  HIP_TRY(x, x->d_trace.reserve((size_t)n), DCP_ENOMEM);
  HIP_TRY(x, hipMemsetAsync(x->d_trace.p, 0, (size_t)n * sizeof(DcpTraceState), x->stream), DCP_EFUNCUSE);
  if ((rc = stage_steps(x, st, n, step_off))) return rc;
  // the classes of a slice are each too small to fill the GPU and each lasts as long as its longest window:
  // they go out on their own streams, forked from and joined back into x->stream
  int classes = 0;
  for (int c = 0; c < DCP_NUM_CLASSES; ++c) classes += st.c_begin[c + 1] > st.c_begin[c];
  Fork fk(x, classes > 1);
  // The checkpoints of the windows that have more than one block, then the blocks from the last to the first.
  // Every class does that on its own stream -- checkpoints, then per block its rows and the traceback through it --
  // without waiting for the others: a class's windows are done when ITS slowest is, and the store kernel of one
  // class runs beside the traceback of another (one join at the end).
  {
    char const *fused_env = getenv("DECIPHON_HIP_PATH_FUSED");
    bool const fused = !(fused_env && fused_env[0] == '0');
    if ((rc = fk.begin(x->stream))) return rc;
    for (int c = 0; c < DCP_NUM_CLASSES; ++c)
    {
      DcpLaunch a = launch_args(x, st, c);
      if (a.nprob <= 0) continue;
      a.arena = nullptr; // DcpProblem::trellis holds the table's address
      if ((rc = fk.enter(x->cls_branch[c], a))) return rc;
      if (c == DCP_STRIP_CLASS)
      {
        // the checkpoints of those that go in blocks, then G blocks at a time; a window that keeps its whole table (no
        // checkpoint address) is one block of the first round
        int const G = std::max(x->path_group, 1);
        if (strip_blocks > 0) HIP_TRY(x, dcp_launch_strip_ckpt(a, x->d_ckpt_addr.p, B), DCP_EFUNCUSE);
        for (int it = 0; it == 0 || it * G < strip_blocks; ++it)
        {
          HIP_TRY(x, dcp_launch_strip_store(a, x->d_ckpt_addr.p, B, G, it), DCP_EFUNCUSE);
          HIP_TRY(x, dcp_launch_traceback(a, x->d_steps.p, x->d_step_off.p, x->d_nsteps.p, x->d_trace.p, B, G, it,
                                          x->d_ckpt_addr.p),
                  DCP_EFUNCUSE);
        }
      }
      else if (x->path_group <= 1 && fused) // one launch: every window walks its own blocks (dcp_path_blocks_kernel)
        HIP_TRY(x, dcp_launch_path_blocks(c, a, x->d_ckpt_addr.p, B, x->d_steps.p, x->d_step_off.p, x->d_nsteps.p, x->d_trace.p),
                DCP_EFUNCUSE);
      else
      {
        // The checkpoints; then, G blocks at a time from the last to the first, the rows of those blocks of every
        // window -- a workgroup per (window, block): G times the wavefronts, each walking 1 / blocks of the rows --
        // and the traceback through them.  (G = 1 with DECIPHON_HIP_PATH_FUSED=0: a launch per block and phase.)
        int const G = std::max(x->path_group, 1);
        if (max_blocks > 1) HIP_TRY(x, dcp_launch_cost_ckpt(c, a, x->d_ckpt_addr.p, B), DCP_EFUNCUSE);
        for (int it = 0; it * G < max_blocks; ++it)
        {
          HIP_TRY(x, dcp_launch_cost_store(c, a, x->d_ckpt_addr.p, B, G, it), DCP_EFUNCUSE);
          HIP_TRY(x, dcp_launch_traceback(a, x->d_steps.p, x->d_step_off.p, x->d_nsteps.p, x->d_trace.p, B, G, it), DCP_EFUNCUSE);
        }
      }
      if ((rc = fk.leave(x->cls_branch[c]))) return rc;
    }
    if ((rc = fk.join())) return rc;
  }
  tm.lap("traceback");
  PathFetched f;
  if ((rc = fetch_results(x, n, 2 * (size_t)n, f))) return rc;
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

int path_run(dcp_hip *x, int n, dcp_hip_window const *w)
{
  HIP_TRY(x, hipSetDevice(x->device), DCP_EFUNCUSE);
  PathContext ctx(x); // its own window lists, result buffers and streams: cost batches may be in flight
  // every window is checked here, whichever pass takes it (path_literal indexes x->profiles before stage() looks)
  int const nseq = (int)x->seq_off.size() - 1;
  for (int i = 0; i < n; ++i)
  {
    if (w[i].profile < 0 || w[i].profile >= (int)x->profiles.size()) return fail(x, DCP_EFUNCUSE, "bad profile index");
    if (w[i].seq < 0 || w[i].seq >= nseq) return fail(x, DCP_EFUNCUSE, "bad sequence index");
    int64_t const len = x->seq_off[(size_t)w[i].seq + 1] - x->seq_off[(size_t)w[i].seq];
    if (w[i].start < 0 || w[i].stop < w[i].start || w[i].stop > len) return fail(x, DCP_EFUNCUSE, "bad window range");
  }
  x->path_wins.assign(w, w + n);
  x->paths.resize((size_t)n);
  x->host_trellis.assign((size_t)n, std::vector<unsigned char>());
  if (n == 0) return 0;
  std::vector<int> redo;
  char const *mode = getenv("DECIPHON_HIP_PATH"); // "literal": skip the fast pass (tests, debugging)
  bool const literal_only = mode && strcmp(mode, "literal") == 0;
  x->path_in_blocks.clear();
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
    int const B = ckpt_rows();
    dcp_hip_window const *ws = x->path_sorted.data();
    // How many blocks of a window are computed side by side: as many as the budget holds tables for, for ALL the
    // windows of the request at once -- with few hits every block of every window (the rows of a window are then
    // walked once by one wavefront, for the checkpoints, and once by many); with many hits one (a slice of windows
    // fills the GPU by itself).  DECIPHON_HIP_PATH_GROUP overrides.
    {
      double one = 0, fixed = 0;
      int most = 1, cap = INT32_MAX;
      x->path_in_blocks.assign((size_t)n, 0);
      for (int i = 0; i < n; ++i)
      {
        HostProfile const &hp = x->profiles[(size_t)ws[i].profile];
        int const L = ws[i].stop - ws[i].start;
        bool const strip = hp.cls == DCP_STRIP_CLASS;
        if (strip && !strip_in_blocks(table_bytes(L, hp.Kp), B, budget))
          fixed += (double)table_bytes(L, hp.Kp);
        else
        {
          x->path_in_blocks[(size_t)i] = strip;
          x->path_blocked += strip;
          one += (double)block_table_bytes(L, hp.Kp, B);
          fixed += (double)ckpt_bytes(L, hp.Kp, hp.W, B, strip);
          most = std::max(most, dcp_num_blocks(L, B));
          cap = std::min(cap, group_chunk_cap(x, block_table_bytes(L, hp.Kp, B), ckpt_bytes(L, hp.Kp, hp.W, B, strip)));
        }
      }
      x->path_group = group_size(budget, fixed, one, most, cap);
    }
    for (int b = 0; b < n;)
    {
      int e = b;
      x->tables.reset();
      x->table_addr.clear();
      while (e < n)
      {
        // the block tables and the checkpoints (dcp_types.h); beyond 4096 positions the whole table where it fits
        HostProfile const &hp = x->profiles[(size_t)ws[e].profile];
        int const L = ws[e].stop - ws[e].start;
        bool const strip = hp.cls == DCP_STRIP_CLASS;
        unsigned char *at = x->tables.place(strip && !x->path_in_blocks[(size_t)e]
                                                ? table_bytes(L, hp.Kp)
                                                : fast_bytes(L, hp.Kp, hp.W, B, x->path_group, strip),
                                            budget);
        if (!at) break;
        x->table_addr.push_back((int64_t)(uintptr_t)at);
        ++e;
      }
      if (e == b) return fail(x, DCP_ENOMEM, "a window's DP table does not fit the device memory left");
      note_placed(x);
      int rc = path_fast(x, b, e, redo);
      if (rc) return rc;
      b = e;
    }
    std::sort(redo.begin(), redo.end());
  }
  x->path_redone = (int)redo.size();
  return path_literal(x, redo, literal_only);
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
  int const rc = path_run(x, n, w);
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
  x->tables.reset();
  // place() allocates chunk after chunk until the arena holds `bytes`
  while (x->tables.held < (size_t)bytes)
  {
    size_t const step = std::min(TableArena::CHUNK, (size_t)bytes - x->tables.held);
    size_t const before = x->tables.held;
    x->tables.cur = x->tables.chunks.size(); // past every chunk: force a new one
    if (!x->tables.place(step, x->tables.held + step) || x->tables.held == before)
      return fail(x, DCP_ENOMEM, "dcp_hip_path_reserve: hipMalloc failed");
  }
  x->tables.reset();
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
  PathContext ctx(x);
  if (!x->paths[(size_t)i].has_trellis)
  {
    // The fast path pass keeps no trellis.  Somebody wants one: run the literal pass for the
    // whole batch once (its paths replace the fast ones; they are the same steps).
    std::vector<int> all((size_t)x->paths.size());
    for (size_t j = 0; j < all.size(); ++j) all[j] = (int)j;
    int rc = path_literal(x, all);
    if (rc) return rc;
  }
  int rc = fetch_trellis(x, i);
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
