// engine.cpp -- device-resident state and the C ABI of include/deciphon_hip.h: the engine itself, its mode, the upload
// of staged window lists and their launches.  What is staged and what a cost pass launches is decided in
// stage_plan.cpp, host only (plan_stage, cost_schedule).  Sequences: engine_sequences.cpp; profiles:
// engine_profiles.cpp, engine_hmm.cpp; cost passes: engine_cost.cpp; path pass: engine_path.cpp; calibration:
// engine_calibrate.cpp; the state they share: engine_internal.h.
//
// HBM layout (one engine = one GPU):
//   pool      float[]          all profiles back to back; per profile
//                              rows[1364][4+Kp] = {null, bg, 0, 0, match[0..Kp)} | trans[8][Kp],
//                              Kp = 64*Q*W, padding = +inf (DcpProfileDev holds the offsets)
//   profiles  DcpProfileDev[]
//   code_rows DcpCodeRow[]     per sequence len+1 rows of 32 B (code_rows.h states a row; built on the GPU by
//                              the kernels of code_rows.hip, from 1 B/nt or from a seed: engine_sequences.cpp)
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

// a staged list goes up from pinned memory (see WindowLists); dev has been reserved
template <class T> int upload(dcp_hip *x, DevBuf<T> &dev, PinBuf<T> &pinned, std::vector<T> const &v, hipStream_t stream)
{
  if (v.empty()) return 0;
  HIP_TRY(x, pinned.reserve(v.size()), DCP_ENOMEM);
  memcpy(pinned.p, v.data(), v.size() * sizeof(T));
  HIP_TRY(x, hipMemcpyAsync(dev.p, pinned.p, v.size() * sizeof(T), hipMemcpyHostToDevice, stream), DCP_EFUNCUSE);
  return 0;
}

} // namespace

// Ask for a plan, reserve, upload.
int stage(Pass const &ps, int n, dcp_hip_window const *w, ArenaKind arena_kind, Staged &st, hipStream_t origin)
{
  dcp_hip *const x = ps.x;
  WindowLists &B = ps.lists;
  if (!origin) origin = ps.on.stream;
  if (n < 0 || (n > 0 && !w)) return fail(x, DCP_EFUNCUSE, "bad window array");
  if (ps.batch && ps.batch->n >= 0) return fail(x, DCP_EFUNCUSE, "a dcp_hip_cost_hits_begin is outstanding on these buffers: call dcp_hip_cost_hits_end first");
  if (x->committed != x->profiles.size()) return fail(x, DCP_EFUNCUSE, "profiles not committed");
  // DECIPHON_HIP_PACK=0 keeps every window on the one-window-per-wavefront kernels, DECIPHON_HIP_PACK_LDS=0 every pack
  // on the kernels that read their rows from global memory (tests compare, and flip them between calls)
  char const *pack_env = getenv("DECIPHON_HIP_PACK"), *lds_env = getenv("DECIPHON_HIP_PACK_LDS");
  StageInput in;
  in.n = n;
  in.w = w;
  in.profiles = x->plan_profiles.data();
  in.nprofiles = (int)x->plan_profiles.size();
  in.nseq = x->seqs.count();
  in.seq_off = x->seqs.seq_off.data();
  in.row_off = x->seqs.row_off.data();
  in.arena = arena_kind;
  in.table_addr = x->table_addr.data(); // ARENA_TABLE: the addresses the caller placed (place_slice)
  in.pack = !(pack_env && pack_env[0] == '0');
  in.pack_lds = !(lds_env && lds_env[0] == '0');
  in.shapes = pack_shapes();
  Refusal const refused = plan_stage(in, st);
  if (refused.code) return fail(x, refused.code, refused.what);
  if (st.c_begin[DCP_STRIP_CLASS + 1] > st.c_begin[DCP_STRIP_CLASS])
    HIP_TRY(x, B.d_ring.reserve((size_t)DCP_RING_SLOTS * DCP_RING_FLOATS), DCP_ENOMEM);
  int rc = ensure_xt(x, st.max_xt_row + 1);
  if (rc) return rc;
  if (ps.batch) x->staged_n = -1; // a cost pass: a batch's problem list and results are about to be replaced
  // every allocation first: after the first copy is enqueued nothing below can fail but a copy itself
  HIP_TRY(x, B.d_problems.reserve(std::max(st.problems.size(), (size_t)1)), DCP_ENOMEM);
  if (!st.packs.empty()) HIP_TRY(x, B.d_packs.reserve(st.packs.size()), DCP_ENOMEM);
  if (!st.pack_groups.empty()) HIP_TRY(x, B.d_pack_groups.reserve(st.pack_groups.size()), DCP_ENOMEM);
  if (B.up_pending) HIP_TRY(x, hipEventSynchronize(B.up_ev), DCP_EFUNCUSE); // the previous lists have gone up
  B.up_pending = false;
  if ((rc = upload(x, B.d_problems, B.h_problems, st.problems, origin))) return rc;
  if ((rc = upload(x, B.d_packs, B.h_packs, st.packs, origin))) return rc;
  if ((rc = upload(x, B.d_pack_groups, B.h_groups, st.pack_groups, origin))) return rc;
  HIP_TRY(x, hipEventRecord(B.up_ev, origin), DCP_EFUNCUSE);
  B.up_pending = true;
  return 0;
}

DcpLaunch launch_args(Pass const &ps, StagedPlan const &st, int c)
{
  dcp_hip const *const x = ps.x;
  DcpLaunch a;
  a.pool = x->d_pool.p;
  a.profiles = x->d_profiles.p;
  a.problems = ps.lists.d_problems.p + st.c_begin[c];
  a.code_rows = x->seqs.d_rows.p;
  a.xt_table = x->d_xt.p;
  a.out = ps.lists.d_out.p;
  a.arena = x->d_trellis.p;
  a.nprob = st.c_begin[c + 1] - st.c_begin[c];
  a.stream = ps.on.stream;
  a.ring = ps.lists.d_ring.p;
  return a;
}

// the device sees a pack group as an int2 (dcp_launch_cost_pack_lds), the plan as two plain int32
static_assert(sizeof(PackGroup) == sizeof(int2) && alignof(PackGroup) <= alignof(int2), "PackGroup goes up as int2");

// Cost pass: ask for the schedule (cost_schedule, stage_plan.h: which kernels, in which order, on which branches), run
// it.  Everything is forked from `origin` (the stream the window lists were uploaded on; the pass's own by default) and
// joined into the pass's stream.
int launch_cost_all(Pass const &ps, StagedPlan const &st, hipStream_t origin)
{
  dcp_hip *const x = ps.x;
  if (!origin) origin = ps.on.stream;
  // DECIPHON_HIP_NARROW=0: the class's kernel for all its windows (tests compare)
  char const *narrow_env = getenv("DECIPHON_HIP_NARROW");
  // DECIPHON_HIP_XCD_PLACEMENT=plain | eighths: every class's cost kernel that way (measurements, tests); auto, or
  // not set: dcp_xcd_placement decides per launch
  int placement = DCP_PLACE_AUTO;
  if (char const *e = getenv("DECIPHON_HIP_XCD_PLACEMENT"))
  {
    if (!strcmp(e, "plain")) placement = DCP_PLACE_PLAIN;
    else if (!strcmp(e, "eighths")) placement = DCP_PLACE_EIGHTHS;
    else if (strcmp(e, "auto")) return fail(x, DCP_EFUNCUSE, "DECIPHON_HIP_XCD_PLACEMENT is not plain, eighths or auto");
  }
  std::vector<CostLaunch> const schedule = cost_schedule(st, !(narrow_env && narrow_env[0] == '0'));
  x->last_cost_launches = schedule; // what dcp_hip_last_cost_launches reports: the loop below runs exactly this
  // the pass's stream joins the kernels only after the last launch (Fork::join): a wait is a barrier in its hardware
  // queue, and a stream that shares that queue would start its kernel behind every barrier issued before
  // (profiles/r02_step_timeline.txt)
  Fork fk(ps, schedule.size() > 1 || origin != ps.on.stream);
  int rc = fk.begin(origin);
  if (rc) return rc;
  WindowLists &B = ps.lists;
  uint32_t const ncode_rows = (uint32_t)x->seqs.code_rows();
  for (CostLaunch const &e : schedule)
  {
    Branch const &branch = (e.branch == BRANCH_NARROW ? x->narrow_branch : e.branch == BRANCH_PACK ? x->pack_branch : ps.on.cls_branch)[e.index];
    DcpLaunch a = launch_args(ps, st, 0);
    if ((rc = fk.enter(branch, a))) return rc;
    a.problems = B.d_problems.p + e.first; // (the pack kernels do not read them)
    a.nprob = e.count;
    a.windows_per_profile = e.windows_per_profile;
    a.placement = placement;
    hipError_t err = hipSuccess;
    switch (e.kernel)
    {
    case COST_CLASS: err = dcp_launch_cost(e.index, a); break;
    case COST_NARROW: err = dcp_launch_cost_narrow(e.index, a); break;
    case COST_FUSED: err = dcp_launch_cost_fused(a); break;
    case COST_PACK: err = dcp_launch_cost_pack(e.index, a, B.d_packs.p + e.first, e.count, ncode_rows); break;
    case COST_PACK_LDS:
      err = dcp_launch_cost_pack_lds(e.index, a, B.d_packs.p + st.pk_begin[e.index],
                                     reinterpret_cast<int2 const *>(B.d_pack_groups.p + e.first), e.count, ncode_rows);
      break;
    default: break; // COST_NONE
    }
    if (err != hipSuccess) return fail(x, DCP_EFUNCUSE, "cost kernel launch", err);
    if ((rc = fk.leave(branch))) return rc;
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
  bool ok = hipStreamCreateWithFlags(&x->cost_set.stream, hipStreamNonBlocking) == hipSuccess;
  ok = ok && hipEventCreateWithFlags(&x->cost_set.fork_ev, hipEventDisableTiming) == hipSuccess;
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
  for (int c = 0; ok && c < DCP_NUM_CLASSES; ++c) ok = create_branch(x->cost_set.cls_branch[c], c >= prio_from ? prio_high : 0);
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
  for (Batch &b : x->batch)
  {
    ok = ok && hipEventCreateWithFlags(&b.done_ev, hipEventDisableTiming) == hipSuccess;
    ok = ok && hipEventCreateWithFlags(&b.up_ev, hipEventDisableTiming) == hipSuccess;
  }
  ok = ok && hipEventCreateWithFlags(&x->path_lists.up_ev, hipEventDisableTiming) == hipSuccess;
  if (!ok)
  {
    dcp_hip_del(x);
    return nullptr;
  }
  return x;
}

void dcp_hip_del(struct dcp_hip *x)
{
  if (!x) return;
  (void)hipSetDevice(x->device);
  (void)hipDeviceSynchronize(); // batches begun and never ended included
  for (int c = 0; c < DCP_NUM_CLASSES; ++c)
  {
    destroy_branch(x->cost_set.cls_branch[c]);
    destroy_branch(x->narrow_branch[c]);
    destroy_branch(x->path_set.cls_branch[c]);
  }
  for (int s = 0; s < DCP_NUM_PACK_SHAPES; ++s) destroy_branch(x->pack_branch[s]);
  if (x->path_set.stream) (void)hipStreamDestroy(x->path_set.stream);
  if (x->path_set.fork_ev) (void)hipEventDestroy(x->path_set.fork_ev);
  if (x->upload_stream) (void)hipStreamDestroy(x->upload_stream);
  for (Batch &b : x->batch)
  {
    if (b.done_ev) (void)hipEventDestroy(b.done_ev);
    if (b.up_ev) (void)hipEventDestroy(b.up_ev);
  }
  if (x->path_lists.up_ev) (void)hipEventDestroy(x->path_lists.up_ev);
  if (x->cost_set.fork_ev) (void)hipEventDestroy(x->cost_set.fork_ev);
  if (x->cost_set.stream) (void)hipStreamDestroy(x->cost_set.stream);
  delete x;
}

char const *dcp_hip_strerror(struct dcp_hip const *x) { return x ? x->err.c_str() : "no engine"; }

int dcp_hip_encode(char const *data, int64_t n, uint8_t *out)
{
  if (n < 0 || (n > 0 && (!data || !out))) return DCP_EFUNCUSE;
  return dcp_encode_sequence(data, n, out);
}

int dcp_hip_set_mode(struct dcp_hip *x, int multi_hits, int hmmer3_compat)
{
  if (!x) return DCP_EFUNCUSE;
  if (outstanding_batches(x)) return refuse_outstanding(x);
  bool mh = multi_hits != 0, h3 = hmmer3_compat != 0;
  ++x->gen;
  drop_calibration(x);
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
  drop_calibration(x);
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
