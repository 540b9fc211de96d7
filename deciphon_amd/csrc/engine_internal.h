// engine_internal.h -- the engine's state and what its translation units share (engine.cpp, engine_sequences.cpp,
// engine_profiles.cpp, engine_hmm.cpp, engine_cost.cpp, engine_path.cpp, engine_calibrate.cpp).  Everything here but
// struct dcp_hip has C++ linkage in namespace dcp_engine, which exports.map keeps inside the library.  What a staged
// window list holds (Staged, StagedPlan) and how it is planned: stage_plan.h, host only.
#pragma once
#include "../../include/deciphon_hip.h"
#include "dcp_db.h"
#include "dcp_errors.h"
#include "dcp_types.h"
#include "host_logic.h"
#include "path_plan.h"
#include "stage_plan.h"
#include "viterbi_kernels.h"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <deque>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <thread>
#include <vector>

namespace dcp_engine
{

template <class T> struct DevBuf
{
  T *p = nullptr;
  size_t cap = 0; // elements
  ~DevBuf() { release(); }
  void release()
  {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
  hipError_t reserve(size_t n)
  {
    if (n <= cap) return hipSuccess;
    release();
    size_t want = n + n / 8 + 64;
    hipError_t e = hipMalloc((void **)&p, want * sizeof(T));
    if (e != hipSuccess)
    {
      p = nullptr;
      return e;
    }
    cap = want;
    return hipSuccess;
  }
};

// Pinned host memory for results that come back while other batches are in flight: a device-to-host copy into
// PAGEABLE memory waits for everything the device has been given (measured: the 19 KB hit list of one batch took
// 370 ms, the rest of the next batch's cost pass), a copy into pinned memory only for its own stream.
template <class T> struct PinBuf
{
  T *p = nullptr;
  size_t cap = 0;
  ~PinBuf()
  {
    if (p) (void)hipHostFree(p);
  }
  hipError_t reserve(size_t n) { return n <= cap ? hipSuccess : reserve_exact(n + n / 4 + 1024); }
  // exactly `want` elements: for a buffer sized once (reserve() adds a quarter, for those that grow from call to call)
  hipError_t reserve_exact(size_t want)
  {
    if (p) (void)hipHostFree(p);
    p = nullptr;
    cap = 0;
    hipError_t const e = hipHostMalloc((void **)&p, want * sizeof(T), hipHostMallocDefault);
    if (e != hipSuccess)
    {
      p = nullptr;
      return e;
    }
    cap = want;
    return hipSuccess;
  }
};

// an event that is destroyed with its owner
struct Event
{
  hipEvent_t e = nullptr;
  Event() = default;
  Event(Event const &) = delete;
  Event &operator=(Event const &) = delete;
  ~Event()
  {
    if (e) (void)hipEventDestroy(e);
  }
  hipError_t create(unsigned flags = hipEventDefault) { return hipEventCreateWithFlags(&e, flags); }
};

// Waits for the stream when it goes: declared behind the pinned buffers and events that queued work uses, so that an
// early return after queuing drains the stream before they are freed.
struct StreamDrain
{
  hipStream_t q;
  ~StreamDrain() { (void)hipStreamSynchronize(q); }
};

// DECIPHON_HIP_STAGE_MB: bytes of a pinned staging chunk (at least 1 MiB), `unset` without it.  The callers convert to
// their own unit and apply their own floor.
inline size_t stage_bytes(size_t unset)
{
  char const *e = getenv("DECIPHON_HIP_STAGE_MB");
  return e ? (size_t)std::max(atol(e), 1L) << 20 : unset;
}

// DECIPHON_HIP_COST_ORDER, read at ingest: 0 = no cost-order copies; "poison" = copies, and the canonical match columns
// of those profiles staged as 0 (a test's proof that the narrow kernels read the copy: their scores stay the oracle's).
enum CostOrder { COST_ORDER_OFF, COST_ORDER_ON, COST_ORDER_POISON };
inline CostOrder cost_order_mode()
{
  char const *e = getenv("DECIPHON_HIP_COST_ORDER");
  if (!e) return COST_ORDER_ON;
  if (e[0] == '0') return COST_ORDER_OFF;
  return strcmp(e, "poison") == 0 ? COST_ORDER_POISON : COST_ORDER_ON;
}

// DECIPHON_HIP_PATH_STRICT=1: the path pass's budget is a hard limit (what exceeds it is a DCP_ENOMEM)
inline bool path_budget_strict()
{
  char const *strict = getenv("DECIPHON_HIP_PATH_STRICT");
  return strict && strict[0] == '1';
}

// DP tables of the fast path pass: chunks that are allocated as slices need them and kept until
// the engine goes (the driver wipes VRAM that is freed, and an allocation that lands on memory
// still being wiped waits for it at ~30 GB/s -- scripts/alloc_timing.py; growing without ever
// freeing never meets that).  place() hands out device addresses, reset() starts a new slice.
struct TableArena
{
  static constexpr size_t CHUNK = (size_t)2 << 30;
  struct Chunk { unsigned char *p; size_t size, used; };
  std::vector<Chunk> chunks;
  size_t held = 0;      // bytes in all chunks
  size_t placed = 0;    // bytes handed out since reset() (not bytes allocated: chunks are kept and reused)
  double alloc_ms = 0;  // time spent in hipMalloc since reset()
  size_t cur = 0;
  ~TableArena()
  {
    for (Chunk &c : chunks) (void)hipFree(c.p);
  }
  // the largest placement the chunks held so far can take (0: none held)
  size_t largest_chunk() const
  {
    size_t m = 0;
    for (Chunk const &c : chunks) m = std::max(m, c.size);
    return m;
  }
  void reset()
  {
    for (Chunk &c : chunks) c.used = 0;
    cur = 0;
    placed = 0;
    alloc_ms = 0;
  }
  // chunk after chunk (of CHUNK at the most) until the arena holds `bytes`; false: the device is full
  bool hold(size_t bytes)
  {
    reset();
    while (held < bytes)
    {
      size_t const step = std::min(CHUNK, bytes - held), before = held;
      cur = chunks.size(); // past every chunk: place() makes a new one
      if (!place(step, held + step) || held == before) return false;
    }
    reset();
    return true;
  }
  // nullptr when `bytes` more would take the arena past `budget` (or the device is full)
  unsigned char *place(size_t bytes, size_t budget)
  {
    bytes = (bytes + 255) & ~(size_t)255;
    for (; cur < chunks.size(); ++cur)
    {
      Chunk &c = chunks[cur];
      if (c.size - c.used >= bytes)
      {
        unsigned char *at = c.p + c.used;
        c.used += bytes;
        placed += bytes;
        return at;
      }
    }
    size_t want = std::max(bytes, std::min(CHUNK, budget > held ? budget - held : 0));
    if (held + want > budget)
    {
      if (placed != 0) return nullptr; // the slice ends here
      // a lone table is tried whatever the budget says -- unless the budget is a hard limit
      // (DECIPHON_HIP_PATH_STRICT=1: the caller then fails with DCP_ENOMEM, as trellis_setup does when realloc fails)
      if (path_budget_strict()) return nullptr;
      want = bytes;
    }
    auto const t0 = std::chrono::steady_clock::now();
    unsigned char *p = nullptr;
    if (hipMalloc((void **)&p, want) != hipSuccess)
    {
      (void)hipGetLastError();
      return nullptr;
    }
    double const ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    alloc_ms += ms;
    if (getenv("DECIPHON_HIP_TIMING")) fprintf(stderr, "TableArena: chunk %zu, %.2f GB in %.1f ms\n", chunks.size(), (double)want / 1e9, ms);
    chunks.push_back(Chunk{p, want, bytes});
    held += want;
    placed += bytes;
    return p;
  }
};

struct HostProfile : StageProfile // K, Kp, cls, pack, narrow: what the plan of a window list reads (dcp_hip::plan_profiles)
{
  int Q, W;
  int cQ = 0, cW = 0;  // shape of the cost kernel its cost-order copy of the rows is for (host_logic.h); 0: no copy
  int64_t pool_off; // floats
  std::string accession;
  // What dcp_hip_set_epsilon needs of a profile that came by dcp_hip_load_hmm (dcp_hip::d_dist, d_dist_models):
  int64_t dist = -1;       // entry of its node 0 among the kept distributions; -1: none kept (add_profile, add_protein, load_dcp)
  int64_t dist_models = 0; // entry of its load's null model among the kept models; the background is the next
  float epsilon = 0;       // the error rate its rows are at
  int gencode = 0;         // the translation table its rows are under (dcp_hip_set_gencode); 0: no distributions kept
  bool poisoned = false;   // DECIPHON_HIP_COST_ORDER=poison at its load: its canonical match columns are 0
};

// Where a profile's parts lie in the pool, in floats from HostProfile::pool_off (and in a host staging buffer, from its
// first float): rows[1364][DCP_ROW_HDR + Kp] | trans[8][Kp] | +inf up to 128 bytes | the cost-order copy
// [1364][dcp_cost_order_stride], for a profile that has one.  Every profile, and the copy behind its tables, starts on
// a line; the padding is +inf wherever a profile is staged, so that a pool's words depend on its profiles alone.
// (The cost kernels hold the same sum on the device side: viterbi_kernels.hip, viterbi_body.h.)
struct ProfileLayout
{
  size_t stride;    // of a row: DCP_ROW_HDR + Kp
  size_t rows = 0;
  size_t trans;
  size_t pad_begin; // behind trans ...
  size_t pad_end;   // ... up to the next multiple of 32 floats
  size_t copy;      // = pad_end
  size_t total;     // = copy without a cost-order copy
  ProfileLayout(int Kp, int cQ, int cW)
      : stride((size_t)Kp + DCP_ROW_HDR), trans((size_t)DCP_TABLE_SIZE * stride),
        pad_begin(trans + (size_t)DCP_NUM_TRANS * (size_t)Kp), pad_end((pad_begin + 31) & ~(size_t)31), copy(pad_end),
        total(copy + (cQ ? (size_t)DCP_TABLE_SIZE * (size_t)dcp_cost_order_stride(cQ, cW) : 0))
  {
  }
  explicit ProfileLayout(HostProfile const &hp) : ProfileLayout(hp.Kp, hp.cQ, hp.cW) {}
};

struct PathResult
{
  int K = 0, L = 0;
  float score = 0;
  size_t trellis_off = 0;      // bytes into d_trellis, valid when has_trellis
  bool has_trellis = false;    // the literal path kernel has run for this window
  bool trellis_on_host = false;
  // the unzipped path, one word per step: state id (c-core/state.h:9-25) | emission length << 16 -- as the device
  // wrote it, in the pinned buffer it came back in (dcp_hip::h_steps), or in `owned` when the host unzipped the trellis
  uint32_t const *steps = nullptr;
  int32_t nsteps = 0;
  std::vector<uint32_t> owned;
};

// The sequences that windows name, as the engine holds them: internal sequence i has nucleotides seq_off[i] ..
// seq_off[i + 1] and code rows row_off[i] .. row_off[i + 1], one more row than nucleotides, in d_rows.  Only
// engine_sequences.cpp writes it, and the offsets become the engine's only once their rows are written: an install that
// fails leaves none, {0}, so that every window is refused (check_window) instead of reading absent rows.
struct Sequences
{
  std::vector<int64_t> seq_off{0}, row_off{0}; // [count() + 1]
  DevBuf<unsigned char> d_nt;            // the reads as given, what the rows are made from (none for random sequences)
  DevBuf<int64_t> d_seq_off, d_row_off;  // ... and the offsets the kernel walks them by
  DevBuf<DcpCodeRow> d_rows;
  int count() const { return (int)seq_off.size() - 1; }
  int64_t code_rows() const { return row_off.back(); }
};

// a side stream for kernels that run beside others, and the event recorded behind its last launch (struct Fork)
struct Branch
{
  hipStream_t stream = nullptr;
  hipEvent_t joined = nullptr;
};

// The streams a pass runs on: the one its work is ordered on, and one side stream per kernel class, so that the kernels
// of different classes (few problems each in small scans) share the GPU instead of queueing.  The engine has two sets
// (dcp_hip::cost_set, path_set).
struct StreamSet
{
  hipStream_t stream = nullptr;
  hipEvent_t fork_ev = nullptr; // what the branches wait for (struct Fork)
  Branch cls_branch[DCP_NUM_CLASSES];
};

// The window lists of a pass and the results of its kernels, on the device; stage() fills the lists.
struct WindowLists
{
  DevBuf<DcpProblem> d_problems;
  DevBuf<DcpPack> d_packs;         // cost pass: windows of short profiles, several per wavefront
  DevBuf<PackGroup> d_pack_groups; // ... and, for four-lane groups, the packs of one profile that share a workgroup
  DevBuf<float> d_out;             // (null, alt) per window
  DevBuf<float> d_ring;            // strip class (K > 4096): the rings of folded rows, one per workgroup in flight
  // the lists go up from pinned memory: a copy from PAGEABLE memory waits for everything the device has been given
  // (the upload of a batch begun while another was in flight took as long as the rest of that batch's cost pass)
  PinBuf<DcpProblem> h_problems;
  PinBuf<DcpPack> h_packs;
  PinBuf<PackGroup> h_groups;
  hipEvent_t up_ev = nullptr; // recorded behind the uploads: the pinned lists are not rewritten before
  bool up_pending = false;
};

// The lists of a cost pass, and what dcp_hip_cost_hits_begin / _end keep of a batch between them
struct Batch : WindowLists
{
  DevBuf<uint32_t> d_hits;      // count, then (window, lrt bits) pairs
  PinBuf<uint32_t> h_hits;      // ... on the host: the whole list comes back behind the filter
  hipEvent_t done_ev = nullptr; // recorded behind the batch's last device operation
  int n = -1;                   // windows of the outstanding batch, -1: none
};

} // namespace dcp_engine

using namespace dcp_engine; // for the engine's own files only: nothing else includes this

struct dcp_hip
{
  int device = 0;
  // The cost passes' streams (the loads and dcp_hip_set_sequences* work on cost_set.stream too) and the path pass's own,
  // which may run while cost batches are in flight.  A pass is handed its set (struct Pass).
  StreamSet cost_set, path_set;
  Branch pack_branch[DCP_NUM_PACK_SHAPES]; // the packed cost kernels, one stream per shape
  Branch narrow_branch[DCP_NUM_CLASSES];   // the narrow cost kernels of classes 4..6
  std::string err;

  // profiles
  std::vector<HostProfile> profiles;
  size_t committed = 0; // profiles whose descriptors are published
  // ... and what the plan of a window list reads of them (stage_plan.h), 20 bytes each: a window list looks its profiles
  // up several times per window
  std::vector<StageProfile> plan_profiles;
  DevBuf<float> d_pool;
  size_t pool_used = 0; // floats of d_pool holding profiles
  int load_chunks = 0;  // staging chunks the last dcp_hip_load_dcp went through
  DevBuf<DcpProfileDev> d_profiles;
  // The inputs of the emission tables of the profiles loaded from HMMER3 files, kept beside the pool for
  // dcp_hip_set_epsilon: every node's entry (press_kernel.h: DCP_PRESS_IN_STRIDE floats, 528 bytes against the 5456 or
  // more of its tables), and per load that added profiles the null model's and the background's.  Counted in entries.
  DevBuf<float> d_dist, d_dist_models;
  size_t dist_used = 0, dist_models_used = 0;
  // What those entries were derived from, in host memory, for dcp_hip_set_gencode: the 20 amino log-odds of every kept
  // node, which do not depend on the translation table (80 bytes beside the 528 in HBM); [dist_used * 20].
  std::vector<float> lodds;

  Sequences seqs; // what dcp_hip_set_sequences*, _set_random_sequences installed last

  // mode
  bool mode_set = false;
  bool multi_hits = true, hmmer3_compat = false;
  DevBuf<float> d_xt;
  int xt_rows = 0;
  std::vector<float> xt_override; // [rows][DCP_XT_STRIDE], dcp_hip_set_xtrans_table

  // problems / results.  Two batches of cost passes may be outstanding at once (dcp_hip_cost_hits_begin / _end), the
  // second queued behind the first on the same kernel streams so that the GPU never drains between them; every other
  // cost call works on batch[0].  The path pass has lists of its own.
  Batch batch[2];
  WindowLists path_lists;
  int outstanding[2] = {-1, -1}; // indices into batch[] of those begun and not yet ended, oldest first
  hipStream_t upload_stream = nullptr;
  DevBuf<int64_t> d_aux;           // strip class, literal path pass: table and scratch addresses per window
  DevBuf<int64_t> d_ckpt_addr;     // fast path pass: checkpoint address per window
  DevBuf<DcpTraceState> d_trace;   // fast path pass: where each window's traceback stands between blocks
  TableArena tables;               // DP tables of the fast path pass
  std::vector<int64_t> table_addr; // per window of the slice being staged (device addresses)
  std::vector<int> path_order;     // fast path pass: request windows, slowest first
  std::vector<dcp_hip_window> path_sorted;
  DevBuf<unsigned char> d_trellis; // trellises of the literal path pass
  std::vector<dcp_hip_window> path_wins; // the windows of the last dcp_hip_path
  int path_redone = 0;                   // how many of them needed the literal pass
  DcpPathPlan path_plan;                 // fast path pass: what every window of path_sorted places (path_plan.h)
  int path_blocked = 0;                  // strip-class windows the last dcp_hip_path took in blocks (dcp_hip_path_blocked)
  int64_t path_table_bytes = 0;          // the most of tables.placed at one time since the last dcp_hip_path began
  PinBuf<int32_t> h_nsteps;        // path pass results on the host (pinned: see PinBuf)
  // the steps of a dcp_hip_path call stay where the copies from the device put them (PathResult::steps points there):
  // one pinned buffer per slice of the fast pass and one for the literal pass, reused by the next call
  std::deque<PinBuf<uint32_t>> h_steps;
  size_t h_steps_used = 0;
  PinBuf<float> h_out;
  DevBuf<uint32_t> d_steps, d_compact;
  DevBuf<int64_t> d_step_off, d_compact_off;
  DevBuf<int32_t> d_nsteps;
  std::vector<std::vector<unsigned char>> host_trellis; // fetched on demand, one per window
  std::vector<PathResult> paths;
  StagedPlan staged; // dcp_hip_stage: the list itself stays in batch[0]'s device buffers
  int staged_n = -1;
  bool staged_ran = false; // a dcp_hip_run_staged with reps > 0 has filled d_out since the dcp_hip_stage
  std::vector<CostLaunch> last_cost_launches; // the schedule launch_cost_all ran last (dcp_hip_last_cost_launches)

  // Calibration (engine_calibrate.cpp): the ladder of read lengths of the last dcp_hip_calibrate / _calibrate_lengths
  // (one rung for the first), and for profiles [0, calib_profile_lambda.size()) the Gumbel location at every rung, the
  // scores each fit left out, [profile][calib_lens.size()], and lambda -- calib_lambda, the call's argument, or the
  // profile's own fit when that was 0.  A profile beyond them has none (NaN); so has every profile once something a
  // score depends on has changed (drop_calibration).
  std::vector<int> calib_lens;
  std::vector<float> calib_mu;
  std::vector<int32_t> calib_excluded;
  std::vector<float> calib_profile_lambda;
  float calib_lambda = NAN;
  DevBuf<float> d_scores; // lrt of [profile][rung][read], gathered chunk by chunk for the one fit launch
  DevBuf<uint32_t> d_mu, d_lambda; // fp32 bits, as the fit kernel stores them
  DevBuf<int32_t> d_excluded;

  // Input generation: moves with every accepted change of the profiles, sequences, mode or xtrans override.  The
  // staged list and the path results remember the generation they were made under; dcp_hip_run_staged /
  // _fetch_staged and dcp_hip_path_trellis (which recomputes) refuse once it has moved.
  uint64_t gen = 0;
  uint64_t staged_gen = 0;
  uint64_t path_gen = UINT64_MAX; // UINT64_MAX: the last dcp_hip_path failed or there was none
};

namespace dcp_engine
{

inline int fail(dcp_hip *x, int rc, char const *what, hipError_t e = hipSuccess)
{
  char buf[256];
  if (e != hipSuccess)
    snprintf(buf, sizeof buf, "%s: %s", what, hipGetErrorString(e));
  else
    snprintf(buf, sizeof buf, "%s", what);
  x->err = buf;
  return rc;
}

#define HIP_TRY(x, call, rc)                                                   \
  do                                                                           \
  {                                                                            \
    hipError_t e_ = (call);                                                    \
    if (e_ != hipSuccess) return fail((x), (rc), #call, e_);                   \
  } while (0)

// What a pass works on: its window lists and its streams, named by the C entry point that begins it.
struct Pass
{
  dcp_hip *x;
  WindowLists &lists;
  StreamSet const &on;
  Batch *batch; // the cost passes: lists is *batch; nullptr: the path pass
};
inline Pass cost_pass(dcp_hip *x, int b = 0) { return Pass{x, x->batch[b], x->cost_set, &x->batch[b]}; }
inline Pass path_pass(dcp_hip *x) { return Pass{x, x->path_lists, x->path_set, nullptr}; }

// Kernels that run side by side: each on a branch that waits for on.fork_ev, recorded on the stream they all come
// behind; on.stream waits for every branch that was used.  Not forking, everything stays on on.stream and these do nothing.
struct Fork
{
  dcp_hip *x;
  StreamSet const &on;
  bool forking;
  std::vector<hipEvent_t> joins;
  Fork(Pass const &ps, bool forking_) : x(ps.x), on(ps.on), forking(forking_) {}
  int begin(hipStream_t origin)
  {
    if (forking) HIP_TRY(x, hipEventRecord(on.fork_ev, origin), DCP_EFUNCUSE);
    return 0;
  }
  // a's launches go to b
  int enter(Branch const &b, DcpLaunch &a)
  {
    if (!forking) return 0;
    a.stream = b.stream;
    HIP_TRY(x, hipStreamWaitEvent(a.stream, on.fork_ev, 0), DCP_EFUNCUSE);
    return 0;
  }
  // b has had its last launch
  int leave(Branch const &b)
  {
    if (!forking) return 0;
    HIP_TRY(x, hipEventRecord(b.joined, b.stream), DCP_EFUNCUSE);
    joins.push_back(b.joined);
    return 0;
  }
  // after the last launch of all (see launch_cost_all)
  int join()
  {
    for (hipEvent_t ev : joins) HIP_TRY(x, hipStreamWaitEvent(on.stream, ev, 0), DCP_EFUNCUSE);
    return 0;
  }
};

// DECIPHON_HIP_TIMING=1: phase times on stderr.  lap() = ms since the last one, the work given to `stream` included
// (it synchronises; nullptr: host time only)
struct Stopwatch
{
  bool on;
  hipStream_t stream;
  std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
  std::string line; // " <what> <ms> ms" of every named lap
  explicit Stopwatch(hipStream_t s, bool wanted = true) : on(wanted && getenv("DECIPHON_HIP_TIMING") != nullptr), stream(s) {}
  double lap()
  {
    if (!on) return 0;
    if (stream) (void)hipStreamSynchronize(stream);
    auto const now = std::chrono::steady_clock::now();
    double const ms = std::chrono::duration<double, std::milli>(now - t).count();
    t = now;
    return ms;
  }
  void lap(char const *what)
  {
    if (!on) return;
    char buf[64];
    snprintf(buf, sizeof buf, " %s %.1f ms", what, lap());
    line += buf;
  }
};

// Plans the window list (plan_stage, stage_plan.h: the checks, the lists, their order and shares) and brings the lists
// to the device, into the pass's
// (origin: the stream the lists are uploaded on -- the pass's own unless a batch is begun asynchronously)
int stage(Pass const &ps, int n, dcp_hip_window const *w, ArenaKind arena_kind, Staged &st, hipStream_t origin = nullptr);
DcpLaunch launch_args(Pass const &ps, StagedPlan const &st, int c);
int launch_cost_all(Pass const &ps, StagedPlan const &st, hipStream_t origin = nullptr);

// the scores are no longer what the profiles were calibrated on: dcp_hip_set_epsilon, _set_gencode, _set_mode,
// _set_xtrans_table, _clear_profiles
inline void drop_calibration(dcp_hip *x)
{
  x->calib_lens.clear();
  x->calib_mu.clear();
  x->calib_excluded.clear();
  x->calib_profile_lambda.clear();
  x->calib_lambda = NAN;
}

// batches begun and not ended
inline int outstanding_batches(dcp_hip const *x) { return (x->outstanding[0] >= 0) + (x->outstanding[1] >= 0); }

inline int refuse_outstanding(dcp_hip *x)
{
  return fail(x, DCP_EFUNCUSE, "cost batches are outstanding (dcp_hip_cost_hits_begin): end them first");
}

// engine_sequences.cpp, for dcp_hip_calibrate as well: what dcp_hip_set_random_sequences checks before anything is
// replaced (t: the thresholds of freq, calibrate.h), and what it does once they have passed
int check_random(dcp_hip *x, int nseq, int len, float const *freq, uint32_t t[3]);
int install_random(dcp_hip *x, int nseq, int len, uint64_t seed, uint32_t const t[3]);

// engine_profiles.cpp, for the loads of engine_hmm.cpp as well:
// class, shape, padded size and cost-order shape of a profile of K positions (pool_off is left 0)
int describe(dcp_hip *x, int K, char const *accession, HostProfile &hp);
// the part of it that needs no engine (dcp_engine_core_size, include/deciphon_host.h): false when no class holds K
bool describe_core_size(int K, StageProfile &p, int &Q, int &W);
// the pack shapes as the plan of a window list reads them, [DCP_NUM_PACK_SHAPES]: the kernels' own tables, asked once
StageShape const *pack_shapes();
// grows a device buffer to `floats`, keeping its first `keep`: once the stream is idle, a new allocation and a copy
int grow_keeping(dcp_hip *x, DevBuf<float> &buf, size_t floats, size_t keep);
// grows the device pool to `floats`, keeping what is resident (and, during a load that has written behind it, the
// first `keep` floats)
int ensure_pool(dcp_hip *x, size_t floats, size_t keep = 0);
// whether the delete costs MD, DD of trans[8][Kp] are non-negative, as the kernels need them
bool delete_costs_ok(float const *trans, int K, int Kp);

} // namespace dcp_engine
