// engine_cost.cpp -- the cost passes of the C ABI: one call, batches in flight, the benchmark's staged list.
#include "engine_internal.h"

namespace
{

// (null, alt) of the n windows of the pass's d_out, behind everything its stream has been given
int fetch_costs(Pass const &ps, size_t n, float *null_cost, float *alt_cost)
{
  std::vector<float> out(2 * n);
  HIP_TRY(ps.x, hipMemcpyAsync(out.data(), ps.lists.d_out.p, out.size() * sizeof(float), hipMemcpyDeviceToHost, ps.on.stream),
          DCP_EFUNCUSE);
  HIP_TRY(ps.x, hipStreamSynchronize(ps.on.stream), DCP_EFUNCUSE);
  for (size_t i = 0; i < n; ++i)
  {
    null_cost[i] = out[2 * i];
    alt_cost[i] = out[2 * i + 1];
  }
  return 0;
}

// device time of what the pass's stream is given between start() and stop(); the events go with the object, whichever way
// the function that holds it is left
struct EventTimer
{
  hipEvent_t e0 = nullptr, e1 = nullptr;
  EventTimer() = default;
  EventTimer(EventTimer const &) = delete;
  EventTimer &operator=(EventTimer const &) = delete;
  ~EventTimer()
  {
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
  }
  int start(Pass const &ps)
  {
    HIP_TRY(ps.x, hipEventCreate(&e0), DCP_EFUNCUSE);
    HIP_TRY(ps.x, hipEventCreate(&e1), DCP_EFUNCUSE);
    HIP_TRY(ps.x, hipEventRecord(e0, ps.on.stream), DCP_EFUNCUSE);
    return 0;
  }
  int stop(Pass const &ps, float &total) // ms
  {
    HIP_TRY(ps.x, hipEventRecord(e1, ps.on.stream), DCP_EFUNCUSE);
    HIP_TRY(ps.x, hipEventSynchronize(e1), DCP_EFUNCUSE);
    HIP_TRY(ps.x, hipEventElapsedTime(&total, e0, e1), DCP_EFUNCUSE);
    return 0;
  }
};

// DECIPHON_HIP_TIMING reports cost passes of more than 1000 windows only
bool worth_timing(int n) { return n > 1000; }

// what dcp_hip_run_staged and dcp_hip_fetch_staged need: no batch in flight, a list, and the inputs it was staged under
int check_staged(dcp_hip *x)
{
  if (outstanding_batches(x)) return refuse_outstanding(x);
  if (x->staged_n <= 0) return fail(x, DCP_EFUNCUSE, "nothing staged (dcp_hip_stage; a cost call since replaces the list)");
  if (x->staged_gen != x->gen)
    return fail(x, DCP_EFUNCUSE, "the profiles, sequences, mode or xtrans table changed since dcp_hip_stage: stage again");
  return 0;
}

} // namespace

extern "C" {

int dcp_hip_cost(struct dcp_hip *x, int n, struct dcp_hip_window const *w, float *null_cost, float *alt_cost)
{
  if (!x || (n > 0 && (!null_cost || !alt_cost))) return DCP_EFUNCUSE;
  if (outstanding_batches(x)) return refuse_outstanding(x);
  HIP_TRY(x, hipSetDevice(x->device), DCP_EFUNCUSE);
  Pass const ps = cost_pass(x);
  Stopwatch sw(ps.on.stream, worth_timing(n));
  Staged st;
  int rc = stage(ps, n, w, ARENA_NONE, st);
  if (rc) return rc;
  if (n == 0) return 0;
  HIP_TRY(x, ps.lists.d_out.reserve(2 * (size_t)n), DCP_ENOMEM);
  double const stage_ms = sw.lap();
  if ((rc = launch_cost_all(ps, st))) return rc;
  double const kernels_ms = sw.lap();
  if ((rc = fetch_costs(ps, (size_t)n, null_cost, alt_cost))) return rc;
  if (sw.on)
    fprintf(stderr, "dcp_hip_cost: %d windows; stage %.1f ms, kernels %.1f ms, fetch %.1f ms\n", n, stage_ms, kernels_ms,
            sw.lap());
  return 0;
}

int dcp_hip_cost_hits_begin(struct dcp_hip *x, int n, struct dcp_hip_window const *w)
{
  if (!x) return DCP_EFUNCUSE;
  if (x->outstanding[1] >= 0) return fail(x, DCP_EFUNCUSE, "two batches are outstanding already: call dcp_hip_cost_hits_end first");
  HIP_TRY(x, hipSetDevice(x->device), DCP_EFUNCUSE);
  int const b = x->outstanding[0] == 0 ? 1 : 0; // the one the batch in flight (if any) does not use
  Batch &B = x->batch[b];
  Pass const ps = cost_pass(x, b);
  Staged st;
  // the lists go up on a stream of their own and the kernels fork from there: a batch begun while another is in
  // flight is ordered behind it only kernel class by kernel class (the class streams), not as a whole
  Stopwatch sw(nullptr, worth_timing(n)); // host time: nothing here waits for the device
  int rc = stage(ps, n, w, ARENA_NONE, st, x->upload_stream);
  if (rc) return rc;
  double const stage_ms = sw.lap();
  if (n > 0)
  {
    HIP_TRY(x, B.d_out.reserve(2 * (size_t)n), DCP_ENOMEM);
    HIP_TRY(x, B.d_hits.reserve(1 + 2 * (size_t)n), DCP_ENOMEM);
    HIP_TRY(x, B.h_hits.reserve(1 + 2 * (size_t)n), DCP_ENOMEM);
    HIP_TRY(x, hipMemsetAsync(B.d_hits.p, 0, sizeof(uint32_t), x->upload_stream), DCP_EFUNCUSE);
    if ((rc = launch_cost_all(ps, st, x->upload_stream))) return rc;
    HIP_TRY(x, dcp_launch_lrt_filter(B.d_out.p, n, B.d_hits.p, ps.on.stream), DCP_EFUNCUSE);
    // count and list together (8 B per window at most: nothing beside the kernels), into pinned memory
    HIP_TRY(x, hipMemcpyAsync(B.h_hits.p, B.d_hits.p, (1 + 2 * (size_t)n) * sizeof(uint32_t), hipMemcpyDeviceToHost, ps.on.stream),
            DCP_EFUNCUSE);
    HIP_TRY(x, hipEventRecord(B.done_ev, ps.on.stream), DCP_EFUNCUSE);
  }
  B.n = n;
  x->outstanding[x->outstanding[0] >= 0 ? 1 : 0] = b;
  if (sw.on) fprintf(stderr, "dcp_hip_cost_hits_begin: %d windows; stage %.1f ms, enqueue %.1f ms\n", n, stage_ms, sw.lap());
  return 0;
}

int dcp_hip_cost_hits_end(struct dcp_hip *x, int *nhits, int32_t *hit_window, float *hit_lrt)
{
  if (!x || !nhits) return DCP_EFUNCUSE;
  int const b = x->outstanding[0];
  if (b < 0) return fail(x, DCP_EFUNCUSE, "dcp_hip_cost_hits_end without dcp_hip_cost_hits_begin");
  Batch &B = x->batch[b];
  int const n = B.n;
  *nhits = 0;
  HIP_TRY(x, hipSetDevice(x->device), DCP_EFUNCUSE);
  // whatever happens below, the batch is over once its device work is
  Stopwatch sw(nullptr, worth_timing(n));
  hipError_t const waited = n > 0 ? hipEventSynchronize(B.done_ev) : hipSuccess;
  double const waited_ms = sw.lap();
  B.n = -1;
  x->outstanding[0] = x->outstanding[1];
  x->outstanding[1] = -1;
  if (waited != hipSuccess) return fail(x, DCP_EFUNCUSE, "hipEventSynchronize", waited);
  if (n == 0) return 0;
  if (!hit_window || !hit_lrt) return DCP_EFUNCUSE;
  uint32_t const count = B.h_hits.p[0];
  if (sw.on) fprintf(stderr, "dcp_hip_cost_hits_end: %d windows, %u hits; waited %.1f ms\n", n, count, waited_ms);
  if (count == 0) return 0;
  uint32_t const *pairs = B.h_hits.p + 1;
  std::vector<std::pair<uint32_t, uint32_t>> hits(count);
  for (uint32_t i = 0; i < count; ++i) hits[i] = {pairs[2 * (size_t)i], pairs[2 * (size_t)i + 1]};
  std::sort(hits.begin(), hits.end()); // the device appends in no particular order
  for (uint32_t i = 0; i < count; ++i)
  {
    hit_window[i] = (int32_t)hits[i].first;
    memcpy(hit_lrt + i, &hits[i].second, sizeof(float));
  }
  *nhits = (int)count;
  return 0;
}

int dcp_hip_cost_hits(struct dcp_hip *x, int n, struct dcp_hip_window const *w, int *nhits, int32_t *hit_window,
                      float *hit_lrt)
{
  if (!x || !nhits || (n > 0 && (!hit_window || !hit_lrt))) return DCP_EFUNCUSE;
  *nhits = 0;
  if (outstanding_batches(x)) return fail(x, DCP_EFUNCUSE, "batches are outstanding: dcp_hip_cost_hits_end first");
  int rc = dcp_hip_cost_hits_begin(x, n, w);
  if (rc) return rc;
  return dcp_hip_cost_hits_end(x, nhits, hit_window, hit_lrt);
}

int dcp_hip_cost_bench(struct dcp_hip *x, int n, struct dcp_hip_window const *w, int warmup, int reps, float *ms,
                       double *cells, float *null_cost, float *alt_cost)
{
  if (!x || n <= 0 || reps <= 0 || !ms || !cells) return DCP_EFUNCUSE;
  if (outstanding_batches(x)) return refuse_outstanding(x);
  HIP_TRY(x, hipSetDevice(x->device), DCP_EFUNCUSE);
  Pass const ps = cost_pass(x);
  Staged st;
  int rc = stage(ps, n, w, ARENA_NONE, st);
  if (rc) return rc;
  HIP_TRY(x, ps.lists.d_out.reserve(2 * (size_t)n), DCP_ENOMEM);
  for (int i = 0; i < warmup; ++i)
    if ((rc = launch_cost_all(ps, st))) return rc;
  EventTimer timer;
  if ((rc = timer.start(ps))) return rc;
  for (int i = 0; i < reps; ++i)
    if ((rc = launch_cost_all(ps, st))) return rc;
  float total = 0;
  if ((rc = timer.stop(ps, total))) return rc;
  *ms = total / (float)reps;
  *cells = st.cells;
  return null_cost && alt_cost ? fetch_costs(ps, (size_t)n, null_cost, alt_cost) : 0;
}

int dcp_hip_stage(struct dcp_hip *x, int n, struct dcp_hip_window const *w)
{
  if (!x) return DCP_EFUNCUSE;
  if (outstanding_batches(x)) return refuse_outstanding(x);
  x->staged_n = -1; // a failed stage leaves no list behind
  if (n <= 0) return fail(x, DCP_EFUNCUSE, "dcp_hip_stage needs at least one window");
  HIP_TRY(x, hipSetDevice(x->device), DCP_EFUNCUSE);
  Pass const ps = cost_pass(x);
  Staged st;
  int rc = stage(ps, n, w, ARENA_NONE, st);
  if (rc) return rc;
  HIP_TRY(x, ps.lists.d_out.reserve(2 * (size_t)n), DCP_ENOMEM);
  HIP_TRY(x, hipStreamSynchronize(ps.on.stream), DCP_EFUNCUSE);
  x->staged = st;
  x->staged_n = n;
  x->staged_ran = false;
  x->staged_gen = x->gen;
  return 0;
}

int dcp_hip_run_staged(struct dcp_hip *x, int reps, float *ms, double *cells)
{
  if (!x || reps < 0) return DCP_EFUNCUSE;
  int rc = check_staged(x);
  if (rc) return rc;
  HIP_TRY(x, hipSetDevice(x->device), DCP_EFUNCUSE);
  Pass const ps = cost_pass(x);
  StagedPlan const &st = x->staged;
  EventTimer timer;
  if ((rc = timer.start(ps))) return rc;
  for (int i = 0; i < reps && !rc; ++i) rc = launch_cost_all(ps, st); // every pass joined before the next starts
  if (rc) return rc;
  float total = 0;
  if ((rc = timer.stop(ps, total))) return rc;
  if (ms) *ms = total;
  if (cells) *cells = st.cells;
  if (reps > 0) x->staged_ran = true;
  return 0;
}

int dcp_hip_fetch_staged(struct dcp_hip *x, float *null_cost, float *alt_cost)
{
  if (!x || !null_cost || !alt_cost) return DCP_EFUNCUSE;
  int rc = check_staged(x);
  if (rc) return rc;
  if (!x->staged_ran) return fail(x, DCP_EFUNCUSE, "dcp_hip_run_staged has not run the staged list yet");
  return fetch_costs(cost_pass(x), (size_t)x->staged_n, null_cost, alt_cost);
}

int dcp_hip_last_cost_launches(struct dcp_hip const *x, int cap, int32_t *out)
{
  if (!x || cap < 0 || (cap > 0 && !out)) return -1;
  std::vector<CostLaunch> const &s = x->last_cost_launches;
  for (size_t i = 0; i < s.size() && i < (size_t)cap; ++i)
  {
    int32_t const row[5] = {s[i].kernel, s[i].index, s[i].first, s[i].count, s[i].windows_per_profile};
    memcpy(out + 5 * i, row, sizeof row);
  }
  return (int)s.size();
}

} // extern "C"
