// engine_calibrate.cpp -- the calibration of the resident profiles on random reads (install_random,
// engine_sequences.cpp): a cost pass over profiles x random reads through the engine's own stage, plan and launch path,
// and a Gumbel fit of every profile's scores (calibrate.hip).  The reads themselves: calibrate.h.
#include "../../include/deciphon_host.h"
#include "engine_internal.h"
#include <limits.h>

namespace
{

// DECIPHON_HIP_CALIB_WINDOWS: the most windows of a calibration's cost pass (a chunk is whole profiles, one at the
// least).  Unset: what a chunk of dcp_scan_run holds, DCP_SCAN_CHUNK_WINDOWS -- the list, its pinned copy and the
// results of that many windows are what a scan keeps per batch anyway.
int64_t calib_windows()
{
  char const *e = getenv("DECIPHON_HIP_CALIB_WINDOWS");
  int64_t const v = e ? atoll(e) : (int64_t)DCP_SCAN_CHUNK_WINDOWS;
  return std::min<int64_t>(std::max<int64_t>(v, 1), INT_MAX);
}

} // namespace

extern "C" {

int dcp_hip_calibrate(struct dcp_hip *x, int nseq, int len, uint64_t seed, float const freq[4], float lambda)
{
  if (!x) return DCP_EFUNCUSE;
  uint32_t t[3];
  if (int rc = check_random(x, nseq, len, freq, t)) return rc;
  if (nseq < 1 || len < 1) return fail(x, DCP_EFUNCUSE, "a calibration needs at least one sequence of at least one nucleotide");
  if (!(lambda > 0.0f) || !(lambda <= 3.4e38f)) return fail(x, DCP_EFUNCUSE, "lambda must be positive and finite");
  if (x->committed != x->profiles.size()) return fail(x, DCP_EFUNCUSE, "profiles not committed");
  int const nprof = (int)x->profiles.size();
  if (nprof > 0 && !x->mode_set) return fail(x, DCP_EFUNCUSE, "dcp_hip_set_mode has not been called");
  for (StageProfile const &p : x->plan_profiles)
    if (p.cls < 0 || p.cls >= DCP_NUM_CLASSES) return fail(x, DCP_ELARGECORESIZE, "profile outside every kernel class");
  Pass const ps = cost_pass(x);
  Stopwatch sw(ps.on.stream);
  if (int rc = install_random(x, nseq, len, seed, t)) return rc;
  if (nprof == 0) return 0;
  double const gen_ms = sw.lap();
  double cost_ms = 0, fit_ms = 0, cells = 0;

  // chunks of whole profiles; profile-major windows {p, s, 0, len}: window i of a chunk is slot i of its d_out
  int const per_chunk = (int)std::max<int64_t>(calib_windows() / nseq, 1);
  HIP_TRY(x, x->d_mu.reserve((size_t)nprof), DCP_ENOMEM);
  HIP_TRY(x, x->d_excluded.reserve((size_t)nprof), DCP_ENOMEM);
  std::vector<dcp_hip_window> wins;
  int chunks = 0;
  for (int p0 = 0; p0 < nprof; p0 += per_chunk, ++chunks)
  {
    int const np = std::min(per_chunk, nprof - p0);
    if ((int64_t)np * nseq > (int64_t)INT_MAX) return fail(x, DCP_EFUNCUSE, "more than INT_MAX windows per profile");
    int const n = np * nseq;
    wins.resize((size_t)n);
    for (int p = 0; p < np; ++p)
      for (int s = 0; s < nseq; ++s) wins[(size_t)p * (size_t)nseq + (size_t)s] = dcp_hip_window{p0 + p, s, 0, len};
    Staged st;
    if (int rc = stage(ps, n, wins.data(), ARENA_NONE, st)) return rc;
    HIP_TRY(x, ps.lists.d_out.reserve(2 * (size_t)n), DCP_ENOMEM);
    if (int rc = launch_cost_all(ps, st)) return rc;
    cells += st.cells;
    cost_ms += sw.lap();
    HIP_TRY(x, dcp_launch_gumbel_fit(ps.lists.d_out.p, np, nseq, lambda, x->d_mu.p + p0, x->d_excluded.p + p0, ps.on.stream),
            DCP_EFUNCUSE);
    fit_ms += sw.lap();
  }
  // mu and the excluded counts of all profiles at once, and only then into the engine: a failure above leaves what was
  std::vector<uint32_t> bits((size_t)nprof);
  std::vector<int32_t> excluded((size_t)nprof);
  HIP_TRY(x, hipMemcpyAsync(bits.data(), x->d_mu.p, bits.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, ps.on.stream), DCP_EFUNCUSE);
  HIP_TRY(x, hipMemcpyAsync(excluded.data(), x->d_excluded.p, excluded.size() * sizeof(int32_t), hipMemcpyDeviceToHost, ps.on.stream),
          DCP_EFUNCUSE);
  HIP_TRY(x, hipStreamSynchronize(ps.on.stream), DCP_EFUNCUSE);
  x->calib_mu.resize((size_t)nprof);
  memcpy(x->calib_mu.data(), bits.data(), bits.size() * sizeof(uint32_t));
  x->calib_excluded = std::move(excluded);
  x->calib_lambda = lambda;
  fit_ms += sw.lap();
  if (sw.on)
    fprintf(stderr,
            "dcp_hip_calibrate: %d profiles, %lld windows in %d chunks, %.4g cells; generation %.6f s, cost pass %.6f s, fit %.6f s\n",
            nprof, (long long)nprof * nseq, chunks, cells, gen_ms / 1e3, cost_ms / 1e3, fit_ms / 1e3);
  return 0;
}

float dcp_hip_profile_mu(struct dcp_hip const *x, int i)
{
  if (!x || i < 0 || (size_t)i >= x->calib_mu.size() || (size_t)i >= x->profiles.size()) return NAN;
  return x->calib_mu[(size_t)i];
}

int dcp_hip_profile_calib_excluded(struct dcp_hip const *x, int i)
{
  if (!x || i < 0 || (size_t)i >= x->calib_excluded.size() || (size_t)i >= x->profiles.size()) return 0;
  return x->calib_excluded[(size_t)i];
}

float dcp_hip_calib_lambda(struct dcp_hip const *x) { return x ? x->calib_lambda : NAN; }

} // extern "C"
