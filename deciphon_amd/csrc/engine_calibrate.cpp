// engine_calibrate.cpp -- the calibration of the resident profiles on random reads (install_random,
// engine_sequences.cpp): a cost pass over profiles x random reads through the engine's own stage, plan and launch path,
// at every rung of a ladder of read lengths, and one Gumbel fit of every profile's scores (calibrate.hip).  The reads
// themselves: calibrate.h; mu at a window length between or beyond the rungs: dcp_calib_mu_at (host_logic.cpp).
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

// The ladder (lens[nlen], checked by the caller: 1 .. DCP_CALIB_MAX_LENS lengths >= 1, increasing) at lambda > 0, or at
// the lambda fitted per profile for lambda == 0.  `name`: the entry point, for the timing line.
int calibrate_ladder(dcp_hip *x, char const *name, int nseq, int nlen, int const *lens, uint64_t seed, float const *freq, float lambda)
{
  uint32_t t[3];
  for (int j = 0; j < nlen; ++j) // every rung's checks before the first rung is installed
    if (int rc = check_random(x, nseq, lens[j], freq, t)) return rc;
  if (x->committed != x->profiles.size()) return fail(x, DCP_EFUNCUSE, "profiles not committed");
  int const nprof = (int)x->profiles.size();
  if (nprof > 0 && !x->mode_set) return fail(x, DCP_EFUNCUSE, "dcp_hip_set_mode has not been called");
  for (StageProfile const &p : x->plan_profiles)
    if (p.cls < 0 || p.cls >= DCP_NUM_CLASSES) return fail(x, DCP_ELARGECORESIZE, "profile outside every kernel class");
  // the scores of every profile at every rung (d_out is every chunk's), and the fit's results: before anything changes
  size_t const rungs = (size_t)nprof * (size_t)nlen;
  if (nprof > 0)
  {
    HIP_TRY(x, hipSetDevice(x->device), DCP_EFUNCUSE);
    HIP_TRY(x, x->d_scores.reserve(rungs * (size_t)nseq), DCP_ENOMEM);
    HIP_TRY(x, x->d_mu.reserve(rungs), DCP_ENOMEM);
    HIP_TRY(x, x->d_excluded.reserve(rungs), DCP_ENOMEM);
    HIP_TRY(x, x->d_lambda.reserve((size_t)nprof), DCP_ENOMEM);
  }
  Pass const ps = cost_pass(x);
  Stopwatch sw(ps.on.stream);
  double gen_ms = 0, cost_ms = 0, gather_ms = 0, fit_ms = 0, cells = 0;
  // chunks of whole profiles; profile-major windows {p, s, 0, len}: window i of a chunk is slot i of its d_out
  // (calib_windows() <= INT_MAX, so a chunk holds at most INT_MAX windows)
  int const per_chunk = (int)std::max<int64_t>(calib_windows() / nseq, 1);
  std::vector<dcp_hip_window> wins;
  int chunks = 0;
  for (int j = 0; j < nlen; ++j)
  {
    int const len = lens[j];
    if (int rc = install_random(x, nseq, len, seed + (uint64_t)j, t)) return rc;
    gen_ms += sw.lap();
    for (int p0 = 0; p0 < nprof; p0 += per_chunk, ++chunks)
    {
      int const np = std::min(per_chunk, nprof - p0);
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
      HIP_TRY(x, dcp_launch_calib_gather(ps.lists.d_out.p, np, nseq, nlen, j, x->d_scores.p + (size_t)p0 * (size_t)nlen * (size_t)nseq,
                                         ps.on.stream),
              DCP_EFUNCUSE);
      gather_ms += sw.lap();
    }
  }
  if (nprof == 0) return 0;
  HIP_TRY(x, dcp_launch_gumbel_ladder_fit(x->d_scores.p, nprof, nlen, nseq, lambda, x->d_mu.p, x->d_excluded.p, x->d_lambda.p, ps.on.stream),
          DCP_EFUNCUSE);
  // the results of all profiles at once, and only then into the engine: a failure above leaves what was
  std::vector<float> mu(rungs), lam((size_t)nprof);
  std::vector<int32_t> excluded(rungs);
  HIP_TRY(x, hipMemcpyAsync(mu.data(), x->d_mu.p, rungs * sizeof(uint32_t), hipMemcpyDeviceToHost, ps.on.stream), DCP_EFUNCUSE);
  HIP_TRY(x, hipMemcpyAsync(excluded.data(), x->d_excluded.p, rungs * sizeof(int32_t), hipMemcpyDeviceToHost, ps.on.stream), DCP_EFUNCUSE);
  HIP_TRY(x, hipMemcpyAsync(lam.data(), x->d_lambda.p, lam.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, ps.on.stream), DCP_EFUNCUSE);
  HIP_TRY(x, hipStreamSynchronize(ps.on.stream), DCP_EFUNCUSE);
  x->calib_lens.assign(lens, lens + nlen);
  x->calib_mu = std::move(mu);
  x->calib_excluded = std::move(excluded);
  x->calib_profile_lambda = std::move(lam);
  x->calib_lambda = lambda;
  fit_ms += sw.lap();
  if (sw.on)
    fprintf(stderr,
            "%s: %d profiles, %d rungs, %lld windows in %d chunks, %.4g cells; generation %.6f s, cost pass %.6f s, gather %.6f s, "
            "fit %.6f s\n",
            name, nprof, nlen, (long long)nprof * nseq * nlen, chunks, cells, gen_ms / 1e3, cost_ms / 1e3, gather_ms / 1e3, fit_ms / 1e3);
  return 0;
}

// profile i at rung j of the calibration in force
bool calibrated_at(dcp_hip const *x, int i, int j)
{
  return x && i >= 0 && (size_t)i < x->calib_profile_lambda.size() && (size_t)i < x->profiles.size() && j >= 0 &&
         (size_t)j < x->calib_lens.size();
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
  return calibrate_ladder(x, "dcp_hip_calibrate", nseq, 1, &len, seed, freq, lambda);
}

int dcp_hip_calibrate_lengths(struct dcp_hip *x, int nseq, int nlen, int const *lens, uint64_t seed, float const freq[4], float lambda)
{
  if (!x) return DCP_EFUNCUSE;
  if (outstanding_batches(x)) return refuse_outstanding(x);
  if (nlen < 1 || nlen > DCP_CALIB_MAX_LENS || !lens) return fail(x, DCP_EFUNCUSE, "a ladder has 1 to DCP_CALIB_MAX_LENS lengths");
  for (int j = 0; j < nlen; ++j)
    if (lens[j] < 1 || (j > 0 && lens[j] <= lens[j - 1])) return fail(x, DCP_EFUNCUSE, "the lengths of a ladder are at least 1 and increase");
  if (nseq < 1) return fail(x, DCP_EFUNCUSE, "a calibration needs at least one sequence");
  if (!(lambda >= 0.0f) || !(lambda <= 3.4e38f)) return fail(x, DCP_EFUNCUSE, "lambda must be positive and finite, or 0: fitted");
  if (lambda == 0.0f && nseq < 2) return fail(x, DCP_EFUNCUSE, "fitting lambda needs at least two sequences");
  return calibrate_ladder(x, "dcp_hip_calibrate_lengths", nseq, nlen, lens, seed, freq, lambda);
}

int dcp_hip_calib_num_lengths(struct dcp_hip const *x) { return x ? (int)x->calib_lens.size() : 0; }

int dcp_hip_calib_length(struct dcp_hip const *x, int j)
{
  return x && j >= 0 && (size_t)j < x->calib_lens.size() ? x->calib_lens[(size_t)j] : 0;
}

float dcp_hip_profile_mu_rung(struct dcp_hip const *x, int i, int j)
{
  return calibrated_at(x, i, j) ? x->calib_mu[(size_t)i * x->calib_lens.size() + (size_t)j] : NAN;
}

int dcp_hip_profile_calib_excluded_rung(struct dcp_hip const *x, int i, int j)
{
  return calibrated_at(x, i, j) ? x->calib_excluded[(size_t)i * x->calib_lens.size() + (size_t)j] : 0;
}

float dcp_hip_profile_lambda(struct dcp_hip const *x, int i) { return calibrated_at(x, i, 0) ? x->calib_profile_lambda[(size_t)i] : NAN; }

double dcp_hip_profile_mu_at(struct dcp_hip const *x, int i, int64_t len)
{
  if (!calibrated_at(x, i, 0)) return NAN;
  int const nlen = (int)x->calib_lens.size();
  return dcp_calib_mu_at(nlen, x->calib_lens.data(), x->calib_mu.data() + (size_t)i * (size_t)nlen, len);
}

float dcp_hip_profile_mu(struct dcp_hip const *x, int i) { return dcp_hip_profile_mu_rung(x, i, 0); }

int dcp_hip_profile_calib_excluded(struct dcp_hip const *x, int i) { return dcp_hip_profile_calib_excluded_rung(x, i, 0); }

float dcp_hip_calib_lambda(struct dcp_hip const *x) { return x ? x->calib_lambda : NAN; }

} // extern "C"
