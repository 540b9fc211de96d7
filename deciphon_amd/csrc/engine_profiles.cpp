// engine_profiles.cpp -- the engine's profiles: add, load, commit, clear, and the cost-order staging.
#include "engine_internal.h"
#include "engine_hmm.h"
#include "parallel_for.h"
#include "../../include/deciphon_host.h"
#include "press_batch.h"
#include "press_reemit.h"
#include "press_rows.h"

#include <limits.h>

extern "C" {

// ---- profiles: HBM is the only resident copy ---------------------------------------
// A profile is laid out on the host in a staging buffer (rows | trans, +inf padded) and
// copied behind the profiles already resident; nothing Pfam-sized is ever held twice.

// rows | trans, rounded up to 128 bytes: every profile, and the cost-order copy behind its tables, starts on a line
static size_t canonical_floats(int Kp)
{
  size_t const floats = (size_t)DCP_TABLE_SIZE * ((size_t)Kp + DCP_ROW_HDR) + (size_t)DCP_NUM_TRANS * (size_t)Kp;
  return (floats + 31) & ~(size_t)31;
}

// the floats of that rounding, behind trans: +inf wherever a profile is staged, so that a pool's words depend on its
// profiles alone
static size_t canonical_tables(int Kp)
{
  return (size_t)DCP_TABLE_SIZE * ((size_t)Kp + DCP_ROW_HDR) + (size_t)DCP_NUM_TRANS * (size_t)Kp;
}

static size_t profile_floats(HostProfile const &hp)
{
  size_t const copy = hp.cQ ? (size_t)DCP_TABLE_SIZE * (size_t)dcp_cost_order_stride(hp.cQ, hp.cW) : 0;
  return canonical_floats(hp.Kp) + copy;
}

// The cost-order copy (host_logic.h) of the staged rows, behind the profile's canonical tables, for the profiles whose
// default cost kernel is a narrow one (dcp_launch_cost_narrow) that gains from it: (5,1) and (10,1), K = 257..320 and
// 513..640.  Their tail chunks of one and two floats were the most strided loads; per class they run 7-10 % and 6-8 %
// faster on the copy, while (6,1), (7,1), (8,1) and (6,2) do not move (profiles/r04_cost_order_ab.txt) -- no copy there.
// Only dcp_cost_kernel<5,1> and <10,1> read it: every other kernel has a shape of its own (the checkpoint and block
// kernels of the path pass run the class shape) and reads the canonical rows.
// DECIPHON_HIP_COST_ORDER, read at ingest: 0 = no copies; "poison" = copies, and the canonical match columns of those
// profiles staged as 0 (a test's proof that the narrow kernels read the copy: their scores stay the oracle's).
static bool cost_order_pays(int Q, int W) { return W == 1 && (Q == 5 || Q == 10); }

static void cost_order_shape(HostProfile &hp)
{
  hp.cQ = hp.cW = 0;
  char const *e = getenv("DECIPHON_HIP_COST_ORDER");
  if (!hp.narrow || (e && e[0] == '0')) return;
  int const q = dcp_class_narrow_q(hp.cls);
  if (!cost_order_pays(q, 1)) return;
  hp.cQ = q;
  hp.cW = 1;
}

static void stage_cost_order(HostProfile const &hp, float *staged)
{
  if (!hp.cQ) return;
  dcp_cost_order_rows(hp.cQ, hp.cW, hp.K, hp.Kp, staged, staged + canonical_floats(hp.Kp));
  char const *e = getenv("DECIPHON_HIP_COST_ORDER");
  if (e && strcmp(e, "poison") == 0)
    for (int c = 0; c < DCP_TABLE_SIZE; ++c)
      memset(staged + (size_t)c * ((size_t)hp.Kp + DCP_ROW_HDR) + DCP_ROW_HDR, 0, sizeof(float) * (size_t)hp.K);
}

static int describe(dcp_hip *x, int K, char const *accession, HostProfile &hp)
{
  if (K < 1 || K > DCP_MODEL_MAX) return fail(x, DCP_ELARGECORESIZE, "core size out of range");
  int const cls = dcp_class_of(K);
  if (cls < 0) return fail(x, DCP_ELARGECORESIZE, "core size beyond DCP_MAX_CORE_SIZE (16383: state ids keep 14 bits for k + 1)");
  hp.K = K;
  hp.cls = cls;
  dcp_class_shape(cls, &hp.Q, &hp.W);
  hp.Kp = 64 * hp.Q * hp.W;
  if (cls == DCP_STRIP_CLASS) hp.Kp *= (K + hp.Kp - 1) / hp.Kp; // whole strips
  hp.pool_off = 0;
  hp.accession = accession ? accession : "";
  hp.narrow = K <= dcp_class_narrow_limit(cls);
  cost_order_shape(hp);
  hp.pack = dcp_pack_shape_of(K);
  if (hp.pack >= 0)
  {
    int pq = 0, ps = 0;
    dcp_pack_shape(hp.pack, &pq, &ps);
    if (hp.W != 1 || ps * pq > hp.Kp) hp.pack = -1; // the shape reads S * Q columns of a row
  }
  return 0;
}

// grows a device buffer to `floats`, keeping its first `keep`: once the stream is idle, a new allocation and a copy
static int grow_keeping(dcp_hip *x, DevBuf<float> &buf, size_t floats, size_t keep)
{
  if (floats <= buf.cap) return 0;
  HIP_TRY(x, hipStreamSynchronize(x->stream), DCP_EFUNCUSE);
  DevBuf<float> bigger;
  HIP_TRY(x, bigger.reserve(std::max(floats, buf.cap + buf.cap / 2)), DCP_ENOMEM);
  if (keep) HIP_TRY(x, hipMemcpy(bigger.p, buf.p, keep * sizeof(float), hipMemcpyDeviceToDevice), DCP_EFUNCUSE);
  buf.release();
  buf.p = bigger.p;
  buf.cap = bigger.cap;
  bigger.p = nullptr;
  bigger.cap = 0;
  return 0;
}

// grows the device pool to `floats`, keeping what is resident (and, during a load that has written behind it, the
// first `keep` floats)
static int ensure_pool(dcp_hip *x, size_t floats, size_t keep = 0)
{
  return grow_keeping(x, x->d_pool, floats, std::max(keep, x->pool_used));
}

// one profile from a host staging buffer to the end of the pool
static int push_profile(dcp_hip *x, HostProfile hp, std::vector<float> const &staged, int *index)
{
  int rc = ensure_pool(x, x->pool_used + staged.size());
  if (rc) return rc;
  hp.pool_off = (int64_t)x->pool_used;
  HIP_TRY(x, hipMemcpy(x->d_pool.p + x->pool_used, staged.data(), staged.size() * sizeof(float), hipMemcpyHostToDevice),
          DCP_EFUNCUSE);
  x->pool_used += staged.size();
  if (index) *index = (int)x->profiles.size();
  x->profiles.push_back(hp);
  ++x->gen;
  return 0;
}

// The kernels take E_l = min_k M_l[k] (viterbi_body.h) and bound what a delete run can carry across a
// wavefront (CostWave::row): both need the delete costs MD, DD to be non-negative, which -log-probabilities
// are.  Anything else (a positive log-probability in a corrupt file, a hand-made table) is refused.
static bool delete_costs_ok(float const *trans, int K, int Kp)
{
  for (int k = 0; k < K; ++k)
    if (!(trans[(size_t)DCP_MD * Kp + k] >= 0.0f) || !(trans[(size_t)DCP_DD * Kp + k] >= 0.0f)) return false;
  return true;
}

int dcp_hip_add_profile(struct dcp_hip *x, int K, float const *trans, float const *match, float const *null_cost,
                        float const *bg_cost, int *index)
{
  if (!x || !trans || !match || !null_cost || !bg_cost) return DCP_EFUNCUSE;
  if (outstanding_batches(x)) return refuse_outstanding(x);
  HIP_TRY(x, hipSetDevice(x->device), DCP_EFUNCUSE);
  HostProfile hp;
  int rc = describe(x, K, nullptr, hp);
  if (rc) return rc;
  int const Kp = hp.Kp;
  size_t const stride = (size_t)Kp + DCP_ROW_HDR;
  std::vector<float> buf(profile_floats(hp), INFINITY);
  float *r = buf.data();
  float *t = r + (size_t)DCP_TABLE_SIZE * stride;
  for (int id = 0; id < DCP_NUM_TRANS; ++id) memcpy(t + (size_t)id * Kp, trans + (size_t)id * K, sizeof(float) * K);
  if (!delete_costs_ok(t, K, Kp)) return fail(x, DCP_EFUNCUSE, "negative (or NaN) delete cost: costs are -log-probabilities");
  for (int c = 0; c < DCP_TABLE_SIZE; ++c)
  {
    float *hdr = r + (size_t)c * stride;
    hdr[0] = null_cost[c];
    hdr[1] = bg_cost[c];
    hdr[2] = hdr[3] = 0.0f;
    memcpy(hdr + DCP_ROW_HDR, match + (size_t)c * K, sizeof(float) * K);
  }
  stage_cost_order(hp, r);
  return push_profile(x, hp, buf, index);
}

int dcp_hip_add_protein(struct dcp_hip *x, int K, float const *node_trans, float const *node_emission,
                        float const *BMk, float const *null_lprob, float const *bg_lprob, int *index)
{
  if (!x || !node_trans || !node_emission || !BMk || !null_lprob || !bg_lprob) return DCP_EFUNCUSE;
  if (outstanding_batches(x)) return refuse_outstanding(x);
  HIP_TRY(x, hipSetDevice(x->device), DCP_EFUNCUSE);
  HostProfile hp;
  int rc = describe(x, K, nullptr, hp);
  if (rc) return rc;
  std::vector<float> buf(profile_floats(hp), INFINITY);
  float *r = buf.data();
  float *t = r + (size_t)DCP_TABLE_SIZE * ((size_t)hp.Kp + DCP_ROW_HDR);
  dcp_setup_profile(K, hp.Kp, node_trans, node_emission, BMk, null_lprob, bg_lprob, t, r);
  if (!delete_costs_ok(t, K, hp.Kp)) return fail(x, DCP_EFDATA, "positive (or NaN) delete log-probability in the protein");
  stage_cost_order(hp, r);
  return push_profile(x, hp, buf, index);
}

// Streams proteins [first, first+count) of a pressed database into HBM: core sizes are read
// first (so the pool is sized once), then the proteins are unpacked and transposed into
// code-major rows by up to 16 host threads, chunk by chunk, into two pinned staging buffers whose
// H2D copies overlap the unpacking of the next chunk.
int dcp_hip_load_dcp(struct dcp_hip *x, char const *path, int first, int count)
{
  if (!x || !path) return DCP_EFUNCUSE;
  if (outstanding_batches(x)) return refuse_outstanding(x);
  HIP_TRY(x, hipSetDevice(x->device), DCP_EFUNCUSE);
  DcpDbReader db;
  int rc = db.open(path);
  if (rc) return fail(x, rc, "cannot open database");
  int const N = db.num_proteins();
  if (first < 0 || first > N) return fail(x, DCP_EINVALPART, "first protein out of range");
  int const last = count < 0 ? N : std::min(N, first + count);
  int const n = last - first;
  if (n <= 0)
  {
    ++x->gen; // nothing to read, but a successful load ends what was computed before it, as every other does
    return 0;
  }

  std::vector<HostProfile> hps((size_t)n);
  std::vector<size_t> off((size_t)n + 1, 0);
  for (int i = 0; i < n; ++i)
  {
    int K = 0;
    std::string acc;
    if ((rc = db.read_protein_head(first + i, K, acc))) return fail(x, rc, "cannot read protein");
    if ((rc = describe(x, K, acc.c_str(), hps[(size_t)i]))) return rc;
    off[(size_t)i + 1] = off[(size_t)i] + profile_floats(hps[(size_t)i]);
  }
  if ((rc = ensure_pool(x, x->pool_used + off[(size_t)n]))) return rc;

  // staging chunks of 256 MiB; DECIPHON_HIP_STAGE_MB shrinks them (never below one profile of the largest
  // size present), which is how the tests drive a small database through many chunks
  size_t chunk_floats = std::max<size_t>((size_t)64 << 20, canonical_floats(DCP_MAX_CORE_SIZE));
  if (char const *e = getenv("DECIPHON_HIP_STAGE_MB"))
  {
    size_t largest = 0;
    for (int i = 0; i < n; ++i) largest = std::max(largest, off[(size_t)i + 1] - off[(size_t)i]);
    chunk_floats = std::max<size_t>(((size_t)std::max(atol(e), 1L) << 20) / sizeof(float), largest);
  }
  int chunks = 0;
  float *stage[2] = {nullptr, nullptr};
  hipEvent_t done[2] = {nullptr, nullptr};
  bool busy[2] = {false, false};
  auto cleanup = [&]() {
    (void)hipStreamSynchronize(x->stream);
    for (int b = 0; b < 2; ++b)
    {
      if (stage[b]) (void)hipHostFree(stage[b]);
      if (done[b]) (void)hipEventDestroy(done[b]);
    }
  };
  for (int b = 0; b < 2; ++b)
  {
    if (hipHostMalloc((void **)&stage[b], std::min(chunk_floats, off[(size_t)n]) * sizeof(float), hipHostMallocDefault) !=
            hipSuccess ||
        hipEventCreateWithFlags(&done[b], hipEventDisableTiming) != hipSuccess)
    {
      cleanup();
      return fail(x, DCP_ENOMEM, "cannot allocate pinned staging buffers");
    }
  }
  int b = 0;
  for (int i0 = 0; i0 < n;)
  {
    int i1 = i0 + 1;
    while (i1 < n && off[(size_t)i1 + 1] - off[(size_t)i0] <= chunk_floats) ++i1;
    if (busy[b] && hipEventSynchronize(done[b]) != hipSuccess)
    {
      cleanup();
      return fail(x, DCP_EFUNCUSE, "staging copy failed");
    }
    float *buf = stage[b];
    std::atomic<int> bad{0};
    // (p: every thread's own copy, reused from protein to protein)
    dcp_parallel_for((size_t)(i1 - i0), 16, 1, 1, [&, p = DcpProtein()](size_t k) mutable {
      int const i = i0 + (int)k;
      int r = db.read_protein(first + i, p);
      if (r || p.core_size != hps[(size_t)i].K)
      {
        int expected = 0;
        bad.compare_exchange_strong(expected, r ? r : DCP_EFDATA);
        return;
      }
      float *rows = buf + (off[(size_t)i] - off[(size_t)i0]);
      float *trans = rows + (size_t)DCP_TABLE_SIZE * ((size_t)hps[(size_t)i].Kp + DCP_ROW_HDR);
      dcp_setup_profile(p.core_size, hps[(size_t)i].Kp, p.trans.data(), p.emission.data(), p.BMk.data(),
                        p.null_emission.data(), p.bg_emission.data(), trans, rows);
      if (!delete_costs_ok(trans, p.core_size, hps[(size_t)i].Kp))
      {
        int expected = 0;
        bad.compare_exchange_strong(expected, DCP_EFDATA); // a positive delete log-probability
      }
      std::fill(rows + canonical_tables(hps[(size_t)i].Kp), rows + canonical_floats(hps[(size_t)i].Kp), INFINITY);
      stage_cost_order(hps[(size_t)i], rows);
    });
    if (bad)
    {
      cleanup();
      return fail(x, bad, "cannot read protein");
    }
    size_t const floats = off[(size_t)i1] - off[(size_t)i0];
    if (hipMemcpyAsync(x->d_pool.p + x->pool_used + off[(size_t)i0], buf, floats * sizeof(float), hipMemcpyHostToDevice,
                       x->stream) != hipSuccess ||
        hipEventRecord(done[b], x->stream) != hipSuccess)
    {
      cleanup();
      return fail(x, DCP_EFUNCUSE, "staging copy failed");
    }
    busy[b] = true;
    b ^= 1;
    i0 = i1;
    ++chunks;
  }
  cleanup();
  x->load_chunks = chunks;
  for (int i = 0; i < n; ++i)
  {
    hps[(size_t)i].pool_off = (int64_t)(x->pool_used + off[(size_t)i]);
    x->profiles.push_back(hps[(size_t)i]);
  }
  x->pool_used += off[(size_t)n];
  ++x->gen;
  return 0;
}

} // extern "C"

// ---- from a HMMER3 file: the tables are made on the device and stay there ---------------------------------
// Profiles are parsed into batches as press does (press_batch.h).  Per batch, queued on the engine's stream: the
// nodes' distributions and the host-made transitions go up, the emission kernel (press_kernel.hip) writes the
// node-major tables into a scratch buffer of the slot, and the rows kernel (press_rows.hip) writes every profile's rows,
// cost-order copy and transitions into its slice of the pool.  Two slots: the host parses batch b + 1 while the GPU
// works on b.  Nothing comes back, and the profiles are published to the engine only when the whole range is in.
namespace
{

struct HmmSlot : DcpPressBatch
{
  PinBuf<float> h_in, h_trans;
  PinBuf<DcpRowsDesc> h_desc;
  DevBuf<float> d_em, d_trans; // (the inputs go up into the engine's kept distributions, dcp_hip::d_dist)
  DevBuf<DcpRowsDesc> d_desc;
  hipEvent_t ev[4] = {}; // before the uploads, after them, after the emission kernel, after the rows kernel
  bool launched = false;
  ~HmmSlot()
  {
    for (hipEvent_t e : ev)
      if (e) (void)hipEventDestroy(e);
  }
};

struct HmmLoad
{
  dcp_hip *x;
  int gencode;
  float epsilon;
  HmmSlot slot[2];
  PinBuf<float> h_models;            // the null model and the background: two entries in, behind the engine's kept ones ...
  DevBuf<float> d_nullbg;            // ... and their tables, null[1364] then bg[1364]
  size_t used;                       // floats of the pool written so far, the resident profiles included
  // The engine keeps what the emission kernel reads (dcp_hip::d_dist, d_dist_models) for dcp_hip_set_epsilon: the
  // entries go up behind the kept ones and count as kept only when the whole load is in, as the pool's floats do.
  size_t dist_used;                  // node entries written so far, the kept ones included
  size_t const models_at;            // where this load's two model entries lie
  std::vector<HostProfile> added;
  bool poison;
  double t_parse = 0, t_upload = 0, t_emission = 0, t_rows = 0, t_wait = 0, t_grow = 0;
  int grown = 0; // times the pool was reallocated during the load
  HmmLoad(dcp_hip *x_, int gencode_id, float eps)
      : x(x_), gencode(gencode_id), epsilon(eps), used(x_->pool_used), dist_used(x_->dist_used), models_at(x_->dist_models_used)
  {
    char const *e = getenv("DECIPHON_HIP_COST_ORDER");
    poison = e && strcmp(e, "poison") == 0;
  }
  ~HmmLoad() { (void)hipStreamSynchronize(x->stream); } // before the slots' buffers go

  int models(DcpHmmReader const &reader)
  {
    HIP_TRY(x, h_models.reserve(2 * DCP_PRESS_IN_STRIDE), DCP_ENOMEM);
    HIP_TRY(x, d_nullbg.reserve(2 * DCP_PRESS_TABLE), DCP_ENOMEM);
    if (int rc = grow_keeping(x, x->d_dist_models, (models_at + 2) * DCP_PRESS_IN_STRIDE, models_at * DCP_PRESS_IN_STRIDE))
      return rc;
    float *d_models = x->d_dist_models.p + models_at * DCP_PRESS_IN_STRIDE;
    dcp_press_put_entry(h_models.p, reader.null_dist());
    dcp_press_put_entry(h_models.p + DCP_PRESS_IN_STRIDE, reader.bg_dist());
    HIP_TRY(x, hipMemcpyAsync(d_models, h_models.p, 2 * DCP_PRESS_IN_STRIDE * sizeof(float), hipMemcpyHostToDevice, x->stream),
            DCP_EFUNCUSE);
    if (dcp_press_emission_launch(d_models, d_nullbg.p, 2, epsilon, x->stream))
      return fail(x, DCP_EFUNCUSE, "the emission kernel could not be launched");
    for (HmmSlot &s : slot)
      for (hipEvent_t &e : s.ev) HIP_TRY(x, hipEventCreate(&e), DCP_ENOMEM);
    return 0;
  }

  // the kept distributions hold `entries` node entries; a reallocation keeps what is written, as grow() does
  int grow_dist(size_t entries)
  {
    return grow_keeping(x, x->d_dist, entries * DCP_PRESS_IN_STRIDE, dist_used * DCP_PRESS_IN_STRIDE);
  }

  // the pool holds `floats`; a reallocation waits for the stream and copies what is written (timed apart)
  int grow(size_t floats)
  {
    if (floats <= x->d_pool.cap) return 0;
    auto const t0 = std::chrono::steady_clock::now();
    int const rc = ensure_pool(x, floats, used);
    t_grow += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    ++grown;
    return rc;
  }

  // The pool is sized once, from the lengths the file's LENG lines announce for profiles [first, first + count): the
  // load then never reallocates, and nothing is held twice.  Only an estimate -- a file whose LENG lines are not one
  // per profile is not sized by them -- so launch() still grows the pool where it falls short.
  int presize(DcpHmmReader const &reader, long first, long count)
  {
    std::vector<long> const &len = reader.announced_lengths();
    if ((long)len.size() != reader.count()) return 0;
    long const last = count < 0 ? (long)len.size() : std::min((long)len.size(), first + count);
    size_t floats = 0, nodes = 0;
    for (long i = first; i < last; ++i)
    {
      HostProfile hp;
      if (len[(size_t)i] < 1 || len[(size_t)i] >= DCP_MODEL_MAX) return 0; // the load will fail there
      if (describe(x, (int)len[(size_t)i], nullptr, hp)) return 0;
      floats += profile_floats(hp);
      nodes += (size_t)hp.K;
    }
    if (!floats) return 0;
    if (int rc = grow(used + floats)) return rc;
    x->lodds.reserve((dist_used + nodes) * 20); // the kept distributions and log-odds are sized by the same lines
    return grow_dist(dist_used + nodes);
  }

  // the slot's batch is through: its buffers are free again
  int wait(HmmSlot &s)
  {
    if (!s.launched) return 0;
    s.launched = false;
    auto const t0 = std::chrono::steady_clock::now();
    HIP_TRY(x, hipEventSynchronize(s.ev[3]), DCP_EFUNCUSE);
    t_wait += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    float ms[3] = {0, 0, 0};
    for (int i = 0; i < 3; ++i) HIP_TRY(x, hipEventElapsedTime(&ms[i], s.ev[i], s.ev[i + 1]), DCP_EFUNCUSE);
    t_upload += ms[0] * 1e-3;
    t_emission += ms[1] * 1e-3;
    t_rows += ms[2] * 1e-3;
    return 0;
  }

  // describes the profiles of the slot's batch, builds their transitions and queues the batch
  int launch(HmmSlot &s, DcpHmmSink *sink)
  {
    size_t const n = s.profiles.size();
    std::vector<HostProfile> hps(n);
    std::vector<size_t> off(n + 1, 0), toff(n + 1, 0);
    int max_Kp = 0;
    for (size_t i = 0; i < n; ++i)
    {
      if (int rc = describe(x, s.profiles[i].core_size, s.profiles[i].accession.c_str(), hps[i])) return rc;
      off[i + 1] = off[i] + profile_floats(hps[i]);
      toff[i + 1] = toff[i] + (canonical_floats(hps[i].Kp) - (size_t)DCP_TABLE_SIZE * ((size_t)hps[i].Kp + DCP_ROW_HDR));
      max_Kp = std::max(max_Kp, hps[i].Kp);
    }
    size_t const entries = (size_t)s.entries;
    HIP_TRY(x, s.h_in.reserve(entries * DCP_PRESS_IN_STRIDE), DCP_ENOMEM);
    HIP_TRY(x, s.d_em.reserve(entries * DCP_PRESS_TABLE), DCP_ENOMEM);
    HIP_TRY(x, s.h_trans.reserve(toff[n]), DCP_ENOMEM);
    HIP_TRY(x, s.d_trans.reserve(toff[n]), DCP_ENOMEM);
    HIP_TRY(x, s.h_desc.reserve(n), DCP_ENOMEM);
    HIP_TRY(x, s.d_desc.reserve(n), DCP_ENOMEM);
    s.put_entries(s.h_in.p);
    for (size_t i = 0; i < n; ++i)
    {
      HostProfile &hp = hps[i];
      DcpHmmProfile const &p = s.profiles[i];
      float *t = s.h_trans.p + toff[i];
      std::fill(t, s.h_trans.p + toff[i + 1], INFINITY);
      dcp_setup_trans(hp.K, hp.Kp, p.trans.data(), p.BMk.data(), t);
      if (!delete_costs_ok(t, hp.K, hp.Kp)) return fail(x, DCP_EFDATA, "positive (or NaN) delete log-probability in the profile");
      hp.pool_off = (int64_t)(used + off[i]);
      DcpRowsDesc &d = s.h_desc.p[i];
      d.src = s.first[i];
      d.rows_off = hp.pool_off;
      d.trans_off = hp.pool_off + (int64_t)DCP_TABLE_SIZE * (hp.Kp + DCP_ROW_HDR);
      d.trans_src = (int64_t)toff[i];
      d.copy_off = hp.pool_off + (int64_t)canonical_floats(hp.Kp);
      d.K = hp.K;
      d.Kp = hp.Kp;
      d.stride = hp.Kp + DCP_ROW_HDR;
      d.trans_floats = (int32_t)(toff[i + 1] - toff[i]);
      d.cQ = hp.cQ;
      d.poison = hp.cQ && poison;
      hp.dist = (int64_t)dist_used + s.first[i];
      hp.dist_models = (int64_t)models_at;
      hp.epsilon = epsilon;
      hp.gencode = gencode;
      hp.poisoned = d.poison != 0;
    }
    if (int rc = grow(used + off[n])) return rc;
    if (int rc = grow_dist(dist_used + entries)) return rc;
    float *const d_in = x->d_dist.p + dist_used * DCP_PRESS_IN_STRIDE;
    hipStream_t const q = x->stream;
    HIP_TRY(x, hipEventRecord(s.ev[0], q), DCP_EFUNCUSE);
    HIP_TRY(x, hipMemcpyAsync(d_in, s.h_in.p, entries * DCP_PRESS_IN_STRIDE * sizeof(float), hipMemcpyHostToDevice, q), DCP_EFUNCUSE);
    HIP_TRY(x, hipMemcpyAsync(s.d_trans.p, s.h_trans.p, toff[n] * sizeof(float), hipMemcpyHostToDevice, q), DCP_EFUNCUSE);
    HIP_TRY(x, hipMemcpyAsync(s.d_desc.p, s.h_desc.p, n * sizeof(DcpRowsDesc), hipMemcpyHostToDevice, q), DCP_EFUNCUSE);
    HIP_TRY(x, hipEventRecord(s.ev[1], q), DCP_EFUNCUSE);
    if (dcp_press_emission_launch(d_in, s.d_em.p, (int)entries, epsilon, q))
      return fail(x, DCP_EFUNCUSE, "the emission kernel could not be launched");
    HIP_TRY(x, hipEventRecord(s.ev[2], q), DCP_EFUNCUSE);
    if (dcp_press_rows_launch(s.d_em.p, d_nullbg.p, d_nullbg.p + DCP_PRESS_TABLE, s.d_trans.p, s.d_desc.p, (int)n, max_Kp,
                              x->d_pool.p, q))
      return fail(x, DCP_EFUNCUSE, "the rows kernel could not be launched");
    HIP_TRY(x, hipEventRecord(s.ev[3], q), DCP_EFUNCUSE);
    s.launched = true;
    used += off[n];
    dist_used += entries;
    // (behind the kept ones, in the order of the entries; dcp_hip_load_hmm_sink drops them again when the load fails)
    for (DcpHmmProfile const &p : s.profiles) x->lodds.insert(x->lodds.end(), p.lodds.begin(), p.lodds.end());
    if (sink)
      for (DcpHmmProfile const &p : s.profiles) sink->profile(p);
    added.insert(added.end(), hps.begin(), hps.end());
    return 0;
  }
};

} // namespace

int dcp_hip_load_hmm_sink(struct dcp_hip *x, char const *hmm, int gencode_id, float epsilon, int first, int count,
                          DcpHmmSink *sink)
{
  if (!x || !hmm) return DCP_EFUNCUSE;
  if (outstanding_batches(x)) return refuse_outstanding(x);
  {
    DcpNucltDist probe;
    float const zero[20] = {};
    if (!dcp_setup_nuclt_dist(gencode_id, zero, probe)) return fail(x, DCP_EGENCODEID, "unknown translation table");
  }
  if (!(epsilon >= 0.0f && epsilon <= 1.0f)) return fail(x, DCP_EFUNCUSE, "epsilon must lie in [0, 1]");
  if (FILE *f = fopen(hmm, "rb")) fclose(f);
  else return fail(x, DCP_EOPENHMM, "cannot open the HMMER3 file");
  HIP_TRY(x, hipSetDevice(x->device), DCP_EFUNCUSE);
  DcpHmmReader reader;
  int rc = reader.open(hmm, gencode_id);
  if (rc) return fail(x, rc, "cannot read the HMMER3 file");
  // a `first` out of range is reported after what reading the file reports: everything is then in front of it
  bool const bad_first = first < 0 || (long)first > reader.count();
  long skip = bad_first ? LONG_MAX : first, limit = bad_first || count < 0 ? -1 : count;

  HmmLoad load(x, gencode_id, epsilon);
  // the amino log-odds go behind the kept ones batch by batch and count, as the entries in HBM do, once dist_used says so
  struct KeptLodds
  {
    dcp_hip *x;
    ~KeptLodds() { x->lodds.resize(x->dist_used * 20); }
  } kept_lodds{x};
  if ((rc = load.models(reader))) return rc;
  if (!bad_first && (rc = load.presize(reader, first, count))) return rc;
  if (sink) sink->models(reader.null_dist(), reader.bg_dist());
  DcpPressFeeder feeder;
  feeder.batch_nodes = dcp_press_batch_nodes();
  for (int b = 0;; b ^= 1)
  {
    HmmSlot &s = load.slot[b];
    if ((rc = load.wait(s))) break;
    auto const t0 = std::chrono::steady_clock::now();
    feeder.fill(reader, s, &skip, &limit);
    if (!s.profiles.empty()) rc = load.launch(s, sink);
    load.t_parse += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (rc) break;
    if (s.rc_after)
    {
      rc = fail(x, s.rc_after, "cannot read a profile of the HMMER3 file");
      break;
    }
    if (s.eof_after) break;
  }
  for (HmmSlot &s : load.slot)
    if (int const wrc = load.wait(s))
      if (!rc) rc = wrc;
  if (!rc) HIP_TRY(x, hipStreamSynchronize(x->stream), DCP_EFUNCUSE); // (the null and background tables of an empty range)
  if (!rc && bad_first) rc = fail(x, DCP_EINVALPART, "first profile out of range");
  if (rc) return rc; // nothing of this load is kept: pool_used and the profiles are what they were
  if (getenv("DECIPHON_HIP_TIMING"))
    fprintf(stderr,
            "dcp_hip_load_hmm: %zu profiles, %.3f GB of tables; parse %.3f s, upload %.6f s, emission kernel %.6f s, "
            "rows kernel %.6f s, wait %.3f s; pool grown %d times in %.3f s (of parse); kept %zu bytes of distributions\n",
            load.added.size(), (double)(load.used - x->pool_used) * 4e-9, load.t_parse, load.t_upload, load.t_emission,
            load.t_rows, load.t_wait, load.grown, load.t_grow,
            (load.dist_used - x->dist_used + (load.added.empty() ? 0 : 2)) * DCP_PRESS_IN_STRIDE * sizeof(float));
  x->profiles.insert(x->profiles.end(), load.added.begin(), load.added.end());
  x->pool_used = load.used;
  x->dist_used = load.dist_used;
  if (!load.added.empty()) x->dist_models_used = load.models_at + 2; // (an empty range keeps no models either)
  ++x->gen;
  return 0;
}

// what the re-emission kernel needs of one profile with kept distributions (press_reemit.h)
static DcpReemitDesc reemit_desc(HostProfile const &hp)
{
  DcpReemitDesc d;
  d.src = hp.dist;
  d.rows_off = hp.pool_off;
  d.copy_off = hp.pool_off + (int64_t)canonical_floats(hp.Kp);
  d.K = hp.K;
  d.Kp = hp.Kp;
  d.stride = hp.Kp + DCP_ROW_HDR;
  d.cQ = hp.cQ;
  d.poison = hp.poisoned;
  d.null_row = (int32_t)hp.dist_models;
  d.bg_row = d.null_row + 1;
  return d;
}

// the first profile without kept distributions refuses dcp_hip_set_epsilon and dcp_hip_set_gencode
static int refuse_without_dist(dcp_hip *x)
{
  for (size_t i = 0; i < x->profiles.size(); ++i)
    if (x->profiles[i].dist < 0)
    {
      char msg[128];
      snprintf(msg, sizeof msg, "profile %zu has no distributions kept: only dcp_hip_load_hmm keeps them", i);
      return fail(x, DCP_EFUNCUSE, msg);
    }
  return 0;
}

// Every kept entry again under another table: the nodes' from their amino log-odds (dcp_hip::lodds) by
// dcp_regencode_entries, on the host threads, chunk by chunk into two pinned buffers whose uploads overlap the
// recomputation of the next chunk; the null model and the background of every load are the table's.  Then what
// dcp_hip_set_epsilon runs, once per error rate among the profiles: the emission kernel over the models and the
// re-emission kernel over the pairs of the profiles at that rate.
int dcp_hip_set_gencode_sink(struct dcp_hip *x, int gencode_id, DcpGencodeSink *sink)
{
  if (!x) return DCP_EFUNCUSE;
  if (outstanding_batches(x)) return refuse_outstanding(x);
  float null_lprobs[20];
  DcpNucltDist null, bg;
  if (!dcp_setup_models(gencode_id, null_lprobs, null, bg)) return fail(x, DCP_EGENCODEID, "unknown translation table");
  if (int rc = refuse_without_dist(x)) return rc;
  size_t const n = x->profiles.size();
  if (!n) return 0;
  if (x->lodds.size() != x->dist_used * 20) return fail(x, DCP_EFUNCUSE, "the kept amino log-odds do not match the kept distributions");
  HIP_TRY(x, hipSetDevice(x->device), DCP_EFUNCUSE);
  auto const t_begin = std::chrono::steady_clock::now();

  // the profiles by error rate: dcp_press_reemit_launch takes one
  std::vector<float> rates;
  std::vector<std::vector<int32_t>> members;
  std::vector<DcpReemitDesc> desc(n);
  size_t nodes = 0;
  for (size_t i = 0; i < n; ++i)
  {
    HostProfile const &hp = x->profiles[i];
    desc[i] = reemit_desc(hp);
    nodes += (size_t)hp.K;
    size_t g = 0;
    while (g < rates.size() && memcmp(&rates[g], &hp.epsilon, sizeof(float)) != 0) ++g;
    if (g == rates.size())
    {
      rates.push_back(hp.epsilon);
      members.emplace_back();
    }
    members[g].push_back((int32_t)i);
  }
  size_t const groups = rates.size();
  std::vector<int64_t> pair_begin(groups + 1, 0);
  std::vector<std::vector<int32_t>> group_Kp(groups);
  for (size_t g = 0; g < groups; ++g)
  {
    for (int32_t i : members[g]) group_Kp[g].push_back(x->profiles[(size_t)i].Kp);
    pair_begin[g + 1] = pair_begin[g] + dcp_reemit_tiles((int)members[g].size(), group_Kp[g].data(), nullptr, nullptr, 0);
  }
  int64_t const pairs = pair_begin[groups];
  std::vector<int32_t> pair_profile((size_t)pairs), pair_k0((size_t)pairs);
  for (size_t g = 0; g < groups; ++g)
  {
    int64_t const count = pair_begin[g + 1] - pair_begin[g];
    int32_t *pp = pair_profile.data() + pair_begin[g];
    (void)dcp_reemit_tiles((int)members[g].size(), group_Kp[g].data(), pp, pair_k0.data() + pair_begin[g], count);
    for (int64_t j = 0; j < count; ++j) pp[j] = members[g][(size_t)pp[j]]; // of the group -> of the engine
  }

  // everything that can fail for want of memory, before the first byte of device memory changes
  size_t const models = x->dist_models_used, kept = x->dist_used;
  size_t chunk = ((size_t)64 << 20) / (DCP_PRESS_IN_STRIDE * sizeof(float));
  if (char const *e = getenv("DECIPHON_HIP_STAGE_MB"))
    chunk = std::max<size_t>(((size_t)std::max(atol(e), 1L) << 20) / (DCP_PRESS_IN_STRIDE * sizeof(float)), 1);
  chunk = std::min(chunk, kept);
  DevBuf<DcpReemitDesc> d_desc;
  DevBuf<int32_t> d_pair_profile, d_pair_k0;
  DevBuf<float> d_tables; // per error rate, the null and background tables of every kept model entry
  PinBuf<float> h_models, stage[2];
  struct Event
  {
    hipEvent_t e = nullptr;
    ~Event()
    {
      if (e) (void)hipEventDestroy(e);
    }
  } up0[2], up1[2], ker[2];
  HIP_TRY(x, d_desc.reserve(n), DCP_ENOMEM);
  HIP_TRY(x, d_pair_profile.reserve((size_t)pairs), DCP_ENOMEM);
  HIP_TRY(x, d_pair_k0.reserve((size_t)pairs), DCP_ENOMEM);
  HIP_TRY(x, d_tables.reserve(groups * models * DCP_PRESS_TABLE), DCP_ENOMEM);
  HIP_TRY(x, h_models.reserve(models * DCP_PRESS_IN_STRIDE), DCP_ENOMEM);
  for (int b = 0; b < 2; ++b)
  {
    HIP_TRY(x, stage[b].reserve(chunk * DCP_PRESS_IN_STRIDE), DCP_ENOMEM);
    HIP_TRY(x, hipEventCreate(&up0[b].e), DCP_ENOMEM);
    HIP_TRY(x, hipEventCreate(&up1[b].e), DCP_ENOMEM);
    HIP_TRY(x, hipEventCreate(&ker[b].e), DCP_ENOMEM);
  }
  // (until the stream is idle the pinned buffers stay: an early return below waits for what it queued)
  struct Drain
  {
    hipStream_t q;
    ~Drain() { (void)hipStreamSynchronize(q); }
  } drain{x->stream};
  HIP_TRY(x, hipMemcpy(d_desc.p, desc.data(), n * sizeof(DcpReemitDesc), hipMemcpyHostToDevice), DCP_EFUNCUSE);
  HIP_TRY(x, hipMemcpy(d_pair_profile.p, pair_profile.data(), (size_t)pairs * sizeof(int32_t), hipMemcpyHostToDevice), DCP_EFUNCUSE);
  HIP_TRY(x, hipMemcpy(d_pair_k0.p, pair_k0.data(), (size_t)pairs * sizeof(int32_t), hipMemcpyHostToDevice), DCP_EFUNCUSE);

  // from here on the kept distributions change
  hipStream_t const q = x->stream;
  if (sink) sink->regencoded(gencode_id, null, bg);
  for (size_t m = 0; m + 1 < models; m += 2)
  {
    dcp_press_put_entry(h_models.p + m * DCP_PRESS_IN_STRIDE, null);
    dcp_press_put_entry(h_models.p + (m + 1) * DCP_PRESS_IN_STRIDE, bg);
  }
  HIP_TRY(x, hipMemcpyAsync(x->d_dist_models.p, h_models.p, models * DCP_PRESS_IN_STRIDE * sizeof(float), hipMemcpyHostToDevice, q),
          DCP_EFUNCUSE);
  double t_host = 0, t_upload = 0;
  bool busy[2] = {false, false};
  auto uploaded = [&](int b) -> int {
    if (!busy[b]) return 0;
    busy[b] = false;
    float ms = 0;
    HIP_TRY(x, hipEventSynchronize(up1[b].e), DCP_EFUNCUSE);
    HIP_TRY(x, hipEventElapsedTime(&ms, up0[b].e, up1[b].e), DCP_EFUNCUSE);
    t_upload += ms * 1e-3;
    return 0;
  };
  int b = 0;
  for (size_t c0 = 0; c0 < kept; c0 += chunk, b ^= 1)
  {
    size_t const c = std::min(chunk, kept - c0);
    if (int rc = uploaded(b)) return rc;
    auto const t0 = std::chrono::steady_clock::now();
    (void)dcp_regencode_entries(gencode_id, (int64_t)c, x->lodds.data() + 20 * c0, 16, stage[b].p); // (the table is held)
    t_host += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (sink) sink->entries(c0, c, stage[b].p);
    HIP_TRY(x, hipEventRecord(up0[b].e, q), DCP_EFUNCUSE);
    HIP_TRY(x, hipMemcpyAsync(x->d_dist.p + c0 * DCP_PRESS_IN_STRIDE, stage[b].p, c * DCP_PRESS_IN_STRIDE * sizeof(float),
                              hipMemcpyHostToDevice, q),
            DCP_EFUNCUSE);
    HIP_TRY(x, hipEventRecord(up1[b].e, q), DCP_EFUNCUSE);
    busy[b] = true;
  }
  HIP_TRY(x, hipEventRecord(ker[0].e, q), DCP_EFUNCUSE);
  for (size_t g = 0; g < groups; ++g)
  {
    float *tables = d_tables.p + g * models * DCP_PRESS_TABLE;
    if (dcp_press_emission_launch(x->d_dist_models.p, tables, (int)models, rates[g], q))
      return fail(x, DCP_EFUNCUSE, "the emission kernel could not be launched");
    if (dcp_press_reemit_launch(x->d_dist.p, tables, d_desc.p, d_pair_profile.p + pair_begin[g], d_pair_k0.p + pair_begin[g],
                                pair_begin[g + 1] - pair_begin[g], rates[g], x->d_pool.p, q))
      return fail(x, DCP_EFUNCUSE, "the re-emission kernel could not be launched");
  }
  HIP_TRY(x, hipEventRecord(ker[1].e, q), DCP_EFUNCUSE);
  for (int s = 0; s < 2; ++s)
    if (int rc = uploaded(s)) return rc;
  HIP_TRY(x, hipStreamSynchronize(q), DCP_EFUNCUSE);
  if (getenv("DECIPHON_HIP_TIMING"))
  {
    float ms = 0;
    HIP_TRY(x, hipEventElapsedTime(&ms, ker[0].e, ker[1].e), DCP_EFUNCUSE);
    fprintf(stderr,
            "dcp_hip_set_gencode: %zu profiles, %zu nodes, table %d, %zu error rates; host recomputation %.6f s, upload %.6f s, "
            "kernels %.6f s, wall %.6f s\n",
            n, nodes, gencode_id, groups, t_host, t_upload, ms * 1e-3,
            std::chrono::duration<double>(std::chrono::steady_clock::now() - t_begin).count());
  }
  for (HostProfile &hp : x->profiles) hp.gencode = gencode_id;
  ++x->gen;
  return 0;
}

extern "C" {

int dcp_hip_load_hmm(struct dcp_hip *x, char const *hmm, int gencode_id, float epsilon, int first, int count)
{
  return dcp_hip_load_hmm_sink(x, hmm, gencode_id, epsilon, first, count, nullptr);
}

// Every profile's rows, cost-order copy and headers again, at `epsilon`, from the kept distributions: the null and
// background tables of every load by the emission kernel, then one launch of the re-emission kernel (press_reemit.hip)
// over all (profile, 64 positions) pairs.  The descriptors and the pair list are built here and uploaded: 56 bytes per
// profile and 8 per pair.
int dcp_hip_set_epsilon(struct dcp_hip *x, float epsilon)
{
  if (!x) return DCP_EFUNCUSE;
  if (outstanding_batches(x)) return refuse_outstanding(x);
  if (!(epsilon >= 0.0f && epsilon <= 1.0f)) return fail(x, DCP_EFUNCUSE, "epsilon must lie in [0, 1]");
  size_t const n = x->profiles.size();
  if (int rc = refuse_without_dist(x)) return rc;
  if (!n) return 0;
  HIP_TRY(x, hipSetDevice(x->device), DCP_EFUNCUSE);

  std::vector<DcpReemitDesc> desc(n);
  std::vector<int32_t> Kp(n);
  size_t nodes = 0, written = 0;
  for (size_t i = 0; i < n; ++i)
  {
    HostProfile const &hp = x->profiles[i];
    DcpReemitDesc &d = desc[i] = reemit_desc(hp);
    Kp[i] = hp.Kp;
    nodes += (size_t)hp.K;
    written += (size_t)DCP_TABLE_SIZE * ((size_t)d.stride + (hp.cQ ? (size_t)dcp_cost_order_stride(hp.cQ, hp.cW) : 0));
  }
  int64_t const pairs = dcp_reemit_tiles((int)n, Kp.data(), nullptr, nullptr, 0);
  std::vector<int32_t> pair_profile((size_t)pairs), pair_k0((size_t)pairs);
  (void)dcp_reemit_tiles((int)n, Kp.data(), pair_profile.data(), pair_k0.data(), pairs);

  DevBuf<DcpReemitDesc> d_desc;
  DevBuf<int32_t> d_pair_profile, d_pair_k0;
  DevBuf<float> d_tables; // the null and background tables at the new error rate, one row per kept model entry
  struct Event
  {
    hipEvent_t e = nullptr;
    ~Event()
    {
      if (e) (void)hipEventDestroy(e);
    }
  } ev[2];
  HIP_TRY(x, d_desc.reserve(n), DCP_ENOMEM);
  HIP_TRY(x, d_pair_profile.reserve((size_t)pairs), DCP_ENOMEM);
  HIP_TRY(x, d_pair_k0.reserve((size_t)pairs), DCP_ENOMEM);
  HIP_TRY(x, d_tables.reserve(x->dist_models_used * DCP_PRESS_TABLE), DCP_ENOMEM);
  for (Event &e : ev) HIP_TRY(x, hipEventCreate(&e.e), DCP_ENOMEM);
  HIP_TRY(x, hipMemcpy(d_desc.p, desc.data(), n * sizeof(DcpReemitDesc), hipMemcpyHostToDevice), DCP_EFUNCUSE);
  HIP_TRY(x, hipMemcpy(d_pair_profile.p, pair_profile.data(), (size_t)pairs * sizeof(int32_t), hipMemcpyHostToDevice), DCP_EFUNCUSE);
  HIP_TRY(x, hipMemcpy(d_pair_k0.p, pair_k0.data(), (size_t)pairs * sizeof(int32_t), hipMemcpyHostToDevice), DCP_EFUNCUSE);
  hipStream_t const q = x->stream;
  if (dcp_press_emission_launch(x->d_dist_models.p, d_tables.p, (int)x->dist_models_used, epsilon, q))
    return fail(x, DCP_EFUNCUSE, "the emission kernel could not be launched");
  HIP_TRY(x, hipEventRecord(ev[0].e, q), DCP_EFUNCUSE);
  if (dcp_press_reemit_launch(x->d_dist.p, d_tables.p, d_desc.p, d_pair_profile.p, d_pair_k0.p, pairs, epsilon, x->d_pool.p, q))
    return fail(x, DCP_EFUNCUSE, "the re-emission kernel could not be launched");
  HIP_TRY(x, hipEventRecord(ev[1].e, q), DCP_EFUNCUSE);
  HIP_TRY(x, hipStreamSynchronize(q), DCP_EFUNCUSE);
  if (getenv("DECIPHON_HIP_TIMING"))
  {
    float ms = 0;
    HIP_TRY(x, hipEventElapsedTime(&ms, ev[0].e, ev[1].e), DCP_EFUNCUSE);
    fprintf(stderr, "dcp_hip_set_epsilon: %zu profiles, %zu nodes, %zu bytes written; re-emission kernel %.6f s\n", n, nodes,
            written * sizeof(float), ms * 1e-3);
  }
  for (HostProfile &hp : x->profiles) hp.epsilon = epsilon;
  ++x->gen;
  return 0;
}

float dcp_hip_profile_epsilon(struct dcp_hip const *x, int i)
{
  if (!x || i < 0 || i >= (int)x->profiles.size() || x->profiles[(size_t)i].dist < 0) return NAN;
  return x->profiles[(size_t)i].epsilon;
}

int dcp_hip_set_gencode(struct dcp_hip *x, int gencode_id) { return dcp_hip_set_gencode_sink(x, gencode_id, nullptr); }

int dcp_hip_profile_gencode(struct dcp_hip const *x, int i)
{
  if (!x || i < 0 || i >= (int)x->profiles.size() || x->profiles[(size_t)i].dist < 0) return 0;
  return x->profiles[(size_t)i].gencode;
}

int64_t dcp_hip_dist_bytes(struct dcp_hip const *x)
{
  return x ? (int64_t)((x->dist_used + x->dist_models_used) * DCP_PRESS_IN_STRIDE * sizeof(float)) : 0;
}

int64_t dcp_hip_profile_floats(struct dcp_hip const *x, int i)
{
  if (!x || i < 0 || i >= (int)x->profiles.size()) return -1;
  return (int64_t)profile_floats(x->profiles[(size_t)i]);
}

int dcp_hip_profile_read(struct dcp_hip const *x, int i, float *out, int64_t n)
{
  if (!x || !out || i < 0 || i >= (int)x->profiles.size()) return DCP_EFUNCUSE;
  HostProfile const &hp = x->profiles[(size_t)i];
  if (n != (int64_t)profile_floats(hp)) return DCP_EFUNCUSE;
  // (every load has waited for its own copies and kernels before it returned)
  if (hipSetDevice(x->device) != hipSuccess) return DCP_EFUNCUSE;
  if (hipMemcpy(out, x->d_pool.p + hp.pool_off, (size_t)n * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) return DCP_EFUNCUSE;
  return 0;
}

int dcp_hip_num_profiles(struct dcp_hip const *x) { return x ? (int)x->profiles.size() : 0; }

int dcp_hip_load_chunks(struct dcp_hip const *x) { return x ? x->load_chunks : 0; }

int64_t dcp_hip_pool_bytes(struct dcp_hip const *x) { return x ? (int64_t)(x->pool_used * sizeof(float)) : 0; }

int dcp_hip_profile_core_size(struct dcp_hip const *x, int i)
{
  if (!x || i < 0 || i >= (int)x->profiles.size()) return -1;
  return x->profiles[(size_t)i].K;
}

char const *dcp_hip_profile_accession(struct dcp_hip const *x, int i)
{
  if (!x || i < 0 || i >= (int)x->profiles.size()) return nullptr;
  return x->profiles[(size_t)i].accession.c_str();
}

int dcp_hip_commit_profiles(struct dcp_hip *x)
{
  if (!x) return DCP_EFUNCUSE;
  if (outstanding_batches(x)) return refuse_outstanding(x);
  HIP_TRY(x, hipSetDevice(x->device), DCP_EFUNCUSE);
  ++x->gen; // even when there is nothing new to publish (the header: every accepted commit)
  if (x->committed == x->profiles.size()) return 0;
  // the tables are already in HBM; what is published here are the profile descriptors
  HIP_TRY(x, hipStreamSynchronize(x->stream), DCP_EFUNCUSE);
  std::vector<DcpProfileDev> dev(x->profiles.size());
  for (size_t i = 0; i < dev.size(); ++i)
  {
    HostProfile const &hp = x->profiles[i];
    dev[i].K = hp.K;
    dev[i].Kp = hp.Kp;
    dev[i].Q = hp.Q;
    dev[i].W = hp.W;
    dev[i].rows_off = hp.pool_off;
    dev[i].trans_off = dev[i].rows_off + (int64_t)DCP_TABLE_SIZE * (hp.Kp + DCP_ROW_HDR);
    dev[i].cost_rows_off = hp.cQ ? hp.pool_off + (int64_t)canonical_floats(hp.Kp) : 0;
    dev[i].cost_shape = hp.cQ ? DCP_COST_SHAPE(hp.cQ, hp.cW) : 0;
  }
  HIP_TRY(x, x->d_profiles.reserve(dev.size()), DCP_ENOMEM);
  HIP_TRY(x, hipMemcpyAsync(x->d_profiles.p, dev.data(), dev.size() * sizeof(DcpProfileDev), hipMemcpyHostToDevice,
                            x->stream),
          DCP_EFUNCUSE);
  HIP_TRY(x, hipStreamSynchronize(x->stream), DCP_EFUNCUSE);
  x->committed = x->profiles.size();
  return 0;
}

void dcp_hip_clear_profiles(struct dcp_hip *x)
{
  if (!x) return;
  if (outstanding_batches(x))
  {
    (void)refuse_outstanding(x); // void in the ABI: the refusal shows in dcp_hip_strerror and num_profiles
    return;
  }
  ++x->gen;
  x->pool_used = 0;
  x->profiles.clear();
  x->committed = 0;
  x->dist_used = x->dist_models_used = 0;
  std::vector<float>().swap(x->lodds);
  (void)hipSetDevice(x->device);
  x->d_dist.release();
  x->d_dist_models.release();
}

} // extern "C"
