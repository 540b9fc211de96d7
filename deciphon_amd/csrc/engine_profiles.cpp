// engine_profiles.cpp -- the engine's profiles: add, load from a pressed file, commit, clear, the cost-order staging and
// the read-only queries.  Loads from a HMMER3 file and what re-presses their profiles in place: engine_hmm.cpp.
#include "engine_internal.h"
#include "parallel_for.h"
#include "../../include/deciphon_host.h"

// ---- profiles: HBM is the only resident copy ---------------------------------------
// A profile is laid out on the host in a staging buffer (ProfileLayout: rows | trans, +inf padded) and
// copied behind the profiles already resident; nothing Pfam-sized is ever held twice.

// The cost-order copy (host_logic.h) of the staged rows, behind the profile's canonical tables, for the profiles whose
// default cost kernel is a narrow one (dcp_launch_cost_narrow) that gains from it: (5,1) and (10,1), K = 257..320 and
// 513..640.  Their tail chunks of one and two floats were the most strided loads; per class they run 7-10 % and 6-8 %
// faster on the copy, while (6,1), (7,1), (8,1) and (6,2) do not move (profiles/r04_cost_order_ab.txt) -- no copy there.
// Only dcp_cost_kernel<5,1> and <10,1> read it: every other kernel has a shape of its own (the checkpoint and block
// kernels of the path pass run the class shape) and reads the canonical rows.  DECIPHON_HIP_COST_ORDER
// (cost_order_mode) turns the copies off, or poisons the canonical match columns of the profiles that have one.
static bool cost_order_pays(int Q, int W) { return W == 1 && (Q == 5 || Q == 10); }

static void cost_order_shape(HostProfile &hp)
{
  hp.cQ = hp.cW = 0;
  if (!hp.narrow || cost_order_mode() == COST_ORDER_OFF) return;
  int const q = dcp_class_narrow_q(hp.cls);
  if (!cost_order_pays(q, 1)) return;
  hp.cQ = q;
  hp.cW = 1;
}

static void stage_cost_order(HostProfile const &hp, float *staged)
{
  if (!hp.cQ) return;
  ProfileLayout const lay(hp);
  dcp_cost_order_rows(hp.cQ, hp.cW, hp.K, hp.Kp, staged + lay.rows, staged + lay.copy);
  if (cost_order_mode() == COST_ORDER_POISON)
    for (int c = 0; c < DCP_TABLE_SIZE; ++c)
      memset(staged + lay.rows + (size_t)c * lay.stride + DCP_ROW_HDR, 0, sizeof(float) * (size_t)hp.K);
}

namespace dcp_engine
{

bool describe_core_size(int K, StageProfile &p, int &Q, int &W)
{
  int const cls = dcp_class_of(K);
  if (cls < 0) return false;
  p.K = K;
  p.cls = cls;
  dcp_class_shape(cls, &Q, &W);
  p.Kp = 64 * Q * W;
  if (cls == DCP_STRIP_CLASS) p.Kp *= (K + p.Kp - 1) / p.Kp; // whole strips
  p.narrow = K <= dcp_class_narrow_limit(cls);
  p.pack = dcp_pack_shape_of(K);
  if (p.pack >= 0)
  {
    int pq = 0, ps = 0;
    dcp_pack_shape(p.pack, &pq, &ps);
    if (W != 1 || ps * pq > p.Kp) p.pack = -1; // the shape reads S * Q columns of a row
  }
  return true;
}

StageShape const *pack_shapes()
{
  static StageShape const *const shapes = [] {
    static StageShape t[DCP_NUM_PACK_SHAPES];
    for (int s = 0; s < DCP_NUM_PACK_SHAPES; ++s)
    {
      int pq = 0, ps = 0;
      dcp_pack_shape(s, &pq, &ps);
      t[s] = StageShape{64 / ps, dcp_pack_lds_waves(s)};
    }
    return t;
  }();
  return shapes;
}

int describe(dcp_hip *x, int K, char const *accession, HostProfile &hp)
{
  if (K < 1 || K > DCP_MODEL_MAX) return fail(x, DCP_ELARGECORESIZE, "core size out of range");
  if (!describe_core_size(K, hp, hp.Q, hp.W))
    return fail(x, DCP_ELARGECORESIZE, "core size beyond DCP_MAX_CORE_SIZE (16383: state ids keep 14 bits for k + 1)");
  hp.pool_off = 0;
  hp.accession = accession ? accession : "";
  cost_order_shape(hp);
  return 0;
}

int grow_keeping(dcp_hip *x, DevBuf<float> &buf, size_t floats, size_t keep)
{
  if (floats <= buf.cap) return 0;
  HIP_TRY(x, hipStreamSynchronize(x->cost_set.stream), DCP_EFUNCUSE);
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

int ensure_pool(dcp_hip *x, size_t floats, size_t keep)
{
  return grow_keeping(x, x->d_pool, floats, std::max(keep, x->pool_used));
}

// The kernels take E_l = min_k M_l[k] (viterbi_body.h) and bound what a delete run can carry across a
// wavefront (dcp_exchange_publish): both need the delete costs MD, DD to be non-negative, which -log-probabilities
// are.  Anything else (a positive log-probability in a corrupt file, a hand-made table) is refused.
bool delete_costs_ok(float const *trans, int K, int Kp)
{
  for (int k = 0; k < K; ++k)
    if (!(trans[(size_t)DCP_MD * Kp + k] >= 0.0f) || !(trans[(size_t)DCP_DD * Kp + k] >= 0.0f)) return false;
  return true;
}

} // namespace dcp_engine

// What is left to do once a profile's rows and transitions are staged: the delete costs are checked (false: the
// kernels cannot take them), the floats behind trans become +inf and the cost-order copy is made.
static bool finish_staged(HostProfile const &hp, float *staged)
{
  ProfileLayout const lay(hp);
  if (!delete_costs_ok(staged + lay.trans, hp.K, hp.Kp)) return false;
  std::fill(staged + lay.pad_begin, staged + lay.pad_end, INFINITY);
  stage_cost_order(hp, staged);
  return true;
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

// Proteins [first, first + hps.size()) of a pressed database into the pool behind the resident profiles, profile i at
// off[i] floats from there: unpacked and transposed into code-major rows by up to 16 host threads, chunk by chunk of at
// most chunk_floats (never less than one profile), into two pinned staging buffers whose H2D copies overlap the
// unpacking of the next chunk.
static int stage_chunks(dcp_hip *x, DcpDbReader &db, int first, std::vector<HostProfile> const &hps,
                        std::vector<size_t> const &off, size_t chunk_floats, int *chunks)
{
  int const n = (int)hps.size();
  PinBuf<float> stage[2];
  Event done[2];
  bool busy[2] = {false, false};
  for (int b = 0; b < 2; ++b)
    if (stage[b].reserve_exact(std::min(chunk_floats, off[(size_t)n])) != hipSuccess ||
        done[b].create(hipEventDisableTiming) != hipSuccess)
      return fail(x, DCP_ENOMEM, "cannot allocate pinned staging buffers");
  StreamDrain drain{x->cost_set.stream}; // (whichever way this ends: before the staging buffers go)
  int b = 0;
  for (int i0 = 0; i0 < n;)
  {
    int i1 = i0 + 1;
    while (i1 < n && off[(size_t)i1 + 1] - off[(size_t)i0] <= chunk_floats) ++i1;
    if (busy[b] && hipEventSynchronize(done[b].e) != hipSuccess) return fail(x, DCP_EFUNCUSE, "staging copy failed");
    float *buf = stage[b].p;
    std::atomic<int> bad{0};
    // (p: every thread's own copy, reused from protein to protein)
    dcp_parallel_for((size_t)(i1 - i0), 16, 1, 1, [&, p = DcpProtein()](size_t k) mutable {
      int const i = i0 + (int)k;
      HostProfile const &hp = hps[(size_t)i];
      int r = db.read_protein(first + i, p);
      if (r || p.core_size != hp.K)
      {
        int expected = 0;
        bad.compare_exchange_strong(expected, r ? r : DCP_EFDATA);
        return;
      }
      ProfileLayout const lay(hp);
      float *staged = buf + (off[(size_t)i] - off[(size_t)i0]);
      dcp_setup_profile(p.core_size, hp.Kp, p.trans.data(), p.emission.data(), p.BMk.data(), p.null_emission.data(),
                        p.bg_emission.data(), staged + lay.trans, staged + lay.rows);
      if (!finish_staged(hp, staged))
      {
        int expected = 0;
        bad.compare_exchange_strong(expected, DCP_EFDATA); // a positive delete log-probability
      }
    });
    if (bad) return fail(x, bad, "cannot read protein");
    size_t const floats = off[(size_t)i1] - off[(size_t)i0];
    if (hipMemcpyAsync(x->d_pool.p + x->pool_used + off[(size_t)i0], buf, floats * sizeof(float), hipMemcpyHostToDevice,
                       x->cost_set.stream) != hipSuccess ||
        hipEventRecord(done[b].e, x->cost_set.stream) != hipSuccess)
      return fail(x, DCP_EFUNCUSE, "staging copy failed");
    busy[b] = true;
    b ^= 1;
    i0 = i1;
    ++*chunks;
  }
  return 0;
}

extern "C" {

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
  ProfileLayout const lay(hp);
  std::vector<float> buf(lay.total, INFINITY);
  float *r = buf.data() + lay.rows;
  float *t = buf.data() + lay.trans;
  for (int id = 0; id < DCP_NUM_TRANS; ++id) memcpy(t + (size_t)id * Kp, trans + (size_t)id * K, sizeof(float) * K);
  for (int c = 0; c < DCP_TABLE_SIZE; ++c)
  {
    float *hdr = r + (size_t)c * lay.stride;
    hdr[0] = null_cost[c];
    hdr[1] = bg_cost[c];
    hdr[2] = hdr[3] = 0.0f;
    memcpy(hdr + DCP_ROW_HDR, match + (size_t)c * K, sizeof(float) * K);
  }
  if (!finish_staged(hp, buf.data())) return fail(x, DCP_EFUNCUSE, "negative (or NaN) delete cost: costs are -log-probabilities");
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
  ProfileLayout const lay(hp);
  std::vector<float> buf(lay.total, INFINITY);
  dcp_setup_profile(K, hp.Kp, node_trans, node_emission, BMk, null_lprob, bg_lprob, buf.data() + lay.trans, buf.data() + lay.rows);
  if (!finish_staged(hp, buf.data())) return fail(x, DCP_EFDATA, "positive (or NaN) delete log-probability in the protein");
  return push_profile(x, hp, buf, index);
}

// Streams proteins [first, first+count) of a pressed database into HBM: core sizes are read
// first (so the pool is sized once), then the proteins go up through stage_chunks.
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
  size_t largest = 0;
  for (int i = 0; i < n; ++i)
  {
    int K = 0;
    std::string acc;
    if ((rc = db.read_protein_head(first + i, K, acc))) return fail(x, rc, "cannot read protein");
    if ((rc = describe(x, K, acc.c_str(), hps[(size_t)i]))) return rc;
    size_t const floats = ProfileLayout(hps[(size_t)i]).total;
    off[(size_t)i + 1] = off[(size_t)i] + floats;
    largest = std::max(largest, floats);
  }
  if ((rc = ensure_pool(x, x->pool_used + off[(size_t)n]))) return rc;

  // staging chunks of 256 MiB; DECIPHON_HIP_STAGE_MB shrinks them (never below one profile of the largest
  // size present), which is how the tests drive a small database through many chunks
  size_t const chunk_floats = std::max(stage_bytes((size_t)256 << 20) / sizeof(float), largest);
  int chunks = 0;
  if ((rc = stage_chunks(x, db, first, hps, off, chunk_floats, &chunks))) return rc;
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

int64_t dcp_hip_profile_floats(struct dcp_hip const *x, int i)
{
  if (!x || i < 0 || i >= (int)x->profiles.size()) return -1;
  return (int64_t)ProfileLayout(x->profiles[(size_t)i]).total;
}

int dcp_hip_profile_read(struct dcp_hip const *x, int i, float *out, int64_t n)
{
  if (!x || !out || i < 0 || i >= (int)x->profiles.size()) return DCP_EFUNCUSE;
  HostProfile const &hp = x->profiles[(size_t)i];
  if (n != (int64_t)ProfileLayout(hp).total) return DCP_EFUNCUSE;
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
  HIP_TRY(x, hipStreamSynchronize(x->cost_set.stream), DCP_EFUNCUSE);
  std::vector<DcpProfileDev> dev(x->profiles.size());
  for (size_t i = 0; i < dev.size(); ++i)
  {
    HostProfile const &hp = x->profiles[i];
    ProfileLayout const lay(hp);
    dev[i].K = hp.K;
    dev[i].Kp = hp.Kp;
    dev[i].Q = hp.Q;
    dev[i].W = hp.W;
    dev[i].rows_off = hp.pool_off + (int64_t)lay.rows;
    dev[i].trans_off = hp.pool_off + (int64_t)lay.trans;
    dev[i].cost_rows_off = hp.cQ ? hp.pool_off + (int64_t)lay.copy : 0;
    dev[i].cost_shape = hp.cQ ? DCP_COST_SHAPE(hp.cQ, hp.cW) : 0;
  }
  HIP_TRY(x, x->d_profiles.reserve(dev.size()), DCP_ENOMEM);
  HIP_TRY(x, hipMemcpyAsync(x->d_profiles.p, dev.data(), dev.size() * sizeof(DcpProfileDev), hipMemcpyHostToDevice,
                            x->cost_set.stream),
          DCP_EFUNCUSE);
  HIP_TRY(x, hipStreamSynchronize(x->cost_set.stream), DCP_EFUNCUSE);
  x->committed = x->profiles.size();
  x->plan_profiles.assign(x->profiles.begin(), x->profiles.end());
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
  drop_calibration(x);
  x->pool_used = 0;
  x->profiles.clear();
  x->plan_profiles.clear();
  x->committed = 0;
  x->dist_used = x->dist_models_used = 0;
  std::vector<float>().swap(x->lodds);
  (void)hipSetDevice(x->device);
  x->d_dist.release();
  x->d_dist_models.release();
}

// ---- include/deciphon_host.h: what the engine decides for a core size and a pack shape, without a device ----
int dcp_engine_core_size(int K, int32_t out[4])
{
  StageProfile p;
  int Q = 0, W = 0;
  if (!out) return DCP_EFUNCUSE;
  if (K < 1 || K > DCP_MODEL_MAX || !describe_core_size(K, p, Q, W)) return DCP_ELARGECORESIZE;
  out[0] = p.cls, out[1] = p.narrow, out[2] = p.pack, out[3] = p.Kp;
  return 0;
}

int dcp_engine_pack_shape(int shape, int32_t out[2])
{
  if (shape < 0 || shape >= DCP_NUM_PACK_SHAPES || !out) return DCP_EFUNCUSE;
  out[0] = pack_shapes()[shape].windows, out[1] = pack_shapes()[shape].lds_waves;
  return 0;
}

} // extern "C"
