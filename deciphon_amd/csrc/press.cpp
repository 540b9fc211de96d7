// press.cpp -- dcp_press_* of include/deciphon.h: HMMER3 text in, a pressed .dcp database out.
//
// Replaces c-core/press.c (the call sequence), c-core/database_writer.c (records streamed to a temporary file, the
// header written at close) and protein_pack (c-core/protein.c:234-281) in the current encoding: f32 arrays as
// `bin` + little-endian floats (c-core/write.c:59-66), the layout deciphon_amd/synth.py pack_protein(legacy=False)
// writes too.  The profile model is host code (hmm_model.h); the emission tables -- 1364 floats per node, nearly all
// of the file -- are made on the GPU (press_kernel.hip).
//
// Read-ahead: profiles are parsed into batches of up to DCP_PRESS_BATCH_NODES nodes, and each batch's tables are
// computed by one launch into one of two pinned buffer sets.  When dcp_press_next first takes a profile of batch b,
// batch b + 1 is parsed and launched (while b's kernel may still run) before b is waited for; the host then writes
// b's records while the GPU works on b + 1.  The calls keep the reference's meaning: one protein per next, end()
// true after the call that found no protein left, and a parse error returned by the next that reaches that protein.
#include "../../include/deciphon.h"
#include "dcp_errors.h"
#include "dcp_types.h"
#include "hmm_model.h"
#include "press_batch.h"
#include "press_kernel.h"

#include <hip/hip_runtime.h>

#include <chrono>
#include <errno.h>
#include <fcntl.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <sys/stat.h>
#include <unistd.h>
#include <vector>

namespace
{

double now()
{
  return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// ---- MessagePack, the forms the writer needs ----
struct Pack
{
  std::vector<uint8_t> b;
  void u8(uint8_t v) { b.push_back(v); }
  void be(uint64_t v, int n)
  {
    for (int i = n - 1; i >= 0; --i) b.push_back((uint8_t)(v >> (8 * i)));
  }
  void uint(uint64_t v)
  {
    if (v < 128) u8((uint8_t)v);
    else if (v < (1u << 8)) u8(0xcc), be(v, 1);
    else if (v < (1u << 16)) u8(0xcd), be(v, 2);
    else if (v <= 0xffffffffu) u8(0xce), be(v, 4);
    else u8(0xcf), be(v, 8);
  }
  void str(std::string const &s)
  {
    size_t const n = s.size();
    if (n < 32) u8((uint8_t)(0xa0 | n));
    else if (n < (1u << 8)) u8(0xd9), be(n, 1);
    else if (n < (1u << 16)) u8(0xda), be(n, 2);
    else u8(0xdb), be(n, 4);
    b.insert(b.end(), s.begin(), s.end());
  }
  void map(uint32_t n) { n < 16 ? u8((uint8_t)(0x80 | n)) : n < (1u << 16) ? (u8(0xde), be(n, 2)) : (u8(0xdf), be(n, 4)); }
  void array(uint32_t n) { n < 16 ? u8((uint8_t)(0x90 | n)) : n < (1u << 16) ? (u8(0xdc), be(n, 2)) : (u8(0xdd), be(n, 4)); }
  void f32(float v)
  {
    uint32_t u;
    memcpy(&u, &v, 4);
    u8(0xca);
    be(u, 4);
  }
  void f32array(float const *v, size_t n) // write_f32array: bin + native (little-endian) floats
  {
    size_t const bytes = 4 * n;
    if (bytes < (1u << 8)) u8(0xc4), be(bytes, 1);
    else if (bytes < (1u << 16)) u8(0xc5), be(bytes, 2);
    else u8(0xc6), be(bytes, 4);
    uint8_t const *p = (uint8_t const *)v;
    b.insert(b.end(), p, p + bytes);
  }
  void nuclt_dist(DcpNucltDist const &d) // nuclt_dist_pack, c-core/nuclt_dist.c:13-20
  {
    array(2);
    f32array(d.nucltp, 4);
    f32array(d.codonm, 125);
  }
  // imm_abc_pack: symbols, the index of every printable character (33..126, 127 = not a symbol; the any-symbol 'X'
  // follows the symbols; the last entry is 0 in the reference's files), any_symbol_id and the alphabet type
  void abc(char const *symbols, int typeid_)
  {
    uint8_t idx[94];
    memset(idx, 127, sizeof idx);
    size_t const n = strlen(symbols);
    for (size_t i = 0; i < n; ++i) idx[symbols[i] - 33] = (uint8_t)i;
    idx['X' - 33] = (uint8_t)n;
    idx[93] = 0;
    map(4);
    str("symbols");
    str(symbols);
    str("idx");
    u8(0xc7), u8(sizeof idx), u8(0); // ext 8, type 0
    b.insert(b.end(), idx, idx + sizeof idx);
    str("any_symbol_id");
    uint('X' - 33);
    str("typeid");
    uint((uint64_t)typeid_);
  }
};

int write_all(int fd, void const *data, size_t n)
{
  uint8_t const *p = (uint8_t const *)data;
  while (n)
  {
    ssize_t const w = ::write(fd, p, n);
    if (w < 0 && errno == EINTR) continue;
    if (w <= 0) return DCP_EFWRITE;
    p += w;
    n -= (size_t)w;
  }
  return 0;
}

struct Slot : DcpPressBatch
{
  int64_t cap = 0;
  float *h_in = nullptr, *h_out = nullptr, *d_in = nullptr, *d_out = nullptr;
  hipEvent_t ev[4] = {}; // before upload, after upload, after the kernel, after the copy-back
  bool launched = false, waited = true;
  void release()
  {
    if (h_in) (void)hipHostFree(h_in);
    if (h_out) (void)hipHostFree(h_out);
    if (d_in) (void)hipFree(d_in);
    if (d_out) (void)hipFree(d_out);
    h_in = h_out = d_in = d_out = nullptr;
    cap = 0;
    for (hipEvent_t &e : ev)
      if (e) (void)hipEventDestroy(e), e = nullptr;
  }
};

} // namespace

struct dcp_press
{
  bool ready = false; // dcp_press_setup has succeeded
  int gencode = 0;
  float epsilon = 0;
  enum { IDLE, OPEN, FAILED } state = IDLE;
  bool end = false;
  long count = 0;
  DcpHmmReader reader;
  std::string db_path, tmp_path;
  int db_fd = -1, tmp_fd = -1;
  bool has_ga = true;
  std::vector<uint32_t> sizes;
  // GPU
  int device = 0;
  hipStream_t stream = nullptr;
  DcpPressFeeder feeder; // batch by batch out of `reader`
  Slot slots[2];
  int cur = 0;     // the slot next() takes profiles from
  size_t pos = 0;  // next profile of it
  std::vector<float> null_table, bg_table;
  Pack rec;
  double timing[DCP_PRESS_TIMING_VALUES] = {0};
};

namespace
{

int loglevel() // c-core/loglevel.c:9-16
{
  char const *x = getenv("DECIPHON_LOGLEVEL");
  return x ? atoi(x) : 2;
}

int raise(int rc, char const *func, char const *detail = nullptr) // c-core/error.c:103-121
{
  if (rc && loglevel() <= 2)
    fprintf(stderr, "%s %s%s%s.\n", func, dcp_error_string(rc), detail ? ". Detail: " : "", detail ? detail : "");
  return rc;
}

// grows a slot's buffers to hold n entries (the slot is not in flight)
int reserve(Slot &s, int64_t n)
{
  if (n <= s.cap) return 0;
  s.release();
  int64_t const want = n < 256 ? 256 : n;
  bool ok = hipHostMalloc((void **)&s.h_in, (size_t)want * DCP_PRESS_IN_STRIDE * 4, hipHostMallocDefault) == hipSuccess;
  ok = ok && hipHostMalloc((void **)&s.h_out, (size_t)want * DCP_PRESS_TABLE * 4, hipHostMallocDefault) == hipSuccess;
  ok = ok && hipMalloc((void **)&s.d_in, (size_t)want * DCP_PRESS_IN_STRIDE * 4) == hipSuccess;
  ok = ok && hipMalloc((void **)&s.d_out, (size_t)want * DCP_PRESS_TABLE * 4) == hipSuccess;
  for (hipEvent_t &e : s.ev) ok = ok && hipEventCreate(&e) == hipSuccess;
  if (!ok)
  {
    s.release();
    return DCP_ENOMEM;
  }
  s.cap = want;
  return 0;
}

// uploads the slot's s.entries inputs (already in h_in), computes their tables and copies them back, all queued
int launch(dcp_press *x, Slot &s)
{
  s.launched = false;
  s.waited = false;
  if (!s.entries) return 0;
  size_t const n = (size_t)s.entries;
  bool ok = hipEventRecord(s.ev[0], x->stream) == hipSuccess;
  ok = ok && hipMemcpyAsync(s.d_in, s.h_in, n * DCP_PRESS_IN_STRIDE * 4, hipMemcpyHostToDevice, x->stream) == hipSuccess;
  ok = ok && hipEventRecord(s.ev[1], x->stream) == hipSuccess;
  ok = ok && dcp_press_emission_launch(s.d_in, s.d_out, (int)n, x->epsilon, x->stream) == 0;
  ok = ok && hipEventRecord(s.ev[2], x->stream) == hipSuccess;
  ok = ok && hipMemcpyAsync(s.h_out, s.d_out, n * DCP_PRESS_TABLE * 4, hipMemcpyDeviceToHost, x->stream) == hipSuccess;
  ok = ok && hipEventRecord(s.ev[3], x->stream) == hipSuccess;
  s.launched = ok;
  return ok ? 0 : DCP_EFUNCUSE;
}

int wait(dcp_press *x, Slot &s)
{
  if (s.waited) return 0;
  s.waited = true;
  if (!s.launched) return 0;
  double const t0 = now();
  if (hipEventSynchronize(s.ev[3]) != hipSuccess) return DCP_EFUNCUSE;
  x->timing[4] += now() - t0;
  float ms[3] = {0, 0, 0};
  for (int i = 0; i < 3; ++i)
    if (hipEventElapsedTime(&ms[i], s.ev[i], s.ev[i + 1]) != hipSuccess) return DCP_EFUNCUSE;
  for (int i = 0; i < 3; ++i) x->timing[1 + i] += ms[i] * 1e-3;
  return 0;
}

// parses the next batch of profiles into slot s and queues its tables
int fill(dcp_press *x, Slot &s)
{
  double const t0 = now();
  x->feeder.fill(x->reader, s);
  if (int rc = reserve(s, s.entries)) return rc;
  s.put_entries(s.h_in);
  x->timing[0] += now() - t0;
  return launch(x, s);
}

// protein_pack (c-core/protein.c:234-281) of profile i of slot s, appended to the temporary file
int write_protein(dcp_press *x, Slot const &s, size_t i)
{
  double const t0 = now();
  DcpHmmProfile const &p = s.profiles[i];
  int const K = p.core_size;
  Pack &r = x->rec;
  r.b.clear();
  r.map(10);
  r.str("accession");
  r.str(p.accession);
  r.str("gencode");
  r.uint((uint64_t)x->gencode);
  r.str("consensus");
  r.str(p.consensus);
  r.str("core_size");
  r.uint((uint64_t)K);
  r.str("null_nuclt_dist");
  r.nuclt_dist(x->reader.null_dist());
  r.str("null_emission");
  r.f32array(x->null_table.data(), DCP_TABLE_SIZE);
  r.str("bg_nuclt_dist");
  r.nuclt_dist(x->reader.bg_dist());
  r.str("bg_emission");
  r.f32array(x->bg_table.data(), DCP_TABLE_SIZE);
  r.str("nodes");
  r.map((uint32_t)(K + 1) * 3);
  for (int n = 0; n <= K; ++n)
  {
    int const m = n < K ? n : K - 1; // node K repeats node K - 1 (protein_absorb)
    r.str("nuclt_dist");
    r.nuclt_dist(p.nodes[(size_t)m]);
    r.str("trans");
    r.f32array(p.trans.data() + 7 * (size_t)n, 7);
    r.str("emission");
    r.f32array(s.h_out + (size_t)(s.first[i] + m) * DCP_PRESS_TABLE, DCP_TABLE_SIZE);
  }
  r.str("BMk");
  r.f32array(p.BMk.data(), (size_t)K);
  if (r.b.size() > 0xffffffffu) return DCP_ELARGEPROTEIN;
  if (int rc = write_all(x->tmp_fd, r.b.data(), r.b.size())) return rc;
  x->sizes.push_back((uint32_t)r.b.size());
  if (!p.has_ga) x->has_ga = false;
  x->timing[5] += now() - t0;
  x->timing[6] += K;
  x->timing[7] += (double)r.b.size();
  return 0;
}

// database_writer_close (c-core/database_writer.c:144-156): the header, then the records behind it
int finish(dcp_press *x)
{
  double const t0 = now();
  Pack h;
  h.map(2);
  h.str("header");
  h.map(8);
  h.str("magic_number");
  h.uint(0xC6F1); // c-core/magic_number.h:4
  h.str("version");
  h.uint(1); // c-core/database_version.h:4
  h.str("entry_dist");
  h.uint(2); // ENTRY_DIST_OCCUPANCY, c-core/entry_dist.h:6-11
  h.str("epsilon");
  h.f32(x->epsilon);
  h.str("abc");
  h.abc("ACGT", 4); // imm_dna_iupac
  h.str("amino");
  h.abc("ACDEFGHIKLMNPQRSTVWY", 2); // imm_amino_iupac
  h.str("has_ga");
  h.u8(x->has_ga ? 0xc3 : 0xc2);
  h.str("protein_sizes");
  h.array((uint32_t)x->sizes.size());
  for (uint32_t v : x->sizes) h.uint(v);
  h.str("proteins");
  h.array((uint32_t)x->sizes.size());
  if (int rc = write_all(x->db_fd, h.b.data(), h.b.size())) return rc;
  if (lseek(x->tmp_fd, 0, SEEK_SET) != 0) return DCP_EFSEEK;
  std::vector<uint8_t> buf(8 << 20);
  for (;;)
  {
    ssize_t const n = ::read(x->tmp_fd, buf.data(), buf.size());
    if (n < 0 && errno == EINTR) continue;
    if (n < 0) return DCP_EFREAD;
    if (n == 0) break;
    if (int rc = write_all(x->db_fd, buf.data(), (size_t)n)) return rc;
  }
  x->timing[7] += (double)h.b.size();
  x->timing[5] += now() - t0;
  return 0;
}

// closes and removes the temporary file; keep_db = false removes the output too
int release(dcp_press *x, bool keep_db)
{
  int rc = 0;
  if (x->stream) (void)hipStreamSynchronize(x->stream);
  for (Slot &s : x->slots)
  {
    s.release();
    s.profiles.clear();
    s.launched = false;
    s.waited = true;
  }
  if (x->stream) (void)hipStreamDestroy(x->stream);
  x->stream = nullptr;
  if (x->tmp_fd >= 0) ::close(x->tmp_fd);
  if (!x->tmp_path.empty()) unlink(x->tmp_path.c_str());
  if (x->db_fd >= 0 && ::close(x->db_fd) != 0) rc = DCP_EFCLOSE;
  if (!keep_db && x->db_fd >= 0) unlink(x->db_path.c_str());
  x->tmp_fd = x->db_fd = -1;
  x->tmp_path.clear();
  x->reader.close();
  x->feeder.have_pending = false;
  x->state = dcp_press::IDLE;
  return rc;
}

int fail(dcp_press *x, int rc, char const *func, char const *detail = nullptr)
{
  x->state = dcp_press::FAILED;
  return raise(rc, func, detail);
}

} // namespace

extern "C" {

struct dcp_press *dcp_press_new(void) { return new (std::nothrow) dcp_press; }

// press.c: dcp_press_setup -- the translation table and the error rate (entry_dist is always occupancy)
int dcp_press_setup(struct dcp_press *x, int gencode_id, float epsilon)
{
  if (!x) return raise(DCP_EFUNCUSE, __func__);
  if (x->state != dcp_press::IDLE) return raise(DCP_EFUNCUSE, __func__, "a press is open: close it first");
  DcpNucltDist probe;
  float const zero[20] = {};
  if (!dcp_setup_nuclt_dist(gencode_id, zero, probe)) return raise(DCP_EGENCODEID, __func__);
  if (!(epsilon >= 0.0f && epsilon <= 1.0f)) return raise(DCP_EFUNCUSE, __func__, "epsilon must lie in [0, 1]");
  x->gencode = gencode_id;
  x->epsilon = epsilon;
  x->ready = true;
  return 0;
}

int dcp_press_open(struct dcp_press *x, char const *hmm, char const *db)
{
  if (!x || !hmm || !db) return raise(DCP_EFUNCUSE, __func__);
  if (!x->ready) return raise(DCP_EFUNCUSE, __func__, "dcp_press_setup has not succeeded");
  if (x->state != dcp_press::IDLE) return raise(DCP_EFUNCUSE, __func__, "a press is open: close it first");
  // the GPU first: without one nothing is created
  x->device = 0;
  if (char const *d = getenv("DECIPHON_HIP_DEVICE")) x->device = atoi(d);
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || x->device < 0 || x->device >= ndev)
    return raise(DCP_EFUNCUSE, __func__, "no HIP device: press computes its emission tables on the GPU");
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, x->device) != hipSuccess || strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return raise(DCP_EFUNCUSE, __func__, "the HIP device is not a gfx950");
  if (hipSetDevice(x->device) != hipSuccess) return raise(DCP_EFUNCUSE, __func__, "hipSetDevice failed");
  x->feeder.batch_nodes = dcp_press_batch_nodes();

  for (double &t : x->timing) t = 0;
  x->end = false;
  x->has_ga = true;
  x->sizes.clear();
  x->cur = 0;
  x->pos = 0;
  x->db_path = db;
  if (int rc = x->reader.open(hmm, x->gencode)) return raise(rc, __func__, hmm);
  x->count = x->reader.count();
  x->state = dcp_press::OPEN;
  // press.c: the output is created at open; the records go to a temporary file beside it
  x->db_fd = ::open(db, O_WRONLY | O_CREAT | O_TRUNC, 0644);
  if (x->db_fd < 0)
  {
    release(x, false);
    return raise(DCP_EFOPEN, __func__, db);
  }
  std::string tmp = x->db_path + ".XXXXXX";
  x->tmp_fd = mkstemp(&tmp[0]);
  if (x->tmp_fd < 0)
  {
    release(x, false);
    return raise(DCP_EMKSTEMP, __func__, db);
  }
  x->tmp_path = tmp;
  int rc = hipStreamCreateWithFlags(&x->stream, hipStreamNonBlocking) == hipSuccess ? 0 : DCP_EFUNCUSE;
  // the null and background tables are the same for every profile: computed once
  Slot &s = x->slots[0];
  if (!rc) rc = reserve(s, 2);
  if (!rc)
  {
    dcp_press_put_entry(s.h_in, x->reader.null_dist());
    dcp_press_put_entry(s.h_in + DCP_PRESS_IN_STRIDE, x->reader.bg_dist());
    s.entries = 2;
    rc = launch(x, s);
  }
  if (!rc) rc = wait(x, s);
  if (!rc)
  {
    x->null_table.assign(s.h_out, s.h_out + DCP_TABLE_SIZE);
    x->bg_table.assign(s.h_out + DCP_TABLE_SIZE, s.h_out + 2 * DCP_TABLE_SIZE);
    rc = fill(x, s); // the read-ahead of the first batch
  }
  if (rc)
  {
    release(x, false);
    return raise(rc, __func__);
  }
  return 0;
}

long dcp_press_nproteins(struct dcp_press const *x) { return x && x->state != dcp_press::IDLE ? x->count : 0; }

int dcp_press_next(struct dcp_press *x)
{
  if (!x) return raise(DCP_EFUNCUSE, __func__);
  if (x->state == dcp_press::IDLE) return raise(DCP_EFUNCUSE, __func__, "dcp_press_open has not succeeded");
  if (x->state == dcp_press::FAILED) return raise(DCP_EFUNCUSE, __func__, "the press has failed: close it");
  if (x->end) return raise(DCP_EFUNCUSE, __func__, "the press has ended");
  for (;;)
  {
    Slot &s = x->slots[x->cur];
    if (!s.waited)
    {
      // first profile of this batch: read ahead into the other slot (its batch is written), then wait for this one
      if (!s.rc_after && !s.eof_after)
        if (int rc = fill(x, x->slots[x->cur ^ 1])) return fail(x, rc, __func__);
      if (int rc = wait(x, s)) return fail(x, rc, __func__, "the emission kernel failed");
    }
    if (x->pos < s.profiles.size())
    {
      if (int rc = write_protein(x, s, x->pos++)) return fail(x, rc, __func__, x->tmp_path.c_str());
      return 0;
    }
    if (s.rc_after) return fail(x, s.rc_after, __func__);
    if (s.eof_after)
    {
      x->end = true;
      return 0;
    }
    x->cur ^= 1;
    x->pos = 0;
  }
}

bool dcp_press_end(struct dcp_press const *x) { return x && x->state == dcp_press::OPEN && x->end; }

int dcp_press_close(struct dcp_press *x)
{
  if (!x) return raise(DCP_EFUNCUSE, __func__);
  if (x->state == dcp_press::IDLE) return 0;
  if (x->state == dcp_press::FAILED)
  {
    release(x, false); // the error was reported by the call that failed
    return 0;
  }
  // an open press, ended or not: the proteins pressed so far make the database (c-core/press.c:140-152)
  if (x->stream) (void)hipStreamSynchronize(x->stream);
  int rc = finish(x);
  int const rc_close = release(x, rc == 0);
  if (!rc) rc = rc_close;
  if (rc) unlink(x->db_path.c_str());
  return raise(rc, __func__);
}

void dcp_press_del(struct dcp_press const *cx)
{
  dcp_press *x = const_cast<dcp_press *>(cx);
  if (!x) return;
  if (x->state != dcp_press::IDLE) release(x, false);
  delete x;
}

int dcp_press_last_timing(struct dcp_press const *x, double *out, int n)
{
  if (!x || (n > 0 && !out)) return 0;
  for (int i = 0; i < n && i < DCP_PRESS_TIMING_VALUES; ++i) out[i] = x->timing[i];
  return DCP_PRESS_TIMING_VALUES;
}

} // extern "C"
