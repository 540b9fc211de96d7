// product_runs.cpp -- see product_runs.h
#include "product_runs.h"
#include "../../include/deciphon_host.h"
#include "dcp_errors.h"
#include <algorithm>
#include <fcntl.h>
#include <queue>
#include <string.h>
#include <unistd.h>

namespace
{

char const HEADER[] = "sequence\twindow\twindow_start\twindow_stop\thit\thit_start\thit_stop\tprofile\tabc\tlrt\tevalue\tmatch\n";
char const HEADER_STRAND[] = "sequence\twindow\twindow_start\twindow_stop\thit\thit_start\thit_stop\tprofile\tabc\tlrt\tevalue\tmatch\tstrand\n";

// a row of a run file: this, then `len` bytes of text
struct Record
{
  int32_t profile, seq, window, zero;
  int64_t serial;
  uint64_t len;
};

bool before(DcpProductRuns::Row const &a, DcpProductRuns::Row const &b)
{
  if (a.profile != b.profile) return a.profile < b.profile;
  if (a.seq != b.seq) return a.seq < b.seq;
  if (a.window != b.window) return a.window < b.window;
  return a.serial < b.serial;
}

bool put_record(FILE *fp, DcpProductRuns::Row const &r)
{
  Record const rec{r.profile, r.seq, r.window, 0, r.serial, (uint64_t)r.text.size()};
  return fwrite(&rec, sizeof rec, 1, fp) == 1 && fwrite(r.text.data(), 1, r.text.size(), fp) == r.text.size();
}

} // namespace

struct DcpProductRuns::Source
{
  FILE *fp = nullptr;
  std::vector<Row> *mem = nullptr;
  size_t at = 0;
  Row cur;
  // 1: cur is the next row; 0: the end; -1: the run file is cut short
  int next()
  {
    if (mem)
    {
      if (at >= mem->size()) return 0;
      cur = std::move((*mem)[at++]);
      return 1;
    }
    Record rec;
    size_t const got = fread(&rec, 1, sizeof rec, fp);
    if (got == 0 && feof(fp)) return 0;
    if (got != sizeof rec) return -1;
    cur.profile = rec.profile;
    cur.seq = rec.seq;
    cur.window = rec.window;
    cur.serial = rec.serial;
    cur.text.resize((size_t)rec.len);
    return fread(&cur.text[0], 1, cur.text.size(), fp) == cur.text.size() ? 1 : -1;
  }
};

DcpProductRuns::DcpProductRuns(std::string dir, int64_t budget_bytes, bool strand_column)
    : dir_(std::move(dir)), budget_(std::max<int64_t>(budget_bytes, 0)), header_(strand_column ? HEADER_STRAND : HEADER)
{
}

DcpProductRuns::~DcpProductRuns()
{
  remove_runs();
  if (fd_ >= 0) ::close(fd_);
}

void DcpProductRuns::remove_runs()
{
  for (std::string const &f : runs_) unlink(f.c_str());
  runs_.clear();
}

// the first error sticks; what is held goes, and so do the runs
int DcpProductRuns::fail(int rc)
{
  if (!rc_) rc_ = rc;
  std::vector<Row>().swap(held_);
  held_bytes_ = 0;
  remove_runs();
  return rc_;
}

std::string DcpProductRuns::next_run_name()
{
  char name[48];
  snprintf(name, sizeof name, "/.products.%03lld.run", (long long)runs_written_);
  return dir_ + name;
}

int DcpProductRuns::write_run(std::string const &path, std::vector<Row> const &rows)
{
  FILE *fp = fopen(path.c_str(), "wbe");
  if (!fp) return DCP_EOPENTMP;
  runs_.push_back(path);
  ++runs_written_;
  bool ok = true;
  for (Row const &r : rows) ok = ok && put_record(fp, r);
  return fclose(fp) != 0 || !ok ? DCP_EWRITEPROD : 0;
}

int DcpProductRuns::spill()
{
  std::sort(held_.begin(), held_.end(), before);
  int const rc = write_run(next_run_name(), held_);
  if (rc) return fail(rc);
  spilled_ = true;
  std::vector<Row>().swap(held_);
  held_bytes_ = 0;
  return 0;
}

int DcpProductRuns::add(std::vector<Row> &&rows)
{
  std::vector<Row> taken = std::move(rows);
  std::lock_guard<std::mutex> lock(mu_);
  if (closed_) return DCP_EFUNCUSE;
  if (rc_) return rc_;
  rows_ += (int64_t)taken.size();
  held_.reserve(held_.size() + taken.size());
  for (Row &r : taken)
  {
    held_bytes_ += (int64_t)r.text.size();
    held_.push_back(std::move(r));
  }
  peak_bytes_ = std::max(peak_bytes_, held_bytes_);
  return held_bytes_ > budget_ ? spill() : 0;
}

// `runs` and, when given, the sorted rows of `mem`, merged into `out`: as the lines of the product file (final) or as
// the records of another run
int DcpProductRuns::merge(std::vector<std::string> const &runs, std::vector<Row> *mem, FILE *out, bool final)
{
  std::vector<Source> src(runs.size() + (mem ? 1 : 0));
  int rc = 0;
  for (size_t i = 0; i < runs.size() && !rc; ++i)
    if (!(src[i].fp = fopen(runs[i].c_str(), "rbe"))) rc = DCP_EFREAD;
  if (mem) src.back().mem = mem;
  auto later = [&src](size_t a, size_t b) { return before(src[b].cur, src[a].cur); };
  std::priority_queue<size_t, std::vector<size_t>, decltype(later)> heap(later);
  for (size_t i = 0; i < src.size() && !rc; ++i)
  {
    int const got = src[i].next();
    if (got < 0) rc = DCP_EFREAD;
    if (got > 0) heap.push(i);
  }
  while (!rc && !heap.empty())
  {
    size_t const i = heap.top();
    heap.pop();
    Row const &r = src[i].cur;
    if (final)
    {
      offsets_.push_back(file_bytes_);
      if (fwrite(r.text.data(), 1, r.text.size(), out) != r.text.size() || fputc('\n', out) == EOF) rc = DCP_EWRITEPROD;
      file_bytes_ += (int64_t)r.text.size() + 1;
    }
    else if (!put_record(out, r))
      rc = DCP_EWRITEPROD;
    int const got = src[i].next();
    if (got < 0 && !rc) rc = DCP_EFREAD;
    if (got > 0) heap.push(i);
  }
  for (Source &s : src)
    if (s.fp) fclose(s.fp);
  return rc;
}

int DcpProductRuns::close(std::string const &file)
{
  std::lock_guard<std::mutex> lock(mu_);
  if (closed_) return DCP_EFUNCUSE;
  closed_ = true;
  if (rc_) return fail(rc_);
  std::sort(held_.begin(), held_.end(), before);
  if (!spilled_)
  {
    // product_close (c-core/product.c:34-88) of rows that were never on disk; the strings stay for row()
    FILE *fp = fopen(file.c_str(), "wb");
    if (!fp) return fail(DCP_EFOPEN);
    bool ok = fputs(header_, fp) >= 0;
    file_bytes_ = (int64_t)strlen(header_);
    for (Row const &r : held_)
    {
      ok = ok && fwrite(r.text.data(), 1, r.text.size(), fp) == r.text.size() && fputc('\n', fp) != EOF;
      file_bytes_ += (int64_t)r.text.size() + 1;
    }
    if (fclose(fp) != 0 || !ok) return fail(DCP_EWRITEPROD);
    closed_ok_ = true;
    return 0;
  }
  // passes over the oldest runs until what is left, and the rows in memory, can be open at once
  size_t const mem = held_.empty() ? 0 : 1;
  while (runs_.size() + mem > FAN_IN)
  {
    std::vector<std::string> const group(runs_.begin(), runs_.begin() + (long)FAN_IN);
    std::string const name = next_run_name();
    FILE *fp = fopen(name.c_str(), "wbe");
    if (!fp) return fail(DCP_EOPENTMP);
    runs_.push_back(name);
    ++runs_written_;
    int rc = merge(group, nullptr, fp, false);
    if (fclose(fp) != 0 && !rc) rc = DCP_EWRITEPROD;
    if (rc) return fail(rc);
    for (std::string const &f : group) unlink(f.c_str());
    runs_.erase(runs_.begin(), runs_.begin() + (long)FAN_IN);
  }
  FILE *fp = fopen(file.c_str(), "wb");
  if (!fp) return fail(DCP_EFOPEN);
  bool const ok = fputs(header_, fp) >= 0;
  file_bytes_ = (int64_t)strlen(header_);
  offsets_.reserve((size_t)rows_ + 1);
  int rc = merge(runs_, mem ? &held_ : nullptr, fp, true);
  offsets_.push_back(file_bytes_);
  if ((fflush(fp) != 0 || !ok) && !rc) rc = DCP_EWRITEPROD;
  if (fclose(fp) != 0 && !rc) rc = DCP_EWRITEPROD;
  if (rc) return fail(rc);
  std::vector<Row>().swap(held_);
  held_bytes_ = 0;
  remove_runs();
  if ((fd_ = open(file.c_str(), O_RDONLY | O_CLOEXEC)) < 0) return fail(DCP_EFOPEN);
  closed_ok_ = true;
  return 0;
}

char const *DcpProductRuns::row(long i)
{
  if (!closed_ok_ || i < 0 || i >= (long)rows_) return nullptr;
  if (!spilled_) return held_[(size_t)i].text.c_str();
  int64_t const at = offsets_[(size_t)i];
  buf_.resize((size_t)(offsets_[(size_t)i + 1] - at - 1)); // (without the newline)
  for (size_t done = 0; done < buf_.size();)
  {
    ssize_t const got = pread(fd_, &buf_[done], buf_.size() - done, (off_t)(at + (int64_t)done));
    if (got <= 0) return nullptr;
    done += (size_t)got;
  }
  return buf_.c_str();
}

void DcpProductRuns::stats(int64_t out[4]) const
{
  std::lock_guard<std::mutex> lock(mu_);
  out[0] = rows_;
  out[1] = runs_written_;
  out[2] = peak_bytes_;
  out[3] = file_bytes_;
}

// ---- the C ABI of include/deciphon_host.h (here, not in host_capi.cpp: that file is also built without this one)

struct dcp_product_runs
{
  DcpProductRuns runs;
  int64_t added = 0; // the serial of the next row: rows in call order
};

extern "C" {

struct dcp_product_runs *dcp_product_runs_new(char const *dir, int64_t budget_bytes)
{
  if (!dir) return nullptr;
  return new dcp_product_runs{{dir, budget_bytes}};
}

void dcp_product_runs_del(struct dcp_product_runs *x) { delete x; }

int dcp_product_runs_add(struct dcp_product_runs *x, int n, int32_t const *profile, int32_t const *seq,
                         int32_t const *window, char const *const *text)
{
  if (!x || n < 0 || (n && (!profile || !seq || !window || !text))) return DCP_EFUNCUSE;
  std::vector<DcpProductRuns::Row> rows((size_t)n);
  for (int i = 0; i < n; ++i)
  {
    if (!text[i]) return DCP_EFUNCUSE;
    rows[(size_t)i] = DcpProductRuns::Row{profile[i], seq[i], window[i], x->added + i, text[i]};
  }
  x->added += n;
  return x->runs.add(std::move(rows));
}

int dcp_product_runs_close(struct dcp_product_runs *x, char const *file)
{
  return x && file ? x->runs.close(file) : DCP_EFUNCUSE;
}

long dcp_product_runs_num_rows(struct dcp_product_runs const *x) { return x ? x->runs.num_rows() : 0; }
char const *dcp_product_runs_row(struct dcp_product_runs *x, long i) { return x ? x->runs.row(i) : nullptr; }

int dcp_product_runs_stats(struct dcp_product_runs const *x, int64_t out[4])
{
  if (x && out) x->runs.stats(out);
  return 4;
}

} // extern "C"
