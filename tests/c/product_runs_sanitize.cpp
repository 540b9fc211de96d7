// product_runs_sanitize.cpp -- TEST INFRASTRUCTURE: csrc/product_runs.cpp under ASan + UBSan.  A few hundred rows go in
// from two threads at budgets of 0 (every add a run: more runs than the merge opens at once) and 64 KB; the file and
// every row() are compared with a stable sort of the same rows; then an object that has spilled is destroyed without
// close, and the directory (argv[1], empty) must be empty again.
#include "product_runs.h"
#include <algorithm>
#include <dirent.h>
#include <stdio.h>
#include <string.h>
#include <string>
#include <thread>
#include <unistd.h>
#include <vector>

typedef DcpProductRuns::Row Row;

static uint32_t lcg(uint32_t &s) { return (s = s * 1664525u + 1013904223u) >> 8; }

static std::vector<Row> make_rows(int n)
{
  std::vector<Row> rows;
  uint32_t s = 12345;
  for (int i = 0; i < n; ++i)
  {
    Row r{(int32_t)(lcg(s) % 4), (int32_t)(lcg(s) % 5), (int32_t)(lcg(s) % 6), i, std::string()};
    size_t const len = i % 97 == 0 ? 70000 : lcg(s) % 3000; // (the first one is long, and some are empty)
    for (size_t k = 0; k < len; ++k) r.text += "ACGT,;\tMx"[lcg(s) % 9];
    rows.push_back(std::move(r));
  }
  return rows;
}

static int entries(char const *dir)
{
  int n = 0;
  DIR *d = opendir(dir);
  if (!d) return -1;
  while (struct dirent *e = readdir(d))
    if (strcmp(e->d_name, ".") && strcmp(e->d_name, "..")) ++n;
  closedir(d);
  return n;
}

// the rows in adds of 1..4, even adds from one thread and odd ones from another (serials say which came first)
static int add_all(DcpProductRuns &runs, std::vector<Row> const &rows)
{
  std::vector<std::vector<Row>> adds;
  for (size_t i = 0; i < rows.size();)
  {
    size_t const n = std::min(rows.size() - i, (size_t)1 + i % 4);
    adds.emplace_back(rows.begin() + (long)i, rows.begin() + (long)(i + n));
    i += n;
  }
  int rc[2] = {0, 0};
  auto work = [&](int t) {
    for (size_t a = (size_t)t; a < adds.size(); a += 2)
      if (int const r = runs.add(std::move(adds[a]))) rc[t] = r;
  };
  std::thread other(work, 1);
  work(0);
  other.join();
  return rc[0] ? rc[0] : rc[1];
}

int main(int argc, char **argv)
{
  if (argc < 2) return 2;
  char const *dir = argv[1];
  std::string const file = std::string(dir) + "/products.tsv";
  std::vector<Row> const rows = make_rows(300);
  std::vector<Row> want = rows;
  std::stable_sort(want.begin(), want.end(), [](Row const &a, Row const &b) {
    if (a.profile != b.profile) return a.profile < b.profile;
    if (a.seq != b.seq) return a.seq < b.seq;
    return a.window < b.window;
  });
  int64_t const budgets[2] = {0, 65536};
  for (int64_t budget : budgets)
  {
    DcpProductRuns runs(dir, budget);
    if (int const rc = add_all(runs, rows)) { printf("add rc %d\n", rc); return 1; }
    if (int const rc = runs.close(file)) { printf("close rc %d\n", rc); return 1; }
    int64_t st[4];
    runs.stats(st);
    printf("budget %lld: %lld rows, %lld runs, peak %lld, file %lld bytes\n", (long long)budget, (long long)st[0],
           (long long)st[1], (long long)st[2], (long long)st[3]);
    if (runs.num_rows() != (long)want.size() || st[1] < 2 || entries(dir) != 1) { printf("counts\n"); return 1; }
    if (budget == 0 && st[1] <= (int64_t)DcpProductRuns::FAN_IN) { printf("no merge pass\n"); return 1; }
    std::string text;
    FILE *fp = fopen(file.c_str(), "rb");
    char buf[65536];
    for (size_t n; fp && (n = fread(buf, 1, sizeof buf, fp)) > 0;) text.append(buf, n);
    if (fp) fclose(fp);
    size_t at = text.find('\n') + 1; // (behind the header)
    for (size_t i = 0; i < want.size(); ++i)
    {
      char const *r = runs.row((long)(want.size() - 1 - i));
      if (!r || want[want.size() - 1 - i].text != r) { printf("row %zu\n", want.size() - 1 - i); return 1; }
      if (text.compare(at, want[i].text.size() + 1, want[i].text + "\n") != 0) { printf("line %zu\n", i); return 1; }
      at += want[i].text.size() + 1;
    }
    if (at != text.size() || (int64_t)at != st[3] || runs.row(-1) || runs.row((long)want.size())) { printf("ends\n"); return 1; }
    unlink(file.c_str());
    if (!runs.row(0) || want[0].text != runs.row(0)) { printf("row 0 of the unlinked file\n"); return 1; }
  }
  {
    DcpProductRuns runs(dir, 1000);
    if (int const rc = add_all(runs, rows)) { printf("add rc %d\n", rc); return 1; }
    if (entries(dir) < 2) { printf("nothing spilled\n"); return 1; }
  }
  if (entries(dir) != 0) { printf("run files left behind\n"); return 1; }
  printf("product runs done\n");
  return 0;
}
