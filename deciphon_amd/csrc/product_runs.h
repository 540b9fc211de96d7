// product_runs.h -- the product rows of a scan, from the order of work to the reference's order, in bounded memory.
//
// The reference never holds its rows: every thread appends to a hidden file of its own in the product directory and
// product_close concatenates those (c-core/product.c:63-81).  Here rows arrive in the order of the path passes, so
// they are sorted: in memory while their text stays within a budget, and through sorted run files
// (<dir>/.products.NNN.run, named like c-core/product.c:66 names its parts) beyond it.  Host only: no engine, no HIP.
//
// A row is {profile, seq, window, serial, text}; the order is (profile, seq, window, serial), serial being the
// arrival number its caller gives -- what a stable sort by (profile, seq, window) of the rows in arrival order makes.
//
// add() counts the text bytes it holds; once they exceed the budget, the rows held are sorted, written as one run and
// dropped, on the calling thread.  After add() returns at most `budget` bytes are held, so the most ever held
// (peak_bytes) is the budget plus the text of the largest single add().  close() without a run sorts, writes and
// keeps the strings; with runs it merges them and the remainder by a heap straight into the file, at most FAN_IN runs
// open at a time (more are merged in passes into intermediate runs), holding one row of each open run beside what
// add() held.  No call leaves a run file behind, and neither does destruction at any point.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <mutex>
#include <string>
#include <vector>

class DcpProductRuns
{
public:
  static constexpr size_t FAN_IN = 64; // runs open at a time: a process has about 1024 descriptors

  struct Row
  {
    int32_t profile, seq, window;
    int64_t serial;
    std::string text;
  };

  // strand_column: the header names a 13th column, `strand` (the rows of a scan of both strands end in it)
  DcpProductRuns(std::string dir, int64_t budget_bytes, bool strand_column = false);
  ~DcpProductRuns();
  DcpProductRuns(DcpProductRuns const &) = delete;
  DcpProductRuns &operator=(DcpProductRuns const &) = delete;

  // Thread-safe.  0, or the first error of this object: DCP_EOPENTMP when a run file cannot be created,
  // DCP_EWRITEPROD when it cannot be written.  The rows are taken (moved from) either way.
  int add(std::vector<Row> &&rows);
  // Header and rows to `file` (DCP_EFOPEN when it cannot be opened, DCP_EWRITEPROD when it cannot be written), or the
  // first error of an add(); the run files are gone afterwards either way.  Once.
  int close(std::string const &file);
  // rows written by close()
  long num_rows() const { return closed_ok_ ? (long)rows_ : 0; }
  // Row i without its newline, or nullptr.  Without a run: the stored string.  With runs: read from `file` through a
  // descriptor kept open (the file may be unlinked meanwhile) into a buffer of this object, which stands until the
  // next row(), and is then not to be called from two threads at once.
  char const *row(long i);
  // rows added, runs written (intermediate ones included), most text bytes held by add(), bytes written to `file`
  void stats(int64_t out[4]) const;

private:
  struct Source; // of the merge: a run file or the rows in memory
  int fail(int rc);
  int spill();                                                        // held_ -> a new run
  int write_run(std::string const &path, std::vector<Row> const &rows);
  int merge(std::vector<std::string> const &runs, std::vector<Row> *mem, FILE *out, bool final);
  std::string next_run_name();
  void remove_runs();

  std::string dir_;
  int64_t budget_;
  char const *header_;
  mutable std::mutex mu_;
  std::vector<Row> held_;
  int64_t held_bytes_ = 0, peak_bytes_ = 0, rows_ = 0, runs_written_ = 0, file_bytes_ = 0;
  int rc_ = 0;
  bool closed_ = false, closed_ok_ = false, spilled_ = false;
  std::vector<std::string> runs_;   // files that exist
  std::vector<int64_t> offsets_;    // of a spilled close: where row i starts in `file`; rows_ + 1 of them
  int fd_ = -1;                     // of `file`, read-only, after a spilled close
  std::string buf_;                 // of row()
};
