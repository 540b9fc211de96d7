// parallel_for.h -- the one pool of plain host threads, joined before it returns (no runtime is left spinning next
// to the HIP callbacks).
#pragma once
#include <algorithm>
#include <atomic>
#include <stddef.h>
#include <thread>
#include <vector>

// fn(i) for every i in [0, n), on min(hardware_concurrency(), max_threads, max(n / grain, 1)) threads, the calling one
// among them; the indices are handed out `step` at a time.  Every thread calls a copy of fn of its own: what fn
// captures by value is that thread's scratch.
template <class F> void dcp_parallel_for(size_t n, unsigned max_threads, size_t grain, size_t step, F fn)
{
  std::atomic<size_t> next{0};
  auto work = [&next, n, step](F f) {
    for (size_t b = next.fetch_add(step); b < n; b = next.fetch_add(step))
      for (size_t i = b, e = std::min(n, b + step); i < e; ++i) f(i);
  };
  unsigned const nthreads = std::min<unsigned>(
      {std::max(1u, std::thread::hardware_concurrency()), max_threads, (unsigned)std::max<size_t>(n / grain, 1)});
  std::vector<std::thread> pool;
  for (unsigned t = 1; t < nthreads; ++t) pool.emplace_back(work, fn);
  work(fn);
  for (std::thread &t : pool) t.join();
}
