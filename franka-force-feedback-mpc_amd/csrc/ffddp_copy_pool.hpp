// Host memcpy / zero-fill pool of the host entry point: persistent threads
// (FFDDP_COPY_THREADS, default the CPUs this process may use, at most 16)
// that split a list of jobs into 1 MiB pieces with the calling thread.
// Standard library and <sched.h> only, so it compiles without HIP
// (copy_pool_stress.cpp; make copy_pool_stress / copy_pool_tsan).
#pragma once

#include <sched.h>

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <thread>
#include <vector>

struct CopyJob {
  void* dst;
  const void* src;  // nullptr: zero-fill dst (first touch of fresh output pages)
  size_t n;
};
class CopyPool {
 public:
  explicit CopyPool(int nthreads) {
    // no exception may cross the C ABI: with fewer threads than asked (or
    // none) the calling thread does the rest of the copies
    try {
      for (int i = 1; i < nthreads; ++i) th_.emplace_back([this] { worker(); });
    } catch (...) {
    }
  }
  ~CopyPool() {
    {
      std::lock_guard<std::mutex> lk(mu_);
      stop_ = true;
    }
    cv_.notify_all();
    for (std::thread& t : th_) t.join();
  }
  int threads() const { return (int)th_.size() + 1; }
  void run(const std::vector<CopyJob>& jobs) {
    constexpr size_t kPiece = size_t(1) << 20;
    std::vector<CopyJob> pieces;
    size_t tot = 0;
    for (const CopyJob& j : jobs) {
      for (size_t o = 0; o < j.n; o += kPiece)
        pieces.push_back(CopyJob{(char*)j.dst + o, j.src ? (const char*)j.src + o : nullptr, std::min(kPiece, j.n - o)});
      tot += j.n;
    }
    if (pieces.empty()) return;
    if (th_.empty() || tot < 4 * kPiece) {  // small: the calling thread alone
      for (const CopyJob& c : pieces) exec(c);
      return;
    }
    {
      std::lock_guard<std::mutex> lk(mu_);
      work_ = &pieces;
      next_.store(0);
      left_ = pieces.size();
      ++gen_;
    }
    cv_.notify_all();
    const size_t did = drain(&pieces);
    // `pieces` dies with this call: every piece done, and no worker left that
    // took work_ for this run (one still inside drain() reads its size)
    std::unique_lock<std::mutex> lk(mu_);
    left_ -= did;
    done_cv_.wait(lk, [&] { return left_ == 0 && active_ == 0; });
    work_ = nullptr;
  }

 private:
  static void exec(const CopyJob& c) {
    if (c.src)
      std::memcpy(c.dst, c.src, c.n);
    else
      std::memset(c.dst, 0, c.n);
  }
  // the pieces are handed out through next_, the one member shared without mu_
  size_t drain(const std::vector<CopyJob>* w) {
    size_t did = 0;
    for (size_t i = next_++; i < w->size(); i = next_++) {
      exec((*w)[i]);
      ++did;
    }
    return did;
  }
  void worker() {
    uint64_t seen = 0;
    std::unique_lock<std::mutex> lk(mu_);
    for (;;) {
      cv_.wait(lk, [&] { return stop_ || (gen_ != seen && work_ != nullptr); });
      if (stop_) return;
      seen = gen_;
      const std::vector<CopyJob>* w = work_;
      ++active_;
      lk.unlock();
      const size_t did = drain(w);
      lk.lock();
      left_ -= did;
      if (--active_ == 0 && left_ == 0) done_cv_.notify_all();
    }
  }
  std::vector<std::thread> th_;
  std::mutex mu_;
  std::condition_variable cv_, done_cv_;
  const std::vector<CopyJob>* work_ = nullptr;  // under mu_, like left_, active_, gen_ and stop_
  std::atomic<size_t> next_{0};
  size_t left_ = 0;
  int active_ = 0;
  uint64_t gen_ = 0;
  bool stop_ = false;
};

// the host-copy pool's size: FFDDP_COPY_THREADS, else the CPUs this process
// may run on (the GPU box grants 16 per GPU), at most 16
inline int copy_threads() {
  if (const char* e = std::getenv("FFDDP_COPY_THREADS")) {
    const int v = std::atoi(e);
    return v < 1 ? 1 : (v > 64 ? 64 : v);
  }
  cpu_set_t cs;
  int n = 8;
  if (sched_getaffinity(0, sizeof(cs), &cs) == 0) n = CPU_COUNT(&cs);
  return n < 1 ? 1 : (n > 16 ? 16 : n);
}
