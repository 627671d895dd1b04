// Host-only stress of CopyPool (ffddp_copy_pool.hpp): no HIP, no GPU.
//   make copy_pool_stress   plain build
//   make copy_pool_tsan     the same under ThreadSanitizer
// usage: copy_pool_stress [rounds]   (back-to-back rounds of the first case, default 20000)
// Exits non-zero on any wrong destination byte.
#include <cstdio>

#include "ffddp_copy_pool.hpp"

namespace {
constexpr size_t MiB = size_t(1) << 20;
int g_bad = 0;

std::vector<unsigned char> pattern(size_t n, unsigned seed) {
  std::vector<unsigned char> v(n);
  unsigned s = seed * 2654435761u + 1u;
  for (size_t i = 0; i < n; ++i) {
    s = s * 1664525u + 1013904223u;
    v[i] = (unsigned char)(s >> 24);
  }
  return v;
}

// dst[0, n) equals src[0, n) (src == nullptr: all zero)
void expect(const char* what, const unsigned char* dst, const unsigned char* src, size_t n) {
  for (size_t i = 0; i < n; ++i)
    if (dst[i] != (src ? src[i] : 0)) {
      std::fprintf(stderr, "FAIL %s: byte %zu of %zu is %u\n", what, i, n, dst[i]);
      ++g_bad;
      return;
    }
}

// 16 threads, one 4 MiB job (four pieces: the smallest that wakes the workers),
// back to back with no check in between; the source alternates, so a piece
// copied late on behalf of an earlier run leaves the other source's bytes
void back_to_back(int rounds) {
  const std::vector<unsigned char> a = pattern(4 * MiB, 1), b = pattern(4 * MiB, 2);
  std::vector<unsigned char> dst(4 * MiB);
  CopyPool pool(16);
  for (int r = 0; r < rounds; ++r) pool.run({CopyJob{dst.data(), (r & 1 ? b : a).data(), 4 * MiB}});
  expect("back to back", dst.data(), ((rounds - 1) & 1 ? b : a).data(), 4 * MiB);
}

// several uneven jobs per run(), no size a multiple of 1 MiB, one a zero-fill
void uneven(int nthreads, int rounds) {
  const size_t n[5] = {3 * MiB + 17, MiB - 1, 5, 2 * MiB + 4093, 2 * MiB + MiB / 2 + 1};
  std::vector<unsigned char> dst[5];
  for (int i = 0; i < 5; ++i) dst[i].resize(n[i] + 64);  // 64 guard bytes behind each
  CopyPool pool(nthreads);
  for (int r = 0; r < rounds; ++r) {
    std::vector<std::vector<unsigned char>> src;
    std::vector<CopyJob> jobs;
    for (int i = 0; i < 5; ++i) {
      src.push_back(pattern(n[i], 100u * r + i));
      std::fill(dst[i].begin(), dst[i].end(), (unsigned char)0xA5);
      jobs.push_back(CopyJob{dst[i].data(), i == 2 ? nullptr : src[i].data(), n[i]});
    }
    pool.run(jobs);
    const std::vector<unsigned char> guard(64, 0xA5);
    for (int i = 0; i < 5; ++i) {
      expect("uneven", dst[i].data(), i == 2 ? nullptr : src[i].data(), n[i]);
      expect("uneven guard", dst[i].data() + n[i], guard.data(), 64);
    }
  }
}

// a total just below 4 MiB: the calling thread alone
void below_threshold() {
  const std::vector<unsigned char> a = pattern(3 * MiB, 3), b = pattern(MiB - 1, 4);
  std::vector<unsigned char> da(3 * MiB), db(MiB - 1, 0xFF);
  CopyPool pool(16);
  for (int r = 0; r < 50; ++r) {
    std::fill(da.begin(), da.end(), (unsigned char)r);
    pool.run({CopyJob{da.data(), a.data(), a.size()}, CopyJob{db.data(), b.data(), b.size()}});
    expect("below threshold a", da.data(), a.data(), a.size());
    expect("below threshold b", db.data(), b.data(), b.size());
  }
}

void lifetimes() {
  {
    CopyPool pool(16);  // constructed and destroyed without a run()
  }
  {
    CopyPool pool(16);
    pool.run({});  // no jobs
    unsigned char c = 7;
    pool.run({CopyJob{&c, nullptr, 0}});  // no bytes
    if (c != 7) ++g_bad;
  }
  const std::vector<unsigned char> a = pattern(6 * MiB + 3, 5);
  for (int r = 0; r < 200; ++r) {  // destroyed right after a run()
    std::vector<unsigned char> dst(a.size());
    {
      CopyPool pool(16);
      pool.run({CopyJob{dst.data(), a.data(), a.size()}});
    }
    expect("destroyed after run", dst.data(), a.data(), a.size());
  }
}
}  // namespace

int main(int argc, char** argv) {
  const int rounds = argc > 1 ? std::atoi(argv[1]) : 20000;
  if (rounds < 1) {
    std::fprintf(stderr, "usage: %s [rounds >= 1]\n", argv[0]);
    return 2;
  }
  back_to_back(rounds);
  uneven(16, std::max(rounds / 100, 20));
  uneven(1, 5);  // a pool of one thread: the caller does everything
  below_threshold();
  lifetimes();
  if (CopyPool(1).threads() != 1 || copy_threads() < 1) ++g_bad;
  std::printf("copy_pool_stress: %d back-to-back rounds, %s\n", rounds, g_bad ? "FAILED" : "ok");
  return g_bad ? 1 : 0;
}
