// The grid barrier of the one-launch BatchNorm backward (yolov7_d2_amd/csrc/bn_barrier.h) on the CPU: the same header the
// kernel instantiates with HIP atomics, here over std::atomic_ref with one std::thread per block.
//   g++ -std=c++20 -O2 -pthread [-fsanitize=thread] tests/native/bn_barrier_host.cpp   (tests/test_bn_barrier_host.py)
// For every block count in {1, 2, 15, 16, 17, 33, 257, 512}: 64 launches on ONE record, never re-zeroed.  A launch is what the
// kernel does around the barrier: read the generation, add to the sums, arrive; the block that arrives last folds the sums into
// a plain total and lets every group go (one call per group, as the kernel's lanes do); the others wait, then read the total.
// Checked: exactly one block per launch is last; the total every block reads is complete (so nobody was released early and
// the last block had seen every arrival); every thread saw every launch's release exactly once, its generation word moved by
// exactly one; no wait gave up; after the 64 launches the record is what tests/bn_ref.py::barrier_expected states - every
// word zero except the generation of group g < min(nb, 16), which equals 64 - and the guard words around it are untouched.
// The kernel orders its payload around the relaxed words by waiting for acknowledgements (s_waitcnt vmcnt(0)); the host
// policy stands for that with acquire / release on the same words, which is also what lets -fsanitize=thread vouch for the
// plain total.  Launches are separated by a std::barrier, as kernel boundaries separate them on the device.
#include <atomic>
#include <barrier>
#include <cstdio>
#include <thread>
#include <vector>
#include "../../yolov7_d2_amd/csrc/bn_barrier.h"

struct BnbStd {
  static unsigned fetch_add(unsigned* p, unsigned v) { return std::atomic_ref<unsigned>(*p).fetch_add(v, std::memory_order_acq_rel); }
  static void add(unsigned* p, unsigned v) { (void)std::atomic_ref<unsigned>(*p).fetch_add(v, std::memory_order_release); }
  static unsigned load(const unsigned* p) { return std::atomic_ref<unsigned>(*const_cast<unsigned*>(p)).load(std::memory_order_acquire); }
  static void store(unsigned* p, unsigned v) { std::atomic_ref<unsigned>(*p).store(v, std::memory_order_release); }
  static void pause() { std::this_thread::yield(); }
};

static const int LAUNCHES = 64, GUARD = 64, SPIN_LIMIT = 1 << 30;
static const unsigned SENT = 0xA5A5A5A5u;

static int run(const int nb) {
  alignas(256) static unsigned rec[GUARD + BNB_WORDS + GUARD];
  for (int i = 0; i < GUARD + BNB_WORDS + GUARD; ++i) rec[i] = (i < GUARD || i >= GUARD + BNB_WORDS) ? SENT : 0u;
  unsigned* bar = rec + GUARD;
  unsigned long long sum = 0;          // the accumulators: atomic adds before the arrival
  unsigned long long total = 0;        // the folded total: plain, written by the last block, read by everybody behind the barrier
  std::atomic<int> lasts{0}, errors{0};
  std::vector<int> seen(nb, 0);
  std::barrier<> boundary(nb);
  auto block = [&](const int bid) {
    for (int l = 0; l < LAUNCHES; ++l) {
      const unsigned gen0 = bnb_generation<BnbStd>(bar, bid, nb);
      std::atomic_ref<unsigned long long>(sum).fetch_add((unsigned long long)(bid + 1) * (l + 1), std::memory_order_relaxed);
      if (bnb_arrive<BnbStd>(bar, bid, nb)) {
        lasts.fetch_add(1, std::memory_order_relaxed);
        total = std::atomic_ref<unsigned long long>(sum).exchange(0, std::memory_order_relaxed);
        for (int q = 0; q < bnb_groups(nb); ++q) bnb_release_group<BnbStd>(bar, q);
      } else if (bnb_wait<BnbStd>(bar, gen0, bid, nb, SPIN_LIMIT)) {
        errors.fetch_add(1, std::memory_order_relaxed);
      }
      if (total != (unsigned long long)nb * (nb + 1) / 2 * (l + 1)) errors.fetch_add(1, std::memory_order_relaxed);
      if (BnbStd::load(bnb_gen(bar, bnb_group(bid, nb))) == gen0 + 1u) seen[bid] += 1;
      boundary.arrive_and_wait();      // the launch ends: the next one begins when every block is done
    }
  };
  std::vector<std::thread> th;
  for (int b = 0; b < nb; ++b) th.emplace_back(block, b);
  for (auto& t : th) t.join();
  int bad = errors.load();
  if (lasts.load() != LAUNCHES) { printf("nb %d: %d last arrivers in %d launches\n", nb, lasts.load(), LAUNCHES); ++bad; }
  for (int b = 0; b < nb; ++b)
    if (seen[b] != LAUNCHES) { printf("nb %d: block %d saw %d releases\n", nb, b, seen[b]); ++bad; break; }
  for (int i = 0; i < GUARD + BNB_WORDS + GUARD; ++i) {
    unsigned exp = SENT;
    if (i >= GUARD && i < GUARD + BNB_WORDS) {
      const int w = i - GUARD;
      exp = 0u;
      for (int g = 0; g < (nb < BNB_G ? nb : BNB_G); ++g)
        if (w == 64 * (1 + g)) exp = (unsigned)LAUNCHES;
    }
    if (rec[i] != exp) { printf("nb %d: word %d is %u, expected %u\n", nb, i - GUARD, rec[i], exp); ++bad; break; }
  }
  printf("nb %3d: %s\n", nb, bad ? "FAILED" : "ok");
  return bad;
}

int main() {
  int bad = 0;
  for (int nb : {1, 2, 15, 16, 17, 33, 257, 512}) bad += run(nb);
  return bad ? 1 : 0;
}
