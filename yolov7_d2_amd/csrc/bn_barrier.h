// The word protocol of the grid-wide barrier of the one-launch BatchNorm backward (bn_act.hip), as plain functions over an
// atomics policy A, so that the SAME text runs in the kernel (BnbHip, conv_bn.h: relaxed agent-scope HIP atomics) and on the
// host (tests/native/bn_barrier_host.cpp: std::atomic, one std::thread per block) - a wrong arrival tree hangs a GPU, so it
// is run on the CPU first.  No HIP, no headers: a policy provides
//   static unsigned fetch_add(unsigned* p, unsigned v)   returning add
//   static void add(unsigned* p, unsigned v)             add whose result nobody waits for
//   static unsigned load(const unsigned* p)
//   static void store(unsigned* p, unsigned v)
//   static void pause()                                   between two polls
// Word layout (uint32; every counter on its own 256-byte line), BNB_WORDS words in all:
//   [0] top arrivals  [2] give-up flag  [64 * (1 + g)] generation of group g  [64 * (1 + G + g)] arrivals of group g
// Arrivals go through a two-level tree: block b counts on group b % G, G = min(nb, BNB_G); the last of a group counts on the
// top word; whoever is last there has seen every block arrive.  Each counter is put back to zero by the one who saw it
// full, so a record needs no reset between launches; the generation words only ever grow (by one per launch that uses them).
#pragma once
#ifdef __HIPCC__
#define BNB_FN __device__ __forceinline__
#else
#define BNB_FN inline
#endif
#define BNB_G 16
#define BNB_WORDS (64 * (1 + 2 * BNB_G))
#define BNB_FLAG 2

BNB_FN int bnb_groups(const int nb) { return nb < BNB_G ? nb : BNB_G; }
BNB_FN int bnb_group(const int bid, const int nb) { return bid % bnb_groups(nb); }
BNB_FN unsigned* bnb_gen(unsigned* bar, const int g) { return bar + 64 * (1 + g); }
BNB_FN unsigned* bnb_cnt(unsigned* bar, const int g) { return bar + 64 * (1 + BNB_G + g); }

// the generation this block will wait to see change: read BEFORE the block arrives
template <class A>
BNB_FN unsigned bnb_generation(unsigned* bar, const int bid, const int nb) {
  return A::load(bnb_gen(bar, bnb_group(bid, nb)));
}
// count this block's arrival; true for the block that arrives last of all (it has reset the counters for the next launch)
template <class A>
BNB_FN bool bnb_arrive(unsigned* bar, const int bid, const int nb) {
  const int G = bnb_groups(nb);
  const int g = bid % G;
  const unsigned gsize = (unsigned)((nb - g + G - 1) / G);
  if (A::fetch_add(bnb_cnt(bar, g), 1u) == gsize - 1u) {
    A::store(bnb_cnt(bar, g), 0u);
    if (A::fetch_add(bar, 1u) == (unsigned)G - 1u) {
      A::store(bar, 0u);
      return true;
    }
  }
  return false;
}
// the last block lets group q go, q < bnb_groups(nb): one call per group - in the kernel one LANE per group, so that the G
// bumps leave in one instruction (a loop of them in one lane took 0.9 us: profiles/bn_bwd_chain_ab.txt)
template <class A>
BNB_FN void bnb_release_group(unsigned* bar, const int q) {
  A::add(bnb_gen(bar, q), 1u);
}
// wait until the generation of this block's group has moved on from gen0; true when the wait gave up after `limit` polls
// (a block that never became resident: report in the flag word instead of hanging the GPU)
template <class A>
BNB_FN bool bnb_wait(unsigned* bar, const unsigned gen0, const int bid, const int nb, const int limit) {
  int spins = 0;
  while (A::load(bnb_gen(bar, bnb_group(bid, nb))) == gen0) {
    A::pause();
    if (++spins > limit) {
      A::store(bar + BNB_FLAG, 1u);
      return true;
    }
  }
  return false;
}
