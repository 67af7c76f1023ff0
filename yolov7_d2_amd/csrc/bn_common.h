// The pieces every train-mode BatchNorm kernel shares, in ONE copy: bn_act.hip (BatchNorm + SiLU), bn_relu.hip (BatchNorm +
// ReLU) and, through conv_bn.h, the two persistent convolution kernels.  The exact tests hold all of them to the same bits, so
// the arithmetic below is written once: fp64 slot accumulators -> mean / clamped variance / invstd -> fp32 scale / shift, the
// record for the backward pass and the running statistics (nn.BatchNorm2d: momentum, unbiased running variance,
// num_batches_tracked), the backward prologue, and the block reduction of channel sums into a slot.
#pragma once
#include "common.h"

#define BN_MAXC 2048
#ifndef BN_TL   // diagnostic build of bn_act.hip (MI_BN_CHAIN_TIMELINE) only
#define BN_TL(k) do { } while (0)
#endif
// accumulator layout: [slot][CA][2] with CA = C rounded up to 32 - the CoutPad the conv epilogue adds its tile sums with
#define BN_ACC_C(C) (((C) + 31) / 32 * 32)
// every tensor access is a 16-byte vector: NULL (an absent optional tensor) passes
static inline bool bn_al16(const void* p) { return ((uintptr_t)p % 16) == 0; }
// nslots outside 1 .. MI_BN_SLOTS means MI_BN_SLOTS
static inline int bn_slots(int nslots) { return (nslots >= 1 && nslots <= MI_BN_SLOTS) ? nslots : MI_BN_SLOTS; }

// ---- forward statistics
struct BnMoments {
  double mean, var, invstd;
};
// folded sums (s1, s2) of one channel -> its moments and (scale, shift).  HOW the slots are loaded and folded stays with
// the caller: that part is measured and differs on purpose (bn_slot_sums below, bnx_tables in conv_bn.h)
__device__ __forceinline__ BnMoments bn_moments(const double s1, const double s2, const double inv_count, const float eps,
                                                const float g, const float b, float& sc, float& sh) {
  BnMoments m;
  m.mean = s1 * inv_count;
  m.var = s2 * inv_count - m.mean * m.mean;
  if (m.var < 0.0) m.var = 0.0;
  m.invstd = 1.0 / sqrt(m.var + (double)eps);
  sc = (float)((double)g * m.invstd);
  sh = (float)((double)b - m.mean * (double)g * m.invstd);
  return m;
}
// `poison` of bn_record where no barrier can time out: x + -0.f is x for every x (x + 0.f would turn -0 into +0)
#define BN_NO_POISON (-0.f)
// one lane per channel of the launch: record scale / shift / mean / invstd for the backward pass and update the running
// statistics.  p: any record with scale, shift, mean, invstd, rmean, rvar, nbt, momentum, unbias.  sc / sh as the caller
// uses them (already poisoned where it poisons); `poison` (NaN after a barrier timeout) also marks mean / invstd.
// PAIRED: running_mean and running_var come together or not at all, rmean is the one tested (mi_bn_act_fwd, the conv
// kernels); otherwise each may be NULL on its own (mi_bn_relu_norm)
template <bool PAIRED, class P>
__device__ __forceinline__ void bn_record(P& p, const int c, const float sc, const float sh, const BnMoments& m, const float poison) {
  const bool has_rmean = p.rmean != nullptr, has_rvar = PAIRED ? has_rmean : p.rvar != nullptr;
  p.scale[c] = sc;
  p.shift[c] = sh;
  p.mean[c] = (float)m.mean + poison;
  p.invstd[c] = (float)m.invstd + poison;
  if (has_rmean) p.rmean[c] = (1.f - p.momentum) * p.rmean[c] + p.momentum * (float)m.mean;
  if (has_rvar) p.rvar[c] = (1.f - p.momentum) * p.rvar[c] + p.momentum * (float)(m.var * p.unbias);
  if (c == 0 && p.nbt) *p.nbt += 1;
}

// channel c's sums over the slots of acc[slot][CA][2], in slot order: plain 16-byte loads, all issued before the first add
// (a rolled loop serialises 16 L2 round trips: ~4.5 us).  For sums a PREVIOUS launch completed.
__device__ __forceinline__ void bn_slot_sums(const double* acc, const int CA, const int c, const int nslots, double& s1, double& s2) {
  f64x2 v[MI_BN_SLOTS];
#pragma unroll
  for (int k = 0; k < MI_BN_SLOTS; ++k) v[k] = k < nslots ? *(const f64x2*)(acc + ((size_t)k * CA + c) * 2) : f64x2{0.0, 0.0};
  s1 = 0.0;
  s2 = 0.0;
#pragma unroll
  for (int k = 0; k < MI_BN_SLOTS; ++k) {
    s1 += v[k][0];
    s2 += v[k][1];
  }
}

// the statistics prologue of a streaming forward kernel (256 threads): scale / shift of every channel into LDS; block 0 also
// records.  n: acc (NULL: eval mode, scale / shift are inputs), nslots, inv_count, eps, gamma, beta + what bn_record takes
template <bool PAIRED, class P>
__device__ __forceinline__ void bn_fwd_prologue(P& n, const int C, const int bid, float* s_sc, float* s_sh) {
  const int CA = BN_ACC_C(C);
  if (n.acc) {
    for (int c = threadIdx.x; c < C; c += 256) {
      double s1, s2;
      bn_slot_sums(n.acc, CA, c, n.nslots, s1, s2);
      float sc, sh;
      const BnMoments m = bn_moments(s1, s2, n.inv_count, n.eps, n.gamma[c], n.beta[c], sc, sh);
      s_sc[c] = sc;
      s_sh[c] = sh;
      if (bid == 0) bn_record<PAIRED>(n, c, sc, sh, m, BN_NO_POISON);
    }
  } else {
    for (int c = threadIdx.x; c < C; c += 256) {
      s_sc[c] = n.scale[c];
      s_sh[c] = n.shift[c];
    }
  }
}

// ---- backward
// the prologue of a streaming apply kernel (256 threads): c1 = sum(dz) / count, c2 = sum(dz * xhat) / count of every channel
// into LDS; block 0 also writes dbeta = sum(dz), dgamma = sum(dz * xhat).  n: dacc, nslots, inv_count, dgamma, dbeta
template <class P>
__device__ __forceinline__ void bn_bwd_prologue(P& n, const int C, const int bid, float* s_c1, float* s_c2) {
  const int CA = BN_ACC_C(C);
  for (int c = threadIdx.x; c < C; c += 256) {
    double s1, s2;
    bn_slot_sums(n.dacc, CA, c, n.nslots, s1, s2);
    s_c1[c] = (float)(s1 * n.inv_count);
    s_c2[c] = (float)(s2 * n.inv_count);
    if (bid == 0) {
      if (n.dbeta) n.dbeta[c] = (float)s1;
      if (n.dgamma) n.dgamma[c] = (float)s2;
    }
  }
}

// channel sums of a block (256 threads; thread = pixel lane pl of channel group c8, PL lanes): red[pl][c8][8 * NS] -> one
// fp32 sum per (channel, quantity), lanes added in lane order, added to the block's slot with an fp64 atomic:
// quantity 0 -> d1[c][0] (and d2[c][0] when there is a second operand: sum dz is common to both), 1 -> d1[c][1], 2 -> d2[c][1]
template <int NS>
__device__ __forceinline__ void bn_block_sums(float* red, const float (*s)[8], const int C8, const int PL, const bool active,
                                              const int pl, const int c8, double* d1, double* d2) {
  const int tid = threadIdx.x;
  if (active) {
#pragma unroll
    for (int q = 0; q < NS; ++q)
#pragma unroll
      for (int e = 0; e < 8; ++e) red[(pl * C8 + c8) * (8 * NS) + q * 8 + e] = s[q][e];
  }
  __syncthreads();
  BN_TL(2);
  const int nout = C8 * 8 * NS;
  for (int j = tid; j < nout; j += 256) {
    float acc = 0.f;
    for (int q = 0; q < PL; ++q) acc += red[q * nout + j];
    const int cc8 = j / (8 * NS), v = j % (8 * NS);
    const int c = cc8 * 8 + (v & 7), q = v >> 3;
    if (q == 2) {
      atomicAdd(d2 + c * 2 + 1, (double)acc);
    } else {
      atomicAdd(d1 + c * 2 + q, (double)acc);
      if (NS == 3 && q == 0) atomicAdd(d2 + c * 2, (double)acc);
    }
  }
}
