// What train-mode BatchNorm shares between bn_act.hip and the two persistent convolution kernels (conv1x1_stream.h /
// conv3x3_ws.h):
//   * the grid-wide barrier over the resident blocks of one launch, in two halves (bn_bar_arrive / bn_bar_finish): the
//     one-launch BatchNorm backward of bn_act.hip (bn_bwd_fused);
//   * CBnFwd, the record of one BatchNorm(train) forward, and cbn_apply8, its expression on 8 channels of a pixel;
//   * cbn_block_stats, the (sum, sumsq) tail of a convolution launch with statistics (MODE 1);
//   * BnXf / bnx_tables / bnx_apply_lds: the BatchNorm + activation of a convolution's INPUT, run by the consuming launch.
#pragma once
#include "common.h"
#include "bn_common.h"
#include "bn_barrier.h"

#define BN_FUS_SPIN_LIMIT (1 << 22)
// diagnostic build of bn_act.hip (MI_BN_CHAIN_TIMELINE): thread 0 of every block stamps point k of the chain; nothing otherwise
#ifndef BN_TL
#define BN_TL(k) do { } while (0)
#endif
// Grid-wide barrier over nb resident blocks.  Agent-scope atomics are performed memory-side, one after the other per
// address (~0.1 us each: 512 arrivals on ONE counter cost ~50 us, measured), so arrivals go through a two-level tree -
// MI_BN_BAR_GROUPS group counters (block % groups), whose last arrivers meet on the top counter - and every group waits
// on its own generation word; each word sits on its own 256-byte line.  Word layout (uint32):
//   [0] top arrivals  [2] give-up flag  [64 * (1 + g)] generation of group g  [64 * (1 + G + g)] arrivals of group g
// (On the tree a block's arrival, its block barrier included, takes 0.5 us and a release is seen 0.1 us after it is issued:
// profiles/bn_bwd_chain_ab.txt.)  The protocol itself is bn_barrier.h's, written over an atomics policy so that tests/native/bn_barrier_host.cpp runs the
// same text on the CPU; BnbHip is the kernel's policy: relaxed agent-scope atomics.
static_assert(BNB_G == MI_BN_BAR_GROUPS && BNB_WORDS == MI_BN_BAR_WORDS, "bn_barrier.h states the layout of include/mi355_det.h");
struct BnbHip {
  static __device__ __forceinline__ unsigned fetch_add(unsigned* p, unsigned v) {
    return __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  static __device__ __forceinline__ void add(unsigned* p, unsigned v) {
    (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // result unused: no return, no wait
  }
  static __device__ __forceinline__ unsigned load(const unsigned* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  static __device__ __forceinline__ void store(unsigned* p, unsigned v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  static __device__ __forceinline__ void pause() { __builtin_amdgcn_s_sleep(8); }
};
// No cache maintenance: an agent-scope acquire / release (or __threadfence) writes back and invalidates the XCD's whole L2
// - issued by hundreds of polling blocks that stalls every block still streaming (measured: +90 us per launch).  It is not
// needed here: the only data that crosses blocks are the fp64 sums, added by memory-side atomics that have been
// acknowledged when the block passes its __syncthreads (workgroup release = s_waitcnt vmcnt(0)), and read back after the
// barrier by agent-scope (sc1) loads, which bypass the non-coherent caches.
// *gave_up (LDS) = 1 when this block's wait timed out: its sums are incomplete and it must poison what it writes.
// The barrier in two halves, so that the block that arrives LAST can do work for everybody before it releases the
// others (bn_bwd_fused: it folds the accumulator slots into one total per channel - one block's worth of loads instead of
// every block's; see bn_act.hip).  *is_last / *gave_up live in LDS.
__device__ __forceinline__ unsigned bn_bar_generation(unsigned* bar, const int bid, const int nb) {
  return bnb_generation<BnbHip>(bar, bid, nb);
}
__device__ __forceinline__ void bn_bar_arrive(unsigned* bar, const int bid, const int nb, int* gave_up, int* is_last) {
  // every thread's fp64 atomicAdds must have been acknowledged before thread 0 counts the arrival: stated explicitly - the
  // memory model does not promise that a workgroup-scope barrier waits for vmcnt(0)
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  BN_TL(3);
  __syncthreads();
  if (threadIdx.x == 0) {
    *gave_up = 0;
    *is_last = bnb_arrive<BnbHip>(bar, bid, nb) ? 1 : 0;
    BN_TL(4);
  }
  __syncthreads();
}
__device__ __forceinline__ void bn_bar_finish(unsigned* bar, const unsigned gen0, const int bid, const int nb, int* gave_up,
                                              const int* is_last) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the last block's write-through stores of the folded totals: acknowledged
  __syncthreads();
  if (*is_last) {
    // one lane per group: the bumps leave in one instruction and nobody waits for what they return
    BN_TL(6);
    if ((int)threadIdx.x < bnb_groups(nb)) bnb_release_group<BnbHip>(bar, (int)threadIdx.x);
    BN_TL(7);
  } else if (threadIdx.x == 0) {
    if (bnb_wait<BnbHip>(bar, gen0, bid, nb, BN_FUS_SPIN_LIMIT)) *gave_up = 1;
    BN_TL(8);
  }
  __syncthreads();
}

// ---- one BatchNorm(train) forward: the record BnXf embeds (and mi_bnx mirrors)
struct CBnFwd {
  const __bf16* res;   // residual added after the activation (Bottleneck shortcut) or NULL
  __bf16* a;           // activated output
  const float* gamma;
  const float* beta;
  float* rmean;        // running statistics (may be NULL)
  float* rvar;
  long long* nbt;
  float* scale;        // written for the backward pass: scale / shift / mean / invstd [C]
  float* shift;
  float* mean;
  float* invstd;
  int ldres, lda, act, pad_;
  double inv_count, unbias;
  float eps, momentum;
};

// 8 channels of one pixel: a = act(y * scale + shift) (+ res), the expression of bn_act_fwd_body
__device__ __forceinline__ u32x4 cbn_apply8(const u32x4 yv, const float* sc, const float* sh, const int act, const bool has_res,
                                            const u32x4 rv) {
  const bf16x8 v = __builtin_bit_cast(bf16x8, yv), r = __builtin_bit_cast(bf16x8, rv);
  float o[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const float z = (float)v[e] * sc[e] + sh[e];
    o[e] = act ? z * sigmoidf_(z) : z;
  }
  if (has_res) {
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] += (float)r[e];
  }
  return __builtin_bit_cast(u32x4, pack8(o));
}

// ---- the block's BatchNorm (sum, sumsq) of a persistent convolution launch: the tail behind the tile loop of c1s_kernel /
// w3_kernel (MODE 1, XF).  Every lane arrives with 16 channels x (sum, sumsq) over ITS pixels: lane (l31, h) of wave
// (wm, wn) holds channel wm * 32 + 8 (r >> 2) + 4 h + (r & 3) in register r (the MFMA accumulator order).
// value of lane (lane ^ OFF), OFF < 32: DPP where gfx950 has a form with these operands (quad_perm for 1 and 2, a rotation
// by half a row for 8), ds_bpermute for 4 and 16.  Called with every lane active.
template <int OFF>
__device__ __forceinline__ float cbn_lane_xor(const float v) {
  const int i = __builtin_bit_cast(int, v);
  if constexpr (OFF == 1) return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, i, 0xB1, 0xF, 0xF, true));        // quad_perm:[1,0,3,2]
  else if constexpr (OFF == 2) return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, i, 0x4E, 0xF, 0xF, true));   // quad_perm:[2,3,0,1]
  else if constexpr (OFF == 8) return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, i, 0x128, 0xF, 0xF, true));  // row_ror:8
  else return __shfl_xor(v, OFF, 64);
}
// One level of the halving exchange over the lane pairs (l, l ^ OFF): the lane whose OFF bit is clear keeps registers
// [0, N), the other one [N, 2 N); each receives the partner's values of the half it keeps.  out[k] = own + partner's: the
// sum the full butterfly `s[r] += shfl_xor(s[r], OFF)` leaves in BOTH lanes (an fp32 addition commutes bit for bit), so the
// pairing tree of every channel - and with it every bit of the block's partial sums - is the butterfly's.
template <int N, int OFF>
__device__ __forceinline__ void cbn_halve(const float (&in)[2 * N], float (&out)[N], const bool up) {
#pragma unroll
  for (int k = 0; k < N; ++k) {
    const float keep = up ? in[k + N] : in[k], send = up ? in[k] : in[k + N];
    out[k] = keep + cbn_lane_xor<OFF>(send);
  }
}
// 16 registers over the 32 lanes of a half-wave -> one: 8 + 4 + 2 + 1 exchanges, then one full exchange across xor 16 (16 in
// place of the butterfly's 80).  Lane l31 ends with register r = 8 b0 + 4 b1 + 2 b2 + b3 (b_i: bit i of l31); lanes l31 and
// l31 ^ 16 hold the same value.
__device__ __forceinline__ float cbn_fold32(const float (&s)[16], const int l31) {
  float t8[8], t4[4], t2[2], t1[1];
  cbn_halve<8, 1>(s, t8, (l31 & 1) != 0);
  cbn_halve<4, 2>(t8, t4, (l31 & 2) != 0);
  cbn_halve<2, 4>(t4, t2, (l31 & 4) != 0);
  cbn_halve<1, 8>(t2, t1, (l31 & 8) != 0);
  return t1[0] + cbn_lane_xor<16>(t1[0]);
}
// The tail.  `red`: the block's LDS from offset 0 (the tile ring: dead once every wave has passed the first barrier - the
// caller has waited for ITS LDS-DMAs with a counted vmcnt, the output stores behind them stay in flight beside all of this);
// stats_of(c): the (sum, sumsq) fp64 pair of the block's channel c = wm * 32 + .. in this block's slot.  WN > 1: the 16
// owning lanes of each half-wave park their channel's pair in red[wn][c], one lane per channel adds the WN values in the
// order 0 .. WN - 1 (from 0.f, as ever) and issues the two atomics.  WN == 1: no LDS stage and no barrier, the owning lanes
// issue them.  noatom: the timing switch (MI_DEBUG_NOATOM), everything but the atomics.
template <int WM, int WN, class StatsOf>
__device__ __forceinline__ void cbn_block_stats(const float (&s1)[16], const float (&s2)[16], float* red, const int wave,
                                                const int lane, const bool noatom, StatsOf&& stats_of) {
#ifdef MI_CONV_STATS_NOTAIL   // diagnostic build (tools/build_variant.sh): the per-tile accumulation without the tail
#pragma unroll
  for (int r = 0; r < 16; ++r) asm volatile("" ::"v"(s1[r]), "v"(s2[r]));
  return;
#endif
  const int wm = wave / WN, wn = wave % WN, l31 = lane & 31, h = lane >> 5;
  const float f1 = cbn_fold32(s1, l31), f2 = cbn_fold32(s2, l31);
  const int r = ((l31 & 1) << 3) | ((l31 & 2) << 1) | ((l31 & 4) >> 1) | ((l31 & 8) >> 3);
  const int c = wm * 32 + 8 * (r >> 2) + 4 * h + (r & 3);
  if constexpr (WN == 1) {
    if (l31 < 16 && !noatom) {
      double* sp = stats_of(c);
      atomicAdd(sp, (double)f1);
      atomicAdd(sp + 1, (double)f2);
    }
  } else {
    // (the address - a slot division, the slice's table entry - before the barriers, not behind them)
    double* const sp = stats_of((wave < WM ? wave : 0) * 32 + l31);
    __syncthreads();   // every wave is done with the ring (its reads and its LDS-DMAs)
    if (l31 < 16) *(float2*)(red + (wn * WM * 32 + c) * 2) = float2{f1, f2};   // red: [WN][WM * 32][2]
    __syncthreads();
    if (wave < WM && lane < 32) {
      float a1 = 0.f, a2 = 0.f;
#pragma unroll
      for (int q = 0; q < WN; ++q) {
        const float2 v = *(const float2*)(red + (q * WM * 32 + wave * 32 + lane) * 2);
        a1 += v.x;
        a2 += v.y;
      }
      if (!noatom) {
        atomicAdd(sp, (double)a1);
        atomicAdd(sp + 1, (double)a2);
      }
    }
  }
}

// ---- BatchNorm(train) + activation of a convolution's INPUT, applied by the consuming launch ("BN in the consumer")
// The producer left the raw output y and its fp64 (sum, sumsq) accumulators; instead of a bn_act_fwd launch that reads y
// and writes a = act(y * scale + shift), the consumer fetches y tiles (LDS-DMA), every wave rewrites the 16-byte pieces it
// fetched itself IN LDS with cbn_apply8 (the expression and the rounding point of bn_act_fwd_body: the fragments the
// matrix cores see are bit-identical to the two-launch form) and the launch's writer job stores the same values to `a`
// for the later readers of the tensor (weight gradient, residuals, pooling).  BaseConv.forward's norm + act
// (yolov7/modeling/backbone/layers/wrappers.py:76-83) without a launch of its own and without re-reading y.
struct BnXf {
  CBnFwd bn;           // gamma .. invstd, running statistics, eps / momentum / counts; a / lda: the activated tensor; res unused
  const double* acc;   // the producer's accumulators [nslots][sld / 2][2]
  int sld, nslots, C, pad_;
};
static_assert(sizeof(BnXf) == sizeof(mi_bnx) && __builtin_offsetof(BnXf, acc) == __builtin_offsetof(mi_bnx, acc) &&
              __builtin_offsetof(BnXf, bn.inv_count) == __builtin_offsetof(mi_bnx, inv_count) &&
              __builtin_offsetof(BnXf, bn.lda) == __builtin_offsetof(mi_bnx, lda), "mi_bnx (include/mi355_det.h) mirrors BnXf");
// every block: (scale, shift) of all C input channels into LDS tables - the arithmetic of bn_fwd_prologue (bn_common.h) with
// ITS loads: plain 16-byte loads, thread c next to thread c + 1 (the sums were completed by the previous launch;
// agent-scope 8-byte atomic loads are for readers BEHIND a grid barrier and cost one L2 request each: with
// every block of a launch asking for the same C x nslots x 16 bytes they took ~9 us of a 512-channel 20x20 launch).
// `rec`: this block also records scale / shift / mean / invstd for the backward pass and updates the running statistics
__device__ __forceinline__ void bnx_tables(const BnXf* __restrict__ xf, float* s_sc, float* s_sh, const int nthreads, const bool rec) {
  const int C = xf->C, nslots = xf->nslots;
  const size_t sld2 = (size_t)(xf->sld >> 1);   // f64x2 elements between slots
  const CBnFwd& bn = xf->bn;
  for (int c = threadIdx.x; c < C; c += nthreads) {
    const f64x2* const ap = (const f64x2*)xf->acc + c;
    f64x2 v[MI_BN_SLOTS];
#pragma unroll
    for (int k = 0; k < MI_BN_SLOTS; ++k) v[k] = ap[(k < nslots ? (size_t)k : 0) * sld2];   // (unconditional: all in flight together)
    double s1 = 0.0, s2 = 0.0;
#pragma unroll
    for (int k = 0; k < MI_BN_SLOTS; ++k) {
      s1 += k < nslots ? v[k][0] : 0.0;
      s2 += k < nslots ? v[k][1] : 0.0;
    }
    float sc, sh;
    const BnMoments m = bn_moments(s1, s2, bn.inv_count, bn.eps, bn.gamma[c], bn.beta[c], sc, sh);
    s_sc[c] = sc;
    s_sh[c] = sh;
    if (rec) bn_record<true>(bn, c, sc, sh, m, BN_NO_POISON);
  }
}
// one 16-byte piece (8 channels cg * 8 .. of one pixel), in place; returns what it wrote
__device__ __forceinline__ u32x4 bnx_apply_lds(char* sp, const float* s_sc, const float* s_sh, const int cg, const int act, const bool valid) {
  const u32x4 raw = *(const u32x4*)sp;
  const f32x4 c0 = *(const f32x4*)(s_sc + cg * 8), c1 = *(const f32x4*)(s_sc + cg * 8 + 4);
  const f32x4 h0 = *(const f32x4*)(s_sh + cg * 8), h1 = *(const f32x4*)(s_sh + cg * 8 + 4);
  const float sc[8] = {c0[0], c0[1], c0[2], c0[3], c1[0], c1[1], c1[2], c1[3]};
  const float sh[8] = {h0[0], h0[1], h0[2], h0[3], h1[0], h1[1], h1[2], h1[3]};
  u32x4 o = cbn_apply8(raw, sc, sh, act, false, u32x4{0u, 0u, 0u, 0u});
  if (!valid) o = u32x4{0u, 0u, 0u, 0u};   // zero padding stays zero (act(shift) is not)
  *(u32x4*)sp = o;
  return o;
}
