// Train-mode BatchNorm + ReLU with a normed or a plain residual, NHWC bf16: the layers and the block tail of a RegNet block
// (detectron2's modeling/backbone/regnet.py as yolov7/modeling/backbone/regnet.py builds it: norm = "SyncBN", ReLU).
//
//   a = act(BN1(y1))                      a 1x1 / grouped 3x3 layer              2 tensor passes
//   a = act(BN1(y1) + BN2(y2))            the tail of a projection block         3
//   a = act(BN1(y1) + res)                the tail of an identity block          3
//
// each in ONE launch with ONE rounding at the store.  Composed from bn_act.hip's launches the projection tail is
// bn_act_fwd(act 0) on the projection (2 passes), bn_act_fwd(act 0, res) on c (3) and an elementwise ReLU (2): 7 passes and
// three roundings; the backward (ReLU' 3, then reduce 2 + apply 3 per norm) is 13 passes where the kernels here take 10 (reduce
// reads da, a, y1, y2; apply reads them again and writes dy1, dy2).
//
// The streaming loops follow the measured choices of bn_act.hip: a block uses TPB = (256 / C8) * C8 of its threads so that a
// thread keeps ONE channel group across the grid stride (C8 = 3, 7, 19, 46 for RegNetX-200MF) and its per-channel constants
// live in registers; four loads per tensor are in flight per trip (two in the apply pass, which holds four tensors); a thread's
// items are pixels pix0 + k * pstep - no 64-bit division per item; all slot loads of the statistics prologue are issued before
// the first add; at most 1024 blocks, since every block pays that prologue.
//
// Backward order: apply RECOMPUTES dz from (da, a) - except where storing it is free.  Both orders move the same number of
// tensors for a layer (7) and for the projection tail (10), and recomputing needs no buffer and keeps reduce read-only.  On the
// identity tail whose dres is overwritten dz IS dres: there reduce writes it and apply reads it back instead of (da, a), 7 passes
// instead of 8 (measured against the recomputing form, which LOST to the composition from bn_act.hip's launches at the largest
// map: profiles/regnet_probe.txt).  With `accumulate` dres already holds a gradient, so that form recomputes.
#include <string.h>
#include <stdlib.h>
#include "common.h"
#include "bn_common.h"

#define BR_MAX_BLOCKS 1024

// FORM: 0 one norm, 1 two norms, 2 one norm + plain residual
struct BrNormFwd {
  const __bf16* y;
  const double* acc;
  const float* gamma;
  const float* beta;
  float* rmean;
  float* rvar;
  int64_t* nbt;
  float* scale;
  float* shift;
  float* mean;
  float* invstd;
  double inv_count, unbias;
  float eps, momentum;
  int ldy, nslots;
};
struct BrFwdK {
  BrNormFwd n[2];
  const __bf16* res;
  __bf16* a;
  int64_t npix;
  int ldres, lda, C8;
};

template <int FORM, int RELU>
__global__ __launch_bounds__(256) void bn_relu_fwd_kernel(const BrFwdK p) {
  __shared__ float s_sc[FORM == 1 ? 2 : 1][BN_MAXC], s_sh[FORM == 1 ? 2 : 1][BN_MAXC];
  const int bid = blockIdx.x, nb = gridDim.x;
  const int C8 = p.C8, C = C8 * 8;
  bn_fwd_prologue<false>(p.n[0], C, bid, s_sc[0], s_sh[0]);
  if (FORM == 1) bn_fwd_prologue<false>(p.n[1], C, bid, s_sc[FORM == 1 ? 1 : 0], s_sh[FORM == 1 ? 1 : 0]);
  __syncthreads();
  const int64_t total = p.npix * C8;
  const int TPB = (256 / C8) * C8;
  if ((int)threadIdx.x >= TPB) return;
  const int c8 = (int)threadIdx.x % C8;
  float sc1[8], sh1[8], sc2[8], sh2[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    sc1[e] = s_sc[0][c8 * 8 + e];
    sh1[e] = s_sh[0][c8 * 8 + e];
    sc2[e] = FORM == 1 ? s_sc[FORM == 1 ? 1 : 0][c8 * 8 + e] : 0.f;
    sh2[e] = FORM == 1 ? s_sh[FORM == 1 ? 1 : 0][c8 * 8 + e] : 0.f;
  }
  const __bf16* y1 = p.n[0].y;
  const __bf16* y2 = FORM == 1 ? p.n[1].y : p.res;   // the second stream of either form
  const int ld1 = p.n[0].ldy, ld2 = FORM == 1 ? p.n[1].ldy : p.ldres;
  const int64_t stride = (int64_t)nb * TPB;
  const int64_t pstep = (int64_t)nb * (TPB / C8);
  int64_t pixb = (int64_t)bid * (TPB / C8) + (int)threadIdx.x / C8;
  for (int64_t idx = (int64_t)bid * TPB + threadIdx.x; idx < total; idx += 4 * stride, pixb += 4 * pstep) {
    bf16x8 v[4], r[4];
    int64_t pix[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      pix[u] = pixb + u * pstep;
      if (idx + u * stride < total) {
        v[u] = *(const bf16x8*)(y1 + pix[u] * ld1 + c8 * 8);
        if (FORM) r[u] = *(const bf16x8*)(y2 + pix[u] * ld2 + c8 * 8);
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (idx + u * stride >= total) break;
      float o[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        float z = (float)v[u][e] * sc1[e] + sh1[e];
        if (FORM == 1) z += (float)r[u][e] * sc2[e] + sh2[e];
        if (FORM == 2) z += (float)r[u][e];
        o[e] = RELU ? (z < 0.f ? 0.f : z) : z;   // (a NaN passes, as it does through torch.relu)
      }
      *(bf16x8*)(p.a + pix[u] * p.lda + c8 * 8) = pack8(o);
    }
  }
}

// ------------------------------------------------------------------ statistics of a map without a statistics epilogue
struct BrStatsK {
  const __bf16* x;
  double* acc;
  int64_t npix;
  int ldx, C8, nslots;
};
__global__ __launch_bounds__(256) void bn_stats_kernel(const BrStatsK p) {
  __shared__ float red[256 * 16];
  const int tid = threadIdx.x, bid = blockIdx.x, nb = gridDim.x;
  const int C8 = p.C8, PL = 256 / C8;
  const bool active = tid < PL * C8;
  const int c8 = tid % C8, pl = active ? tid / C8 : 0;
  float s[2][8];
#pragma unroll
  for (int e = 0; e < 8; ++e) s[0][e] = s[1][e] = 0.f;
  const int64_t pstride = (int64_t)nb * PL;
  for (int64_t pix0 = active ? (int64_t)bid * PL + pl : p.npix; pix0 < p.npix; pix0 += 4 * pstride) {
    bf16x8 xv[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t pix = pix0 + u * pstride;
      if (pix < p.npix) xv[u] = *(const bf16x8*)(p.x + pix * p.ldx + c8 * 8);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (pix0 + u * pstride >= p.npix) break;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float x = (float)xv[u][e];
        s[0][e] += x;
        s[1][e] += x * x;
      }
    }
  }
  double* slot = p.acc + (size_t)(bid % p.nslots) * BN_ACC_C(C8 * 8) * 2;
  bn_block_sums<2>(red, s, C8, PL, active, pl, c8, slot, nullptr);
}

// ------------------------------------------------------------------ backward
struct BrNormBwd {
  const __bf16* y;
  const float* mean;
  const float* invstd;
  const float* gamma;
  double* dacc;
  __bf16* dy;
  float* dgamma;
  float* dbeta;
  double inv_count;
  int ldy, lddy, nslots, pad_;
};
struct BrBwdK {
  BrNormBwd n[2];
  const __bf16* da;
  const __bf16* a;
  __bf16* dres;
  int64_t npix;
  int ldda, lda, lddres, accumulate, C8, pad_;
};

// pass 1: (sum dz, sum dz * xhat_1 [, sum dz * xhat_2]); sum dz goes to both operands' accumulators.  STORE (the residual
// form whose dres is overwritten): dz IS the residual's gradient - written here, read back by apply instead of (da, a)
template <int TWO, int RELU, int STORE>
__global__ __launch_bounds__(256) void bn_relu_bwd_reduce_kernel(const BrBwdK p) {
  constexpr int NS = TWO ? 3 : 2;
  __shared__ float red[256 * 8 * NS];
  const int tid = threadIdx.x, bid = blockIdx.x, nb = gridDim.x;
  const int C8 = p.C8, PL = 256 / C8;
  const bool active = tid < PL * C8;
  const int c8 = tid % C8, pl = active ? tid / C8 : 0;
  float mu1[8], is1[8], mu2[8], is2[8], s[NS][8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    mu1[e] = p.n[0].mean[c8 * 8 + e];
    is1[e] = p.n[0].invstd[c8 * 8 + e];
    mu2[e] = TWO ? p.n[1].mean[c8 * 8 + e] : 0.f;
    is2[e] = TWO ? p.n[1].invstd[c8 * 8 + e] : 0.f;
#pragma unroll
    for (int q = 0; q < NS; ++q) s[q][e] = 0.f;
  }
  const int64_t pstride = (int64_t)nb * PL;
  for (int64_t pix0 = active ? (int64_t)bid * PL + pl : p.npix; pix0 < p.npix; pix0 += 4 * pstride) {
    bf16x8 dv[4], av[4], y1[4], y2[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t pix = pix0 + u * pstride;
      if (pix < p.npix) {
        dv[u] = *(const bf16x8*)(p.da + pix * p.ldda + c8 * 8);
        if (RELU) av[u] = *(const bf16x8*)(p.a + pix * p.lda + c8 * 8);
        y1[u] = *(const bf16x8*)(p.n[0].y + pix * p.n[0].ldy + c8 * 8);
        if (TWO) y2[u] = *(const bf16x8*)(p.n[1].y + pix * p.n[1].ldy + c8 * 8);
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (pix0 + u * pstride >= p.npix) break;
      float dzv[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        float dz = (float)dv[u][e];
        if (RELU) dz = (float)av[u][e] > 0.f ? dz : 0.f;
        dzv[e] = dz;
        s[0][e] += dz;
        s[1][e] += dz * (((float)y1[u][e] - mu1[e]) * is1[e]);
        if (TWO) s[NS - 1][e] += dz * (((float)y2[u][e] - mu2[e]) * is2[e]);
      }
      if (STORE) *(bf16x8*)(p.dres + (pix0 + u * pstride) * p.lddres + c8 * 8) = pack8(dzv);   // (exact: da or 0)
    }
  }
  const size_t so = (size_t)BN_ACC_C(C8 * 8) * 2;
  double* d1 = p.n[0].dacc + (size_t)(bid % p.n[0].nslots) * so;
  double* d2 = TWO ? p.n[1].dacc + (size_t)(bid % p.n[1].nslots) * so : nullptr;
  bn_block_sums<NS>(red, s, C8, PL, active, pl, c8, d1, d2);
}

// pass 2
// FROMDZ: reduce stored dz in dres (see there); da, a are not read and dres is not written again
template <int TWO, int RELU, int FROMDZ>
__global__ __launch_bounds__(256) void bn_relu_bwd_apply_kernel(const BrBwdK p) {
  __shared__ float s_c1[TWO ? 2 : 1][BN_MAXC], s_c2[TWO ? 2 : 1][BN_MAXC];
  const int bid = blockIdx.x, nb = gridDim.x;
  const int C8 = p.C8, C = C8 * 8;
  bn_bwd_prologue(p.n[0], C, bid, s_c1[0], s_c2[0]);
  if (TWO) bn_bwd_prologue(p.n[1], C, bid, s_c1[TWO ? 1 : 0], s_c2[TWO ? 1 : 0]);
  __syncthreads();
  const int64_t total = p.npix * C8;
  const int TPB = (256 / C8) * C8;
  if ((int)threadIdx.x >= TPB) return;
  const int c8 = (int)threadIdx.x % C8;
  float mu[2][8], is[2][8], gi[2][8], k1[2][8], k2[2][8];
#pragma unroll
  for (int k = 0; k < (TWO ? 2 : 1); ++k)
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int c = c8 * 8 + e;
      mu[k][e] = p.n[k].mean[c];
      is[k][e] = p.n[k].invstd[c];
      gi[k][e] = p.n[k].gamma[c] * is[k][e];
      k1[k][e] = s_c1[k][c];
      k2[k][e] = s_c2[k][c];
    }
  const bool racc = !FROMDZ && p.dres && p.accumulate;
  const int64_t stride = (int64_t)nb * TPB;
  const int64_t pstep = (int64_t)nb * (TPB / C8);
  int64_t pixb = (int64_t)bid * (TPB / C8) + (int)threadIdx.x / C8;
  for (int64_t idx = (int64_t)bid * TPB + threadIdx.x; idx < total; idx += 2 * stride, pixb += 2 * pstep) {
    bf16x8 dv[2], av[2], y1[2], y2[2], rv[2];
    int64_t pix[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      pix[u] = pixb + u * pstep;
      if (idx + u * stride < total) {
        if (FROMDZ) dv[u] = *(const bf16x8*)(p.dres + pix[u] * p.lddres + c8 * 8);
        else dv[u] = *(const bf16x8*)(p.da + pix[u] * p.ldda + c8 * 8);
        if (RELU && !FROMDZ) av[u] = *(const bf16x8*)(p.a + pix[u] * p.lda + c8 * 8);
        y1[u] = *(const bf16x8*)(p.n[0].y + pix[u] * p.n[0].ldy + c8 * 8);
        if (TWO) y2[u] = *(const bf16x8*)(p.n[1].y + pix[u] * p.n[1].ldy + c8 * 8);
        if (racc) rv[u] = *(const bf16x8*)(p.dres + pix[u] * p.lddres + c8 * 8);
      }
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      if (idx + u * stride >= total) break;
      float dz[8], o[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        dz[e] = (float)dv[u][e];
        if (RELU && !FROMDZ) dz[e] = (float)av[u][e] > 0.f ? dz[e] : 0.f;
        const float xh = ((float)y1[u][e] - mu[0][e]) * is[0][e];
        o[e] = gi[0][e] * (dz[e] - k1[0][e] - xh * k2[0][e]);
      }
      *(bf16x8*)(p.n[0].dy + pix[u] * p.n[0].lddy + c8 * 8) = pack8(o);
      if (TWO) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float xh = ((float)y2[u][e] - mu[TWO ? 1 : 0][e]) * is[TWO ? 1 : 0][e];
          o[e] = gi[TWO ? 1 : 0][e] * (dz[e] - k1[TWO ? 1 : 0][e] - xh * k2[TWO ? 1 : 0][e]);
        }
        *(bf16x8*)(p.n[1].dy + pix[u] * p.n[1].lddy + c8 * 8) = pack8(o);
      }
      if (!FROMDZ && p.dres) {
        if (racc) {
#pragma unroll
          for (int e = 0; e < 8; ++e) dz[e] += (float)rv[u][e];
        }
        *(bf16x8*)(p.dres + pix[u] * p.lddres + c8 * 8) = pack8(dz);
      }
    }
  }
}

// ------------------------------------------------------------------ host side
// 512 items per block as bn_act.hip's ew_blocks measured.  The backward sums take 1024 (four items per thread: the grid the callers
// of mi_bn_act_bwd_reduce ask for), the statistics pass 2048: each of their blocks ends with 2 - 3 fp64 atomics per channel
static int br_blocks(int64_t total, int64_t per) {
  int64_t b = (total + per - 1) / per;
  if (b > BR_MAX_BLOCKS) b = BR_MAX_BLOCKS;
  if (b < 1) b = 1;
  return (int)b;
}

static int br_check_common(const mi_bn_relu_desc* d, const char* who) {
  MI_REQUIRE(d != nullptr, "%s: null descriptor", who);
  MI_REQUIRE(d->C > 0 && d->C % 8 == 0 && d->C <= BN_MAXC, "%s: C %d (need C %% 8 == 0, 0 < C <= %d)", who, d->C, BN_MAXC);
  MI_REQUIRE(d->npix > 0, "%s: npix %lld is not positive", who, (long long)d->npix);
  MI_REQUIRE(d->n1.y != nullptr, "%s: null n1.y (the main operand is mandatory)", who);
  return MI_OK;
}
static int br_check_view(const void* p, int ld, int C, const char* who, const char* name) {
  MI_REQUIRE(ld % 8 == 0 && ld >= C, "%s: leading dimension %s %d is not a multiple of 8 that is >= C %d", who, name, ld, C);
  MI_REQUIRE(bn_al16(p), "%s: %s is not 16-byte aligned", who, name);
  return MI_OK;
}

extern "C" int mi_bn_relu_desc_size(void) { return (int)sizeof(mi_bn_relu_desc); }

extern "C" int mi_bn_stats(const void* x, int ldx, int64_t npix, int C, double* acc, int nslots, mi_stream_t st) {
  MI_REQUIRE(C > 0 && C % 8 == 0 && C <= BN_MAXC, "mi_bn_stats: C %d (need C %% 8 == 0, 0 < C <= %d)", C, BN_MAXC);
  MI_REQUIRE(npix > 0, "mi_bn_stats: npix %lld is not positive", (long long)npix);
  MI_REQUIRE(x != nullptr && acc != nullptr, "mi_bn_stats: null x / acc");
  if (int rc = br_check_view(x, ldx, C, "mi_bn_stats", "ldx / x")) return rc;
  MI_REQUIRE(bn_al16(acc), "mi_bn_stats: acc is not 16-byte aligned");
  BrStatsK k;
  k.x = (const __bf16*)x; k.acc = acc; k.npix = npix; k.ldx = ldx; k.C8 = C / 8; k.nslots = bn_slots(nslots);
  hipLaunchKernelGGL(bn_stats_kernel, dim3(br_blocks(npix * (C / 8), 2048)), dim3(256), 0, (hipStream_t)st, k);
  MI_CHECK_LAUNCH("bn_stats");
  return MI_OK;
}

static int br_fill_fwd(const mi_bn_relu_norm& n, int C, const char* who, const char* name, BrNormFwd* o) {
  if (int rc = br_check_view(n.y, n.ldy, C, who, name)) return rc;
  MI_REQUIRE(n.scale != nullptr && n.shift != nullptr, "%s: null scale / shift of %s", who, name);
  MI_REQUIRE(!n.acc || (n.gamma && n.beta && n.mean && n.invstd && n.count > 0),
             "%s: train mode needs gamma / beta / mean / invstd and a positive count of %s", who, name);
  MI_REQUIRE(bn_al16(n.acc), "%s: acc of %s is not 16-byte aligned", who, name);
  o->y = (const __bf16*)n.y; o->acc = n.acc; o->gamma = n.gamma; o->beta = n.beta; o->rmean = n.running_mean;
  o->rvar = n.running_var; o->nbt = n.num_batches_tracked; o->scale = n.scale; o->shift = n.shift; o->mean = n.mean;
  o->invstd = n.invstd; o->inv_count = n.count > 0 ? 1.0 / (double)n.count : 0.0;
  o->unbias = n.count > 1 ? (double)n.count / (double)(n.count - 1) : 1.0;
  o->eps = n.eps; o->momentum = n.momentum; o->ldy = n.ldy; o->nslots = bn_slots(n.nslots);
  return MI_OK;
}

extern "C" int mi_bn_relu_fwd(const mi_bn_relu_desc* d, mi_stream_t st) {
  const char* who = "mi_bn_relu_fwd";
  if (int rc = br_check_common(d, who)) return rc;
  MI_REQUIRE(d->a != nullptr, "%s: null output a", who);
  MI_REQUIRE(!(d->n2.y && d->res), "%s: both a second norm operand (n2.y) and a plain residual (res) given", who);
  BrFwdK k;
  memset(&k, 0, sizeof(k));
  if (int rc = br_fill_fwd(d->n1, d->C, who, "n1.y", &k.n[0])) return rc;
  if (d->n2.y)
    if (int rc = br_fill_fwd(d->n2, d->C, who, "n2.y", &k.n[1])) return rc;
  if (d->res)
    if (int rc = br_check_view(d->res, d->ldres, d->C, who, "res")) return rc;
  if (int rc = br_check_view(d->a, d->lda, d->C, who, "a")) return rc;
  k.res = (const __bf16*)d->res; k.a = (__bf16*)d->a; k.npix = d->npix; k.ldres = d->ldres; k.lda = d->lda; k.C8 = d->C / 8;
  const int form = d->n2.y ? 1 : (d->res ? 2 : 0);
  const dim3 g(br_blocks(d->npix * (d->C / 8), 512)), b(256);
  hipStream_t s = (hipStream_t)st;
  if (d->relu) {
    if (form == 0) hipLaunchKernelGGL((bn_relu_fwd_kernel<0, 1>), g, b, 0, s, k);
    else if (form == 1) hipLaunchKernelGGL((bn_relu_fwd_kernel<1, 1>), g, b, 0, s, k);
    else hipLaunchKernelGGL((bn_relu_fwd_kernel<2, 1>), g, b, 0, s, k);
  } else {
    if (form == 0) hipLaunchKernelGGL((bn_relu_fwd_kernel<0, 0>), g, b, 0, s, k);
    else if (form == 1) hipLaunchKernelGGL((bn_relu_fwd_kernel<1, 0>), g, b, 0, s, k);
    else hipLaunchKernelGGL((bn_relu_fwd_kernel<2, 0>), g, b, 0, s, k);
  }
  MI_CHECK_LAUNCH("bn_relu_fwd");
  return MI_OK;
}

static int br_fill_bwd(const mi_bn_relu_norm& n, int C, bool apply, const char* who, const char* name, BrNormBwd* o) {
  if (int rc = br_check_view(n.y, n.ldy, C, who, name)) return rc;
  MI_REQUIRE(n.mean != nullptr && n.invstd != nullptr && n.dacc != nullptr, "%s: null mean / invstd / dacc of %s", who, name);
  MI_REQUIRE(bn_al16(n.dacc), "%s: dacc of %s is not 16-byte aligned", who, name);
  if (apply) {
    MI_REQUIRE(n.gamma != nullptr && n.dy != nullptr && n.count > 0, "%s: null gamma / dy or no count of %s", who, name);
    if (int rc = br_check_view(n.dy, n.lddy, C, who, "dy")) return rc;
  }
  o->y = (const __bf16*)n.y; o->mean = n.mean; o->invstd = n.invstd; o->gamma = n.gamma; o->dacc = n.dacc;
  o->dy = (__bf16*)n.dy; o->dgamma = n.dgamma; o->dbeta = n.dbeta; o->inv_count = n.count > 0 ? 1.0 / (double)n.count : 0.0;
  o->ldy = n.ldy; o->lddy = n.lddy; o->nslots = bn_slots(n.nslots); o->pad_ = 0;
  return MI_OK;
}

// the residual form whose dres is overwritten: reduce writes dres = dz and apply reads it back - 7 tensor passes instead of 8
static inline bool br_stores_dz(const mi_bn_relu_desc* d) { return !d->n2.y && d->dres && !d->accumulate; }

static int br_bwd_args(const mi_bn_relu_desc* d, bool apply, const char* who, BrBwdK* k) {
  if (int rc = br_check_common(d, who)) return rc;
  MI_REQUIRE(d->da != nullptr, "%s: null da", who);
  MI_REQUIRE(!d->relu || d->a != nullptr, "%s: null saved output a (relu needs it)", who);
  MI_REQUIRE(!(d->n2.y && (d->res || d->dres)), "%s: both a second norm operand (n2.y) and a plain residual (res / dres) given", who);
  memset(k, 0, sizeof(*k));
  if (int rc = br_fill_bwd(d->n1, d->C, apply, who, "n1.y", &k->n[0])) return rc;
  if (d->n2.y)
    if (int rc = br_fill_bwd(d->n2, d->C, apply, who, "n2.y", &k->n[1])) return rc;
  if (int rc = br_check_view(d->da, d->ldda, d->C, who, "da")) return rc;
  if (d->relu)
    if (int rc = br_check_view(d->a, d->lda, d->C, who, "a")) return rc;
  // reduce touches dres only where it stores dz there (br_stores_dz)
  const bool use_dres = d->dres && (apply || br_stores_dz(d));
  if (use_dres)
    if (int rc = br_check_view(d->dres, d->lddres, d->C, who, "dres")) return rc;
  k->da = (const __bf16*)d->da; k->a = (const __bf16*)d->a; k->dres = use_dres ? (__bf16*)d->dres : nullptr; k->npix = d->npix;
  k->ldda = d->ldda; k->lda = d->lda; k->lddres = d->lddres; k->accumulate = d->accumulate; k->C8 = d->C / 8;
  return MI_OK;
}

extern "C" int mi_bn_relu_bwd_reduce(const mi_bn_relu_desc* d, mi_stream_t st) {
  BrBwdK k;
  if (int rc = br_bwd_args(d, false, "mi_bn_relu_bwd_reduce", &k)) return rc;
  const dim3 g(br_blocks(d->npix * (d->C / 8), 1024)), b(256);
  hipStream_t s = (hipStream_t)st;
  if (d->n2.y) {
    if (d->relu) hipLaunchKernelGGL((bn_relu_bwd_reduce_kernel<1, 1, 0>), g, b, 0, s, k);
    else hipLaunchKernelGGL((bn_relu_bwd_reduce_kernel<1, 0, 0>), g, b, 0, s, k);
  } else if (br_stores_dz(d)) {
    if (d->relu) hipLaunchKernelGGL((bn_relu_bwd_reduce_kernel<0, 1, 1>), g, b, 0, s, k);
    else hipLaunchKernelGGL((bn_relu_bwd_reduce_kernel<0, 0, 1>), g, b, 0, s, k);
  } else {
    if (d->relu) hipLaunchKernelGGL((bn_relu_bwd_reduce_kernel<0, 1, 0>), g, b, 0, s, k);
    else hipLaunchKernelGGL((bn_relu_bwd_reduce_kernel<0, 0, 0>), g, b, 0, s, k);
  }
  MI_CHECK_LAUNCH("bn_relu_bwd_reduce");
  return MI_OK;
}

extern "C" int mi_bn_relu_bwd_apply(const mi_bn_relu_desc* d, mi_stream_t st) {
  BrBwdK k;
  if (int rc = br_bwd_args(d, true, "mi_bn_relu_bwd_apply", &k)) return rc;
  const dim3 g(br_blocks(d->npix * (d->C / 8), 512)), b(256);
  hipStream_t s = (hipStream_t)st;
  if (d->n2.y) {
    if (d->relu) hipLaunchKernelGGL((bn_relu_bwd_apply_kernel<1, 1, 0>), g, b, 0, s, k);
    else hipLaunchKernelGGL((bn_relu_bwd_apply_kernel<1, 0, 0>), g, b, 0, s, k);
  } else if (br_stores_dz(d)) {
    hipLaunchKernelGGL((bn_relu_bwd_apply_kernel<0, 0, 1>), g, b, 0, s, k);
  } else {
    if (d->relu) hipLaunchKernelGGL((bn_relu_bwd_apply_kernel<0, 1, 0>), g, b, 0, s, k);
    else hipLaunchKernelGGL((bn_relu_bwd_apply_kernel<0, 0, 0>), g, b, 0, s, k);
  }
  MI_CHECK_LAUNCH("bn_relu_bwd_apply");
  return MI_OK;
}
