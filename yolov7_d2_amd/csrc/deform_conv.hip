// Deformable 3x3 convolution (detectron2 DeformConv: unmodulated, one deformable group, groups 1) in the STAGED form: this
// file samples, the GEMMs stay on the convolution kernels.
//   forward   mi_deform_im2col : x[N,H,W,C] + offsets -> col[N*Ho*Wo, 9*C] (bf16, tap-major, channels contiguous inside a tap);
//             y = col . W is then an ordinary 1x1 convolution with 9*C input channels (mi_conv2d)
//   backward  dcol = dy . W^T (1x1 data gradient), gW = col^T . dy (weight gradient), then
//             mi_deform_col2im : dcol, x, offsets -> d_offset[N,Ho,Wo,32] (bf16) and dx32[N,H,W,C] += dcol * corner weight
//             (fp32 atomics; mi_deform_zero_f32 clears it first), mi_deform_dx_finish : dx32 -> bf16 dx (* ReLU mask)
//             mi_deform_absmax : max |dcol|, from which col2im takes the grid that makes its atomic sums order-independent
// Layouts: bf16 NHWC, C a multiple of 32.  Offsets are read where the offset convolution wrote them: bf16 NHWC, pixel stride
// ldoff (32), 18 live channels; for tap t = i*3 + j channel 2t is the row offset and 2t + 1 the column offset.
// Sample point of output pixel (ho, wo), tap (i, j): h = ho*stride - 1 + i + off_h, w = wo*stride - 1 + j + off_w (pad 1, dil 1).
// It counts only if h > -1 && w > -1 && h < H && w < W; then the cell is floor(h), floor(h) + 1 (same for w), a corner outside
// [0, H-1] x [0, W-1] contributes zero, and everything is fp32.  Compiled with -ffp-contract=off: the tests compare exactly.
#include "common.h"

#define DC_TAPS 9
#define DC_OFF_LD 32      // pixel stride of d_offset (18 live channels + 14 zero)

// the sample of (pixel, tap): false when it does not count.  h0 in [-1, H-1], w0 in [-1, W-1] otherwise.  A NaN offset fails
// every comparison and so does not count either: no address is ever formed from it.
__device__ __forceinline__ bool dc_sample(const __bf16* __restrict__ offp, int t, int ho, int wo, int stride, int H, int W,
                                          int& h0, int& w0, float& lh, float& lw) {
  const float h = (float)(ho * stride - 1 + t / 3) + (float)offp[2 * t];
  const float w = (float)(wo * stride - 1 + t % 3) + (float)offp[2 * t + 1];
  if (!(h > -1.f && w > -1.f && h < (float)H && w < (float)W)) return false;
  const float hf = floorf(h), wf = floorf(w);
  h0 = (int)hf;
  w0 = (int)wf;
  lh = h - hf;
  lw = w - wf;
  return true;
}

// 8 lanes per (pixel, tap), 8 channels (16 bytes) per lane and pass: the offsets and the four weights once per lane, then a
// loop over its channel chunks.  Four corner rows of C contiguous channels each.
__global__ __launch_bounds__(256) void deform_im2col_kernel(const __bf16* __restrict__ x, int ldx, const __bf16* __restrict__ off,
                                                            int ldoff, __bf16* __restrict__ col, int N, int H, int W, int C8,
                                                            int Ho, int Wo, int stride) {
  const int64_t items = (int64_t)N * Ho * Wo * DC_TAPS;
  for (int64_t idx = blockIdx.x * 256LL + threadIdx.x; idx < items * 8; idx += (int64_t)gridDim.x * 256) {
    const int sub = (int)(idx & 7);
    const int64_t item = idx >> 3;
    const int t = (int)(item % DC_TAPS);
    const int64_t pix = item / DC_TAPS;
    const int wo = (int)(pix % Wo);
    const int ho = (int)((pix / Wo) % Ho);
    const int n = (int)(pix / ((int64_t)Wo * Ho));
    int h0 = 0, w0 = 0;
    float lh = 0.f, lw = 0.f;
    const bool ok = dc_sample(off + pix * ldoff, t, ho, wo, stride, H, W, h0, w0, lh, lw);
    __bf16* cp = col + item * (int64_t)(C8 * 8);
    if (!ok) {
      bf16x8 z;
#pragma unroll
      for (int e = 0; e < 8; ++e) z[e] = (__bf16)0.f;
      for (int c8 = sub; c8 < C8; c8 += 8) *(bf16x8*)(cp + c8 * 8) = z;
      continue;
    }
    const float hh = 1.f - lh, hw = 1.f - lw;
    const float w1 = hh * hw, w2 = hh * lw, w3 = lh * hw, w4 = lh * lw;
    const bool top = h0 >= 0, bot = h0 + 1 <= H - 1, lef = w0 >= 0, rig = w0 + 1 <= W - 1;
    const int64_t p1 = (((int64_t)n * H + h0) * W + w0) * ldx;      // (only dereferenced under its corner's flags)
    const int64_t p2 = p1 + ldx, p3 = p1 + (int64_t)W * ldx, p4 = p3 + ldx;
    for (int c8 = sub; c8 < C8; c8 += 8) {
      float v1[8], v2[8], v3[8], v4[8], o[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) v1[e] = v2[e] = v3[e] = v4[e] = 0.f;
      if (top && lef) unpack8(*(const bf16x8*)(x + p1 + c8 * 8), v1);
      if (top && rig) unpack8(*(const bf16x8*)(x + p2 + c8 * 8), v2);
      if (bot && lef) unpack8(*(const bf16x8*)(x + p3 + c8 * 8), v3);
      if (bot && rig) unpack8(*(const bf16x8*)(x + p4 + c8 * 8), v4);
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = ((w1 * v1[e] + w2 * v2[e]) + w3 * v3[e]) + w4 * v4[e];
      *(bf16x8*)(cp + c8 * 8) = pack8(o);
    }
  }
}

// one wave per (pixel, tap); lanes run along C, one channel per lane and pass: every float atomic wave-instruction covers up
// to 64 contiguous channels (256 bytes) of ONE corner row.  The coordinate gradients are reduced over C in fp32 (registers,
// then across the wave).  Corners outside the map or with zero weight are skipped.
__global__ __launch_bounds__(256) void deform_col2im_kernel(const __bf16* __restrict__ dcol, const __bf16* __restrict__ x, int ldx,
                                                            const __bf16* __restrict__ off, int ldoff, float* __restrict__ dx32,
                                                            __bf16* __restrict__ doff, const float* __restrict__ gmax, int N, int H,
                                                            int W, int C, int Ho, int Wo, int stride) {
  const int lane = threadIdx.x & 63;
  // Reproducible sums: float atomics arrive in any order, and fp32 addition is not associative - unless every addend is a
  // multiple of one power of two q and the sums stay below 2^24 q, where every addition is exact.  With m = max |dcol| <= 2^e,
  // q = 2^(e - 16): an addend |dcol * weight| <= 2^e is rounded to the grid by (p + M) - M, M = 1.5 * 2^23 q, and up to 256
  // addends of the largest magnitude sum exactly.  The rounding error, at most m * 2^-16 per addend, is far below the bf16
  // rounding dx gets afterwards.  gmax NULL, m zero, not finite or tiny: plain adds.
  float M = 0.f;
  if (gmax) {
    const float m = *gmax;
    int e = 0;
    if (m > 0.f && m < 3.0e38f) {
      frexpf(m, &e);
      if (e - 16 > -100) M = 1.5f * 8388608.f * ldexpf(1.f, e - 16);
    }
  }
  const bool grid = M > 0.f;
  const int64_t items = (int64_t)N * Ho * Wo * DC_TAPS;
  for (int64_t item = blockIdx.x * 4LL + (threadIdx.x >> 6); item < items; item += (int64_t)gridDim.x * 4) {
    const int t = (int)(item % DC_TAPS);
    const int64_t pix = item / DC_TAPS;
    const int wo = (int)(pix % Wo);
    const int ho = (int)((pix / Wo) % Ho);
    const int n = (int)(pix / ((int64_t)Wo * Ho));
    int h0 = 0, w0 = 0;
    float lh = 0.f, lw = 0.f;
    const bool ok = dc_sample(off + pix * ldoff, t, ho, wo, stride, H, W, h0, w0, lh, lw);      // (uniform over the wave)
    float gh = 0.f, gw = 0.f;
    if (ok) {
      const float hh = 1.f - lh, hw = 1.f - lw;
      const float w1 = hh * hw, w2 = hh * lw, w3 = lh * hw, w4 = lh * lw;
      const bool top = h0 >= 0, bot = h0 + 1 <= H - 1, lef = w0 >= 0, rig = w0 + 1 <= W - 1;
      const bool c1 = top && lef, c2 = top && rig, c3 = bot && lef, c4 = bot && rig;
      const int64_t q1 = ((int64_t)n * H + h0) * W + w0;             // (pixel index; only used under its corner's flags)
      const int64_t q2 = q1 + 1, q3 = q1 + W, q4 = q3 + 1;
      const __bf16* dc = dcol + item * (int64_t)C;
      for (int c = lane; c < C; c += 64) {
        const float g = (float)dc[c];
        const float v1 = c1 ? (float)x[q1 * ldx + c] : 0.f;
        const float v2 = c2 ? (float)x[q2 * ldx + c] : 0.f;
        const float v3 = c3 ? (float)x[q3 * ldx + c] : 0.f;
        const float v4 = c4 ? (float)x[q4 * ldx + c] : 0.f;
        gh += g * (hw * (v3 - v1) + lw * (v4 - v2));
        gw += g * (hh * (v2 - v1) + lh * (v4 - v3));
        float a1 = g * w1, a2 = g * w2, a3 = g * w3, a4 = g * w4;
        if (grid) {
          a1 = (a1 + M) - M;
          a2 = (a2 + M) - M;
          a3 = (a3 + M) - M;
          a4 = (a4 + M) - M;
        }
        if (c1 && w1 != 0.f) atomicAdd(dx32 + q1 * C + c, a1);
        if (c2 && w2 != 0.f) atomicAdd(dx32 + q2 * C + c, a2);
        if (c3 && w3 != 0.f) atomicAdd(dx32 + q3 * C + c, a3);
        if (c4 && w4 != 0.f) atomicAdd(dx32 + q4 * C + c, a4);
      }
    }
    gh = wave_sum(gh);
    gw = wave_sum(gw);
    __bf16* dp = doff + pix * DC_OFF_LD;
    if (lane == 0) {
      dp[2 * t] = (__bf16)gh;
      dp[2 * t + 1] = (__bf16)gw;
    }
    if (t == 0 && lane >= 2 * DC_TAPS && lane < DC_OFF_LD) dp[lane] = (__bf16)0.f;      // the 14 padding channels
  }
}

// out (zeroed by the caller) = max |v| over n8 * 8 bf16 values: non-negative floats order like their bit patterns, so the
// integer atomic maximum gives the same result in any order.  NaN is ignored (fmaxf).
__global__ __launch_bounds__(256) void deform_absmax_kernel(const __bf16* __restrict__ v, int64_t n8, float* __restrict__ out) {
  float m = 0.f;
  for (int64_t i = blockIdx.x * 256LL + threadIdx.x; i < n8; i += (int64_t)gridDim.x * 256) {
    const bf16x8 a = *(const bf16x8*)(v + i * 8);
#pragma unroll
    for (int e = 0; e < 8; ++e) m = fmaxf(m, fabsf((float)a[e]));
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  if ((threadIdx.x & 63) == 0) atomicMax((unsigned int*)out, __float_as_uint(m));
}

__global__ __launch_bounds__(256) void deform_zero_f32_kernel(float* __restrict__ p, int64_t n4) {
  const f32x4 z = {0.f, 0.f, 0.f, 0.f};
  for (int64_t i = blockIdx.x * 256LL + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) ((f32x4*)p)[i] = z;
}

// dx = bf16(dx32), zeroed where mask <= 0 (the bits of mi_ew_bf16 op 2 applied to the rounded value)
__global__ __launch_bounds__(256) void deform_dx_finish_kernel(const float* __restrict__ dx32, const __bf16* __restrict__ mask,
                                                               int ldmask, __bf16* __restrict__ dx, int lddx, int64_t npix, int C8) {
  const int64_t total = npix * C8;
  for (int64_t idx = blockIdx.x * 256LL + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
    const int c8 = (int)(idx % C8);
    const int64_t pix = idx / C8;
    const f32x4 a = *(const f32x4*)(dx32 + idx * 8), b = *(const f32x4*)(dx32 + idx * 8 + 4);
    const float f[8] = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
    bf16x8 out = pack8(f);
    if (mask) {
      const bf16x8 m = *(const bf16x8*)(mask + pix * ldmask + c8 * 8);
#pragma unroll
      for (int e = 0; e < 8; ++e)
        if (!((float)m[e] > 0.f)) out[e] = (__bf16)0.f;
    }
    *(bf16x8*)(dx + pix * lddx + c8 * 8) = out;
  }
}

static int dc_blocks(int64_t work, int per_block, int cap) {
  int64_t b = (work + per_block - 1) / per_block;
  if (b > cap) b = cap;
  if (b < 1) b = 1;
  return (int)b;
}

// the geometry this operator serves; everything else is refused before anything is launched
static int dc_geometry(const char* who, int N, int H, int W, int C, int stride, int pad, int dil) {
  MI_REQUIRE(stride == 1 || stride == 2, "%s: stride %d is not served (1 or 2)", who, stride);
  MI_REQUIRE(pad == 1, "%s: padding %d is not served (1)", who, pad);
  MI_REQUIRE(dil == 1, "%s: dilation %d is not served (1)", who, dil);
  MI_REQUIRE(N > 0 && H > 0 && W > 0 && C > 0, "%s: sizes N %d H %d W %d C %d must be positive", who, N, H, W, C);
  MI_REQUIRE(C % 32 == 0, "%s: C %d must be a multiple of 32", who, C);
  MI_REQUIRE((int64_t)N * H * W * C < (1LL << 40), "%s: map too large", who);
  return MI_OK;
}

extern "C" int mi_deform_im2col(const void* x, int ldx, const void* offset, int ldoff, void* col, int N, int H, int W, int C,
                                int stride, int pad, int dil, mi_stream_t st) {
  const int rc = dc_geometry("deform_im2col", N, H, W, C, stride, pad, dil);
  if (rc != MI_OK) return rc;
  MI_REQUIRE(x && offset && col, "deform_im2col: null pointer");
  MI_REQUIRE(ldx % 8 == 0 && ldx >= C, "deform_im2col: pixel stride ldx %d must be a multiple of 8 and >= C %d", ldx, C);
  MI_REQUIRE(ldoff >= 2 * DC_TAPS, "deform_im2col: offset pixel stride ldoff %d must be >= 18", ldoff);
  MI_REQUIRE(((uintptr_t)x & 15) == 0 && ((uintptr_t)col & 15) == 0 && ((uintptr_t)offset & 1) == 0,
             "deform_im2col: x / col must be 16-byte aligned (offset: 2)");
  const int Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
  const int64_t lanes = (int64_t)N * Ho * Wo * DC_TAPS * 8;
  hipLaunchKernelGGL(deform_im2col_kernel, dim3(dc_blocks(lanes, 256, 1 << 16)), dim3(256), 0, (hipStream_t)st, (const __bf16*)x,
                     ldx, (const __bf16*)offset, ldoff, (__bf16*)col, N, H, W, C / 8, Ho, Wo, stride);
  MI_CHECK_LAUNCH("deform_im2col");
  return MI_OK;
}

extern "C" int mi_deform_col2im(const void* dcol, const void* x, int ldx, const void* offset, int ldoff, float* dx32,
                                void* d_offset, const float* grid_max, int N, int H, int W, int C, int stride, int pad, int dil,
                                mi_stream_t st) {
  const int rc = dc_geometry("deform_col2im", N, H, W, C, stride, pad, dil);
  if (rc != MI_OK) return rc;
  MI_REQUIRE(dcol && x && offset && dx32 && d_offset, "deform_col2im: null pointer");
  MI_REQUIRE(ldx >= C, "deform_col2im: pixel stride ldx %d must be >= C %d", ldx, C);
  MI_REQUIRE(ldoff >= 2 * DC_TAPS, "deform_col2im: offset pixel stride ldoff %d must be >= 18", ldoff);
  MI_REQUIRE(((uintptr_t)dcol & 1) == 0 && ((uintptr_t)x & 1) == 0 && ((uintptr_t)offset & 1) == 0 && ((uintptr_t)d_offset & 1) == 0 &&
                 ((uintptr_t)dx32 & 3) == 0 && ((uintptr_t)grid_max & 3) == 0, "deform_col2im: misaligned pointer");
  const int Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
  const int64_t items = (int64_t)N * Ho * Wo * DC_TAPS;
  hipLaunchKernelGGL(deform_col2im_kernel, dim3(dc_blocks(items, 4, 1 << 18)), dim3(256), 0, (hipStream_t)st, (const __bf16*)dcol,
                     (const __bf16*)x, ldx, (const __bf16*)offset, ldoff, dx32, (__bf16*)d_offset, grid_max, N, H, W, C, Ho, Wo, stride);
  MI_CHECK_LAUNCH("deform_col2im");
  return MI_OK;
}

extern "C" int mi_deform_absmax(const void* v, int64_t n, float* out, mi_stream_t st) {
  MI_REQUIRE(v && out, "deform_absmax: null pointer");
  MI_REQUIRE(n > 0 && n % 8 == 0, "deform_absmax: count %lld must be a positive multiple of 8", (long long)n);
  MI_REQUIRE(((uintptr_t)v & 15) == 0 && ((uintptr_t)out & 3) == 0, "deform_absmax: v must be 16-byte aligned (out: 4)");
  hipLaunchKernelGGL(deform_absmax_kernel, dim3(dc_blocks(n / 8, 256, 2048)), dim3(256), 0, (hipStream_t)st, (const __bf16*)v, n / 8,
                     out);
  MI_CHECK_LAUNCH("deform_absmax");
  return MI_OK;
}

extern "C" int mi_deform_zero_f32(float* p, int64_t n, mi_stream_t st) {
  MI_REQUIRE(p, "deform_zero_f32: null pointer");
  MI_REQUIRE(n > 0 && n % 4 == 0, "deform_zero_f32: count %lld must be a positive multiple of 4", (long long)n);
  MI_REQUIRE(((uintptr_t)p & 15) == 0, "deform_zero_f32: pointer must be 16-byte aligned");
  hipLaunchKernelGGL(deform_zero_f32_kernel, dim3(dc_blocks(n / 4, 256, 4096)), dim3(256), 0, (hipStream_t)st, p, n / 4);
  MI_CHECK_LAUNCH("deform_zero_f32");
  return MI_OK;
}

extern "C" int mi_deform_dx_finish(const float* dx32, const void* mask, int ldmask, void* dx, int lddx, int64_t npix, int C,
                                   mi_stream_t st) {
  MI_REQUIRE(dx32 && dx, "deform_dx_finish: null pointer");
  MI_REQUIRE(npix > 0 && C > 0, "deform_dx_finish: sizes npix %lld C %d must be positive", (long long)npix, C);
  MI_REQUIRE(C % 8 == 0, "deform_dx_finish: C %d must be a multiple of 8", C);
  MI_REQUIRE(lddx % 8 == 0 && lddx >= C, "deform_dx_finish: pixel stride lddx %d must be a multiple of 8 and >= C %d", lddx, C);
  MI_REQUIRE(!mask || (ldmask % 8 == 0 && ldmask >= C), "deform_dx_finish: pixel stride ldmask %d must be a multiple of 8 and >= C %d",
             ldmask, C);
  MI_REQUIRE(((uintptr_t)dx32 & 15) == 0 && ((uintptr_t)dx & 15) == 0 && ((uintptr_t)mask & 15) == 0,
             "deform_dx_finish: pointers must be 16-byte aligned");
  hipLaunchKernelGGL(deform_dx_finish_kernel, dim3(dc_blocks(npix * (C / 8), 256, 4096)), dim3(256), 0, (hipStream_t)st, dx32,
                     (const __bf16*)mask, ldmask, (__bf16*)dx, lddx, npix, C / 8);
  MI_CHECK_LAUNCH("deform_dx_finish");
  return MI_OK;
}
