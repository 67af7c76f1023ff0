// ResNet-vd (timm resnet50d / resnet101d, the reference's build_resnet_vd_backbone): the 2x2 stride-2 average pool in front
// of a projection shortcut, nn.AvgPool2d(2, 2, ceil_mode=True, count_include_pad=False), on bf16 NHWC maps.  One work item
// per (pixel, 8 channels) on a grid-stride loop, 16-byte accesses: both passes are HBM-bound.
#include "common.h"

static int ew_blocks(int64_t total, int cap = 4096) {
  int64_t b = (total + 255) / 256;
  if (b > cap) b = cap;
  if (b < 1) b = 1;
  return (int)b;
}

// y[oy][ox] = (fp32 sum, row-major window order, of the 1, 2 or 4 inputs inside the map) / that count, one bf16 rounding
__global__ __launch_bounds__(256) void avgpool2x2s2_fwd_kernel(const __bf16* __restrict__ x, int ldx, __bf16* __restrict__ y,
                                                               int ldy, int N, int H, int W, int C8) {
  const int Ho = (H + 1) / 2, Wo = (W + 1) / 2;
  const int64_t total = (int64_t)N * Ho * Wo * C8;
  for (int64_t idx = blockIdx.x * 256LL + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
    const int c8 = (int)(idx % C8);
    int64_t r = idx / C8;
    const int ox = (int)(r % Wo); r /= Wo;
    const int oy = (int)(r % Ho);
    const int n = (int)(r / Ho);
    const int ny = (2 * oy + 1 < H) ? 2 : 1, nx = (2 * ox + 1 < W) ? 2 : 1;
    float acc[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = 0.f;
    for (int dy = 0; dy < ny; ++dy)
      for (int dx = 0; dx < nx; ++dx) {
        const bf16x8 v = *(const bf16x8*)(x + (((int64_t)n * H + 2 * oy + dy) * W + 2 * ox + dx) * ldx + c8 * 8);
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] += (float)v[e];
      }
    const float inv = 1.f / (float)(ny * nx);      // 1, 1/2 or 1/4: the product is the exact quotient
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] *= inv;
    *(bf16x8*)(y + (((int64_t)n * Ho + oy) * Wo + ox) * ldy + c8 * 8) = pack8(acc);
  }
}

// dx[iy][ix] (+)= dy[iy/2][ix/2] / count of that window; optionally zeroed where mask <= 0 (the ReLU gradient of the block
// input: the bits of mi_ew_bf16 op 2 applied to the rounded result).  Every pixel of dx is written.
__global__ __launch_bounds__(256) void avgpool2x2s2_bwd_kernel(const __bf16* __restrict__ dy, int lddy, __bf16* dx, int lddx,
                                                               const __bf16* __restrict__ mask, int ldmask, int accumulate,
                                                               int N, int H, int W, int C8) {
  const int Ho = (H + 1) / 2, Wo = (W + 1) / 2;
  const int64_t total = (int64_t)N * H * W * C8;
  for (int64_t idx = blockIdx.x * 256LL + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
    const int c8 = (int)(idx % C8);
    int64_t r = idx / C8;
    const int ix = (int)(r % W); r /= W;
    const int iy = (int)(r % H);
    const int n = (int)(r / H);
    const int oy = iy >> 1, ox = ix >> 1;
    const int ny = (2 * oy + 1 < H) ? 2 : 1, nx = (2 * ox + 1 < W) ? 2 : 1;
    const float inv = 1.f / (float)(ny * nx);
    const bf16x8 g = *(const bf16x8*)(dy + (((int64_t)n * Ho + oy) * Wo + ox) * lddy + c8 * 8);
    const int64_t pix = ((int64_t)n * H + iy) * W + ix;
    __bf16* dp = dx + pix * lddx + c8 * 8;
    float acc[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = (float)g[e] * inv;
    if (accumulate) {
      const bf16x8 o = *(const bf16x8*)dp;
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[e] += (float)o[e];
    }
    bf16x8 out = pack8(acc);
    if (mask) {
      const bf16x8 m = *(const bf16x8*)(mask + pix * ldmask + c8 * 8);
#pragma unroll
      for (int e = 0; e < 8; ++e)
        if (!((float)m[e] > 0.f)) out[e] = (__bf16)0.f;
    }
    *(bf16x8*)dp = out;
  }
}

extern "C" int mi_avgpool2x2s2_fwd(const void* x, int ldx, void* y, int ldy, int N, int H, int W, int C, mi_stream_t st) {
  MI_REQUIRE(x && y, "avgpool2x2s2_fwd: null pointer");
  MI_REQUIRE(N > 0 && H > 0 && W > 0 && C > 0, "avgpool2x2s2_fwd: sizes N %d H %d W %d C %d must be positive", N, H, W, C);
  MI_REQUIRE(C % 8 == 0, "avgpool2x2s2_fwd: C %d must be a multiple of 8", C);
  MI_REQUIRE(ldx % 8 == 0 && ldy % 8 == 0 && ldx >= C && ldy >= C,
             "avgpool2x2s2_fwd: pixel strides ldx %d / ldy %d must be multiples of 8 and >= C %d", ldx, ldy, C);
  MI_REQUIRE(((uintptr_t)x & 15) == 0 && ((uintptr_t)y & 15) == 0, "avgpool2x2s2_fwd: pointers must be 16-byte aligned");
  const int64_t total = (int64_t)N * ((H + 1) / 2) * ((W + 1) / 2) * (C / 8);
  hipLaunchKernelGGL(avgpool2x2s2_fwd_kernel, dim3(ew_blocks(total)), dim3(256), 0, (hipStream_t)st, (const __bf16*)x, ldx,
                     (__bf16*)y, ldy, N, H, W, C / 8);
  MI_CHECK_LAUNCH("avgpool2x2s2_fwd");
  return MI_OK;
}

extern "C" int mi_avgpool2x2s2_bwd(const void* dy, int lddy, void* dx, int lddx, const void* mask, int ldmask, int accumulate,
                                   int N, int H, int W, int C, mi_stream_t st) {
  MI_REQUIRE(dy && dx, "avgpool2x2s2_bwd: null pointer");
  MI_REQUIRE(N > 0 && H > 0 && W > 0 && C > 0, "avgpool2x2s2_bwd: sizes N %d H %d W %d C %d must be positive", N, H, W, C);
  MI_REQUIRE(C % 8 == 0, "avgpool2x2s2_bwd: C %d must be a multiple of 8", C);
  MI_REQUIRE(lddy % 8 == 0 && lddx % 8 == 0 && lddy >= C && lddx >= C,
             "avgpool2x2s2_bwd: pixel strides lddy %d / lddx %d must be multiples of 8 and >= C %d", lddy, lddx, C);
  MI_REQUIRE(!mask || (ldmask % 8 == 0 && ldmask >= C),
             "avgpool2x2s2_bwd: pixel stride ldmask %d must be a multiple of 8 and >= C %d", ldmask, C);
  MI_REQUIRE(((uintptr_t)dy & 15) == 0 && ((uintptr_t)dx & 15) == 0 && ((uintptr_t)mask & 15) == 0,
             "avgpool2x2s2_bwd: pointers must be 16-byte aligned");
  const int64_t total = (int64_t)N * H * W * (C / 8);
  hipLaunchKernelGGL(avgpool2x2s2_bwd_kernel, dim3(ew_blocks(total)), dim3(256), 0, (hipStream_t)st, (const __bf16*)dy, lddy,
                     (__bf16*)dx, lddx, (const __bf16*)mask, ldmask, accumulate, N, H, W, C / 8);
  MI_CHECK_LAUNCH("avgpool2x2s2_bwd");
  return MI_OK;
}
