// Grouped 3x3 convolution (padding 1, dilation 1, stride 1 or 2) with square groups of Cg in {8, 16, 24, 32} channels:
// forward, data gradient and weight gradient, each ONE launch over all groups (the weight gradient: one launch + its
// fixed-order split reduction).  The 3x3 of a RegNet X / Y block (group widths 8 / 16 / 24) and ResNeXt's 32x8d.
//
// The operator is bandwidth-sized (9 * Cg MACs per output element), so the form is: read the activation operand once into
// an LDS halo tile shared by the groups a block owns, keep the weights in registers, write the result once.
//
// Forward / data gradient (gconv_fwd_kernel) - v_mfma_f32_16x16x32_bf16 with A = weights (M = 16 output channels of ONE
// group), B = pixels (N = 16 consecutive output columns), K = (tap, input channel) in 8-channel octets:
//   * per group MT = ceil(Cg / 16) M tiles; rows >= Cg of the last tile carry zero weights and are not stored
//     (Cg = 8: half a tile, Cg = 24: one and a half - no tile ever straddles two groups, so no weight of another group,
//     no block-diagonal padding between groups, and no channel of another group is ever multiplied);
//   * K = 9 * Cg / 8 octets, padded to a multiple of 4 (one MFMA = 4 octets): 3 / 5 / 7 / 9 MFMAs per tile for
//     Cg = 8 / 16 / 24 / 32; the pad octets are zero in BOTH operands (the B side is a register zero, never an LDS read);
//   * a block = 256 threads = one pixel tile TH x 16 of one image x GB groups (GB in {1, 2, 4}, <= 64 channels); wave w
//     owns group w % GB and the pixel rows w / GB, w / GB + 4 / GB, ...; its weight fragments (MT * NK * 4 VGPRs) are
//     loaded once from the packed image, whose layout IS the fragment order (one 16-byte load per lane and fragment);
//   * the halo tile is octet-major in LDS: [octet][halo pixel] of 16-byte vectors, so the 16 lanes of a B fragment read
//     consecutive vectors (stride 1) or every second one (stride 2);
//   * the accumulator leaves as 4 consecutive channels per lane: one 8-byte store, fp32 bias added before the rounding.
// The data gradient is the same kernel on the out-gradient with the data-gradient image (taps mirrored, channel roles
// swapped).  For stride 2 the halo tile holds the out-gradient zero-upsampled by 2 (odd virtual rows / columns are zero):
// every pixel of dx is then one stride-1 gather and is written by the launch, also where no tap reaches.
//
// Weight gradient (gconv_wgrad_kernel) - the same MFMA with K = pixels: A = dy (M = 16 output channels), B = x shifted by
// the tap (N = 16 input channels), one accumulator per (tap, input-channel tile).  Both operands need 8 consecutive PIXELS
// of one channel per lane, so the tiles are transposed while they are filled: LDS holds [channel][pixel] (for stride 2 the
// x rows are split into an even and an odd column plane, which makes every tap's 8 pixels contiguous again).  A block
// walks a fixed range of pixel tiles with the sums in registers and writes ONE partial [C][Cg][9] (+ [C] column sums of dy
// for the bias gradient, an extra MFMA against a vector of ones); gconv_wgrad_reduce_kernel adds the partials in a fixed
// order.  No atomics anywhere: the bits do not depend on scheduling.
#include "common.h"

namespace {

constexpr int GC_THREADS = 256;
constexpr int GC_MAX_CH = 64;      // channels a block owns

__host__ __device__ constexpr int gc_mt(int cg) { return (cg + 15) / 16; }
__host__ __device__ constexpr int gc_nk(int cg) { return (9 * cg / 8 + 3) / 4; }

__device__ __forceinline__ bf16x8 gc_zero8() {
  bf16x8 z;
#pragma unroll
  for (int e = 0; e < 8; ++e) z[e] = (__bf16)0.f;
  return z;
}

// groups per block: as many as fit GC_MAX_CH channels and four waves, not more than the layer has
int gc_groups_per_block(int Cg, int G) {
  int gb = GC_MAX_CH / Cg >= 4 ? 4 : 2;
  while (gb > 1 && gb / 2 >= G) gb /= 2;
  return gb;
}

// ------------------------------------------------------------------------------------------------ weight images
// image[g][mt][m][lane][j] (bf16) = the A fragment of lane `lane` for M tile mt, k-step m of group g:
//   row  = mt * 16 + (lane & 15), octet q = 4 * m + (lane >> 4), tap t = q / (Cg / 8), channel k = (q % (Cg / 8)) * 8 + j
//   forward image:       w[g * Cg + row][k][t / 3][t % 3]
//   data-gradient image: w[g * Cg + k][row][2 - t / 3][2 - t % 3]
//   zero where row >= Cg or q >= 9 * Cg / 8
__global__ __launch_bounds__(256) void gconv_pack_kernel(const float* __restrict__ w, __bf16* __restrict__ wf,
                                                         __bf16* __restrict__ wd, int G, int Cg) {
  const int MT = gc_mt(Cg), NK = gc_nk(Cg), OPT = Cg / 8, KO = 9 * OPT;
  const int64_t total = (int64_t)G * MT * NK * 64 * 8;
  for (int64_t i = blockIdx.x * 256LL + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int j = (int)(i & 7), lane = (int)((i >> 3) & 63);
    int64_t rest = i >> 9;
    const int m = (int)(rest % NK);
    rest /= NK;
    const int mt = (int)(rest % MT);
    const int g = (int)(rest / MT);
    const int row = mt * 16 + (lane & 15), q = 4 * m + (lane >> 4);
    float vf = 0.f, vd = 0.f;
    if (row < Cg && q < KO) {
      const int t = q / OPT, k = (q % OPT) * 8 + j;
      vf = w[((int64_t)(g * Cg + row) * Cg + k) * 9 + t];
      vd = w[((int64_t)(g * Cg + k) * Cg + row) * 9 + (8 - t)];
    }
    if (wf) wf[i] = f2bf(vf);
    if (wd) wd[i] = f2bf(vd);
  }
}

// ------------------------------------------------------------------------------------------------ forward / data gradient
struct GcArgs {
  const __bf16* x;    // the tensor that is read: [N][IH][IW] pixels of ldx elements
  const __bf16* w;    // packed image
  __bf16* y;          // the tensor that is written: [N][OH][OW] pixels of ldy elements
  const float* bias;
  int ldx, ldy, IH, IW, OH, OW;
  int s;              // output pixel -> virtual input pixel stride
  int up;             // 1, or 2: virtual input pixel (vy, vx) is input pixel (vy / 2, vx / 2) when both are even, else zero
  int G, GB, TH, tilesX;
};

template <int CG>
__global__ __launch_bounds__(GC_THREADS) void gconv_fwd_kernel(GcArgs a) {
  constexpr int OPT = CG / 8, KO = 9 * OPT, NK = gc_nk(CG), MT = gc_mt(CG);
  extern __shared__ __attribute__((aligned(16))) unsigned char gc_smem[];
  bf16x8* tile = (bf16x8*)gc_smem;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tx = blockIdx.x % a.tilesX, ty = blockIdx.x / a.tilesX, n = blockIdx.z;
  const int oy0 = ty * a.TH, ox0 = tx * 16;
  const int HWc = 15 * a.s + 3, HHc = (a.TH - 1) * a.s + 3;
  const int NPIX = HHc * HWc, NP = NPIX | 1;
  const int g0 = blockIdx.y * a.GB;
  const int ng = min(a.GB, a.G - g0);
  const int NOCT = ng * OPT;
  const bf16x8 zero = gc_zero8();
  {
    const __bf16* xb = a.x + (int64_t)n * a.IH * a.IW * a.ldx + g0 * CG;
    for (int i = tid; i < NPIX * NOCT; i += GC_THREADS) {
      const int oct = i % NOCT, pix = i / NOCT;
      const int hy = pix / HWc, hx = pix - hy * HWc;
      int iy = oy0 * a.s - 1 + hy, ix = ox0 * a.s - 1 + hx;
      bool ok = iy >= 0 && ix >= 0;
      if (a.up == 2) {
        ok = ok && !((iy | ix) & 1);
        iy >>= 1;
        ix >>= 1;
      }
      bf16x8 v = zero;
      if (ok && iy < a.IH && ix < a.IW) v = *(const bf16x8*)(xb + ((int64_t)iy * a.IW + ix) * a.ldx + oct * 8);
      tile[oct * NP + pix] = v;
    }
  }
  __syncthreads();
  const int gi = wave % a.GB, part = wave / a.GB, nparts = 4 / a.GB;
  if (gi >= ng) return;      // (no barrier follows)
  const int g = g0 + gi;
  bf16x8 wa[MT][NK];
  {
    const bf16x8* wimg = (const bf16x8*)a.w + (int64_t)g * MT * NK * 64 + lane;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int m = 0; m < NK; ++m) wa[mt][m] = wimg[(mt * NK + m) * 64];
  }
  int off[NK];
#pragma unroll
  for (int m = 0; m < NK; ++m) {
    const int q = 4 * m + (lane >> 4);
    const int t = q / OPT, cio = q % OPT;
    off[m] = q < KO ? (gi * OPT + cio) * NP + (t / 3) * HWc + (t % 3) + (lane & 15) * a.s : -1;
  }
  const int ox = ox0 + (lane & 15), co4 = (lane >> 4) * 4;
  for (int pr = part; pr < a.TH; pr += nparts) {
    const int oy = oy0 + pr;
    if (oy >= a.OH) break;
    const int rowoff = pr * a.s * HWc;
    f32x4 acc[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) acc[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int m = 0; m < NK; ++m) {
      const bf16x8 b = off[m] >= 0 ? tile[off[m] + rowoff] : zero;
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) acc[mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wa[mt][m], b, acc[mt], 0, 0, 0);
    }
    if (ox < a.OW) {
      __bf16* yp = a.y + (((int64_t)n * a.OH + oy) * a.OW + ox) * a.ldy + g * CG;
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        const int co = mt * 16 + co4;
        if (co < CG) {
          f32x4 v = acc[mt];
          if (a.bias) {
            const f32x4 b4 = *(const f32x4*)(a.bias + g * CG + co);
            v += b4;
          }
          bf16x4 o;
#pragma unroll
          for (int e = 0; e < 4; ++e) o[e] = f2bf(v[e]);
          *(bf16x4*)(yp + co) = o;
        }
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------ weight gradient
struct GwArgs {
  const __bf16* x;
  const __bf16* dy;
  float* ws;          // [nsplit][C * Cg * 9 + C]
  int ldx, ldy, N, H, W, OH, OW, st;
  int G, GB, TW, TH, tilesX, tilesY, ntiles, nsplit, want_bias;
  int XR, RP, PW, CS, DS;   // x^T rows, row pitch, plane width (stride 2), channel strides of x^T / dy^T (elements)
};

template <int CG>
__global__ __launch_bounds__(GC_THREADS) void gconv_wgrad_kernel(GwArgs a) {
  constexpr int OPT = CG / 8, MT = gc_mt(CG);
  extern __shared__ __attribute__((aligned(16))) unsigned char gc_smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int split = blockIdx.x;
  const int g0 = blockIdx.y * a.GB;
  const int ng = min(a.GB, a.G - g0);
  const int NOCT = ng * OPT;
  __bf16* xT = (__bf16*)gc_smem;
  __bf16* dyT = xT + a.GB * CG * a.CS;       // (CS is a multiple of 8 elements + 2: the host keeps dyT 16-byte aligned)
  const int gi = wave / MT, mtc = wave % MT;
  const bool active = gi < ng;                // (inactive waves still fill and meet every barrier)
  const int arow = mtc * 16 + (lane & 15);
  const bool a_ok = arow < CG;
  const bf16x8 zero = gc_zero8();
  bf16x8 ones;
#pragma unroll
  for (int e = 0; e < 8; ++e) ones[e] = (__bf16)1.f;
  f32x4 acc[9][MT];
  f32x4 accb = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int mtn = 0; mtn < MT; ++mtn) acc[t][mtn] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int XC = (a.TW - 1) * a.st + 3, NXP = a.XR * XC, NDP = a.TH * a.TW;
  const int octw = a.TW / 8, nks = NDP / 32;
  const int t0 = (int)((int64_t)split * a.ntiles / a.nsplit), t1 = (int)((int64_t)(split + 1) * a.ntiles / a.nsplit);
  for (int tile = t0; tile < t1; ++tile) {
    const int tx = tile % a.tilesX, ty = (tile / a.tilesX) % a.tilesY, n = tile / (a.tilesX * a.tilesY);
    __syncthreads();      // the previous tile has been consumed
    {
      const __bf16* xb = a.x + (int64_t)n * a.H * a.W * a.ldx + g0 * CG;
      const int iy0 = ty * a.TH * a.st - 1, ix0 = tx * a.TW * a.st - 1;
      for (int i = tid; i < NXP * NOCT; i += GC_THREADS) {
        const int oct = i % NOCT, pix = i / NOCT;
        const int hy = pix / XC, hx = pix - hy * XC;
        const int iy = iy0 + hy, ix = ix0 + hx;
        bf16x8 v = zero;
        if (iy >= 0 && ix >= 0 && iy < a.H && ix < a.W) v = *(const bf16x8*)(xb + ((int64_t)iy * a.W + ix) * a.ldx + oct * 8);
        const int pos = hy * a.RP + (a.st == 2 ? (hx & 1) * a.PW + (hx >> 1) : hx);
#pragma unroll
        for (int e = 0; e < 8; ++e) xT[(oct * 8 + e) * a.CS + pos] = v[e];
      }
      const __bf16* db = a.dy + (int64_t)n * a.OH * a.OW * a.ldy + g0 * CG;
      const int oy0 = ty * a.TH, ox0 = tx * a.TW;
      for (int i = tid; i < NDP * NOCT; i += GC_THREADS) {
        const int oct = i % NOCT, pix = i / NOCT;
        const int py = pix / a.TW, px = pix - py * a.TW;
        const int oy = oy0 + py, ox = ox0 + px;
        bf16x8 v = zero;
        if (oy < a.OH && ox < a.OW) v = *(const bf16x8*)(db + ((int64_t)oy * a.OW + ox) * a.ldy + oct * 8);
#pragma unroll
        for (int e = 0; e < 8; ++e) dyT[(oct * 8 + e) * a.DS + pix] = v[e];
      }
    }
    __syncthreads();
    if (!active) continue;
    for (int kk = 0; kk < nks; ++kk) {
      const int q = 4 * kk + (lane >> 4);
      const int pr = q / octw, col0 = (q - pr * octw) * 8;
      const bf16x8 av = a_ok ? *(const bf16x8*)(dyT + (gi * CG + arow) * a.DS + q * 8) : zero;
      if (a.want_bias) accb = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av, ones, accb, 0, 0, 0);
#pragma unroll
      for (int t = 0; t < 9; ++t) {
        const int r = t / 3, c = t % 3;
        const int pos = (pr * a.st + r) * a.RP + (a.st == 2 ? (c & 1) * a.PW + col0 + (c >> 1) : col0 + c);
#pragma unroll
        for (int mtn = 0; mtn < MT; ++mtn) {
          const int brow = mtn * 16 + (lane & 15);
          bf16x8 bv = zero;
          if (brow < CG) __builtin_memcpy(&bv, xT + (gi * CG + brow) * a.CS + pos, 16);      // (2-byte aligned: the tap shift)
          acc[t][mtn] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av, bv, acc[t][mtn], 0, 0, 0);
        }
      }
    }
  }
  if (!active) return;
  const int C = a.G * CG, g = g0 + gi;
  float* part = a.ws + (int64_t)split * ((int64_t)C * CG * 9 + C);
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int co = mtc * 16 + (lane >> 4) * 4 + e;
    if (co >= CG) continue;
#pragma unroll
    for (int mtn = 0; mtn < MT; ++mtn) {
      const int ci = mtn * 16 + (lane & 15);
      if (ci >= CG) continue;
      float* p = part + ((int64_t)(g * CG + co) * CG + ci) * 9;
#pragma unroll
      for (int t = 0; t < 9; ++t) p[t] = acc[t][mtn][e];
    }
    if (a.want_bias && (lane & 15) == 0) part[(int64_t)C * CG * 9 + g * CG + co] = accb[e];
  }
}

// gw[i] = sum over the split partials in a FIXED order: slice k of GR_S adds splits k, k + GR_S, ... in rising order, then the
// slices are added in rising order (a thread per (element, slice): a single thread per element walks nsplit dependent
// loads - measured 176 us at 512 splits).  The last C entries of a partial are the column sums of dy.
constexpr int GR_E = 32, GR_S = 8;
__global__ __launch_bounds__(GR_E * GR_S) void gconv_wgrad_reduce_kernel(const float* __restrict__ ws, float* __restrict__ gw,
                                                                       float* __restrict__ gbias, int64_t nw, int C, int nsplit) {
  __shared__ float part[GR_S][GR_E];
  const int e = threadIdx.x % GR_E, k = threadIdx.x / GR_E;
  const int64_t per = nw + C, n = nw + (gbias ? C : 0);
  const int64_t i = blockIdx.x * (int64_t)GR_E + e;
  float sacc = 0.f;
  if (i < n) {
#pragma unroll 8
    for (int sp = k; sp < nsplit; sp += GR_S) sacc += ws[sp * per + i];
  }
  part[k][e] = sacc;
  __syncthreads();
  if (k == 0 && i < n) {
    float t = part[0][e];
#pragma unroll
    for (int j = 1; j < GR_S; ++j) t += part[j][e];
    if (i < nw) gw[i] = t;
    else gbias[i - nw] = t;
  }
}

// ------------------------------------------------------------------------------------------------ host side
struct GcGeo {
  int Cg, C, Ho, Wo;
};

// geometry first (the offending quantity by name), then sizes, strides, pointers
int gc_check_geometry(const mi_gconv_desc* d, const char* who, GcGeo* o) {
  MI_REQUIRE(d != nullptr, "%s: null descriptor", who);
  MI_REQUIRE(d->kh == 3 && d->kw == 3, "%s: kernel size %dx%d not served (3x3 only)", who, d->kh, d->kw);
  MI_REQUIRE(d->stride == 1 || d->stride == 2, "%s: stride %d not served (1 or 2)", who, d->stride);
  MI_REQUIRE(d->padding == 1, "%s: padding %d not served (1 only)", who, d->padding);
  MI_REQUIRE(d->dilation == 1, "%s: dilation %d not served (1 only)", who, d->dilation);
  MI_REQUIRE(d->G > 0 && d->Cin > 0 && d->Cout > 0, "%s: groups / channel counts must be positive (G %d Cin %d Cout %d)", who,
             d->G, d->Cin, d->Cout);
  MI_REQUIRE(d->Cin % d->G == 0 && d->Cout % d->G == 0, "%s: channels are not G * Cg (Cin %d Cout %d G %d)", who, d->Cin, d->Cout,
             d->G);
  MI_REQUIRE(d->Cin == d->Cout, "%s: groups are not square: Cin / G = %d, Cout / G = %d", who, d->Cin / d->G, d->Cout / d->G);
  const int Cg = d->Cin / d->G;
  MI_REQUIRE(Cg == 8 || Cg == 16 || Cg == 24 || Cg == 32, "%s: group width Cg %d not served (8, 16, 24, 32)", who, Cg);
  MI_REQUIRE(d->N > 0 && d->H > 0 && d->W > 0, "%s: N, H, W must be positive (%d %d %d)", who, d->N, d->H, d->W);
  MI_REQUIRE(d->N <= 65535 && d->G <= 65535, "%s: N / G beyond the grid (%d %d)", who, d->N, d->G);
  o->Cg = Cg;
  o->C = d->Cin;
  o->Ho = (d->H - 1) / d->stride + 1;
  o->Wo = (d->W - 1) / d->stride + 1;
  return MI_OK;
}

int gc_check_views(const mi_gconv_desc* d, const char* who, const GcGeo& o) {
  MI_REQUIRE(d->ldx >= o.C, "%s: ldx %d < C %d", who, d->ldx, o.C);
  MI_REQUIRE(d->ldy >= o.C, "%s: ldy %d < C %d", who, d->ldy, o.C);
  MI_REQUIRE(d->ldx % 8 == 0 && d->ldy % 8 == 0, "%s: pixel strides must be a multiple of 8 (ldx %d ldy %d)", who, d->ldx, d->ldy);
  MI_REQUIRE(d->x != nullptr && d->y != nullptr, "%s: null x / y", who);
  MI_REQUIRE(((uintptr_t)d->x & 15) == 0 && ((uintptr_t)d->y & 15) == 0, "%s: x / y not 16-byte aligned", who);
  return MI_OK;
}

template <int CG>
int gc_launch_fwd(const GcArgs& a, int N, int lds, hipStream_t st) {
  static bool attr = false;
  if (!attr) {
    hipFuncSetAttribute((const void*)gconv_fwd_kernel<CG>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    attr = true;
  }
  const dim3 grid(a.tilesX * mi_cdiv(a.OH, a.TH), mi_cdiv(a.G, a.GB), N);
  hipLaunchKernelGGL(gconv_fwd_kernel<CG>, grid, dim3(GC_THREADS), lds, st, a);
  MI_CHECK_LAUNCH("gconv_fwd_kernel");
  return MI_OK;
}

int gc_run_fwd(GcArgs a, int Cg, int N, mi_stream_t s) {
  a.GB = gc_groups_per_block(Cg, a.G);
  a.TH = a.s == 1 ? 8 : 4;
  a.tilesX = mi_cdiv(a.OW, 16);
  MI_REQUIRE((int64_t)a.tilesX * mi_cdiv(a.OH, a.TH) < (1LL << 31), "gconv: too many pixel tiles");
  const int npix = ((a.TH - 1) * a.s + 3) * (15 * a.s + 3);
  const int lds = a.GB * (Cg / 8) * (npix | 1) * 16;
  hipStream_t st = (hipStream_t)s;
  switch (Cg) {
    case 8: return gc_launch_fwd<8>(a, N, lds, st);
    case 16: return gc_launch_fwd<16>(a, N, lds, st);
    case 24: return gc_launch_fwd<24>(a, N, lds, st);
    default: return gc_launch_fwd<32>(a, N, lds, st);
  }
}

// the weight gradient's launch record (pointers may be unset); returns the LDS bytes
int gc_wgrad_fill(const mi_gconv_desc* d, const GcGeo& o, GwArgs* a) {
  a->ldx = d->ldx, a->ldy = d->ldy, a->N = d->N, a->H = d->H, a->W = d->W, a->OH = o.Ho, a->OW = o.Wo, a->st = d->stride;
  a->G = d->G;
  a->GB = o.Cg >= 24 ? 2 : 4;      // GB * MT == 4 waves
  int tw = 32;                     // the tile width that wastes the fewest columns (ties: the wider one)
  for (int c : {16, 8})
    if (mi_cdiv(o.Wo, c) * c < mi_cdiv(o.Wo, tw) * tw) tw = c;
  a->TW = tw;
  a->TH = (d->stride == 1 ? 256 : 128) / tw;
  a->tilesX = mi_cdiv(o.Wo, a->TW), a->tilesY = mi_cdiv(o.Ho, a->TH);
  const int64_t nt = (int64_t)d->N * a->tilesX * a->tilesY;
  if (nt >= (1LL << 31)) return -1;
  a->ntiles = (int)nt;
  const int chunks = mi_cdiv(d->G, a->GB);
  int ns = mi_cdiv(512, chunks);
  a->nsplit = ns < a->ntiles ? ns : a->ntiles;
  a->XR = (a->TH - 1) * a->st + 3;
  a->PW = a->TW + 2;
  a->RP = a->st == 2 ? 2 * a->PW : a->TW + 2;
  auto odd8 = [](int n) { int c = (n + 7) / 8; return (c | 1) * 8; };
  a->CS = odd8(a->XR * a->RP) + 2;
  a->DS = odd8(a->TH * a->TW + 8);
  // x^T then dy^T; dy^T starts 16-byte aligned: GB * Cg * CS * 2 bytes with GB * Cg a multiple of 8 and CS even
  return (a->GB * o.Cg * a->CS + a->GB * o.Cg * a->DS) * 2;
}

template <int CG>
int gc_launch_wgrad(const GwArgs& a, int lds, hipStream_t st) {
  static bool attr = false;
  if (!attr) {
    hipFuncSetAttribute((const void*)gconv_wgrad_kernel<CG>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    attr = true;
  }
  hipLaunchKernelGGL(gconv_wgrad_kernel<CG>, dim3(a.nsplit, mi_cdiv(a.G, a.GB)), dim3(GC_THREADS), lds, st, a);
  MI_CHECK_LAUNCH("gconv_wgrad_kernel");
  return MI_OK;
}

}  // namespace

extern "C" int mi_gconv_desc_size(void) { return (int)sizeof(mi_gconv_desc); }

extern "C" int64_t mi_gconv_weight_image_bytes(int C, int Cg) {
  MI_REQUIRE(Cg == 8 || Cg == 16 || Cg == 24 || Cg == 32, "mi_gconv_weight_image_bytes: group width Cg %d not served (8, 16, 24, 32)", Cg);
  MI_REQUIRE(C > 0 && C % Cg == 0, "mi_gconv_weight_image_bytes: C %d is not a positive multiple of Cg %d", C, Cg);
  return (int64_t)(C / Cg) * gc_mt(Cg) * gc_nk(Cg) * 64 * 8 * 2;
}

extern "C" int mi_gconv_pack_weight(const float* w, int C, int Cg, void* wf, void* wd, mi_stream_t s) {
  MI_REQUIRE(Cg == 8 || Cg == 16 || Cg == 24 || Cg == 32, "mi_gconv_pack_weight: group width Cg %d not served (8, 16, 24, 32)", Cg);
  MI_REQUIRE(C > 0 && C % Cg == 0, "mi_gconv_pack_weight: C %d is not a positive multiple of Cg %d", C, Cg);
  MI_REQUIRE(w != nullptr && (wf != nullptr || wd != nullptr), "mi_gconv_pack_weight: null weight / no image asked for");
  MI_REQUIRE(((uintptr_t)w & 3) == 0 && ((uintptr_t)wf & 15) == 0 && ((uintptr_t)wd & 15) == 0, "mi_gconv_pack_weight: misaligned pointer");
  const int G = C / Cg;
  const int64_t total = (int64_t)G * gc_mt(Cg) * gc_nk(Cg) * 64 * 8;
  const int blocks = (int)(mi_cdiv64(total, 256) < 4096 ? mi_cdiv64(total, 256) : 4096);
  hipLaunchKernelGGL(gconv_pack_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)s, w, (__bf16*)wf, (__bf16*)wd, G, Cg);
  MI_CHECK_LAUNCH("gconv_pack_kernel");
  return MI_OK;
}

extern "C" int mi_gconv_fwd(const mi_gconv_desc* d, mi_stream_t s) {
  GcGeo o;
  if (int rc = gc_check_geometry(d, "mi_gconv_fwd", &o)) return rc;
  if (int rc = gc_check_views(d, "mi_gconv_fwd", o)) return rc;
  MI_REQUIRE(d->w != nullptr, "mi_gconv_fwd: null weight image");
  MI_REQUIRE(((uintptr_t)d->w & 15) == 0 && ((uintptr_t)d->bias & 15) == 0, "mi_gconv_fwd: weight image / bias not 16-byte aligned");
  GcArgs a{};
  a.x = (const __bf16*)d->x, a.w = (const __bf16*)d->w, a.y = (__bf16*)d->y, a.bias = d->bias;
  a.ldx = d->ldx, a.ldy = d->ldy, a.IH = d->H, a.IW = d->W, a.OH = o.Ho, a.OW = o.Wo, a.s = d->stride, a.up = 1, a.G = d->G;
  return gc_run_fwd(a, o.Cg, d->N, s);
}

extern "C" int mi_gconv_dgrad(const mi_gconv_desc* d, mi_stream_t s) {
  GcGeo o;
  if (int rc = gc_check_geometry(d, "mi_gconv_dgrad", &o)) return rc;
  if (int rc = gc_check_views(d, "mi_gconv_dgrad", o)) return rc;
  MI_REQUIRE(d->w != nullptr, "mi_gconv_dgrad: null weight image");
  MI_REQUIRE(((uintptr_t)d->w & 15) == 0, "mi_gconv_dgrad: weight image not 16-byte aligned");
  GcArgs a{};
  a.x = (const __bf16*)d->y, a.w = (const __bf16*)d->w, a.y = (__bf16*)d->x, a.bias = nullptr;
  a.ldx = d->ldy, a.ldy = d->ldx, a.IH = o.Ho, a.IW = o.Wo, a.OH = d->H, a.OW = d->W, a.s = 1, a.up = d->stride, a.G = d->G;
  return gc_run_fwd(a, o.Cg, d->N, s);
}

extern "C" int64_t mi_gconv_wgrad_plan(const mi_gconv_desc* d, int32_t* nsplit) {
  GcGeo o;
  if (int rc = gc_check_geometry(d, "mi_gconv_wgrad_plan", &o)) return rc;
  GwArgs a{};
  MI_REQUIRE(gc_wgrad_fill(d, o, &a) > 0, "mi_gconv_wgrad_plan: too many pixel tiles");
  if (nsplit) *nsplit = a.nsplit;
  return (int64_t)a.nsplit * ((int64_t)o.C * o.Cg * 9 + o.C) * 4;
}

extern "C" int mi_gconv_wgrad(const mi_gconv_desc* d, mi_stream_t s) {
  GcGeo o;
  if (int rc = gc_check_geometry(d, "mi_gconv_wgrad", &o)) return rc;
  if (int rc = gc_check_views(d, "mi_gconv_wgrad", o)) return rc;
  MI_REQUIRE(d->gw != nullptr && d->ws != nullptr, "mi_gconv_wgrad: null gw / workspace");
  MI_REQUIRE(((uintptr_t)d->gw & 3) == 0 && ((uintptr_t)d->gbias & 3) == 0 && ((uintptr_t)d->ws & 15) == 0,
             "mi_gconv_wgrad: gw / gbias / workspace misaligned");
  GwArgs a{};
  const int lds = gc_wgrad_fill(d, o, &a);
  MI_REQUIRE(lds > 0, "mi_gconv_wgrad: too many pixel tiles");
  MI_REQUIRE(lds <= 160 * 1024, "mi_gconv_wgrad: LDS %d too large", lds);
  const int64_t nw = (int64_t)o.C * o.Cg * 9;
  const int64_t need = (int64_t)a.nsplit * (nw + o.C) * 4;
  MI_REQUIRE(d->ws_bytes >= need, "mi_gconv_wgrad: workspace %lld bytes < %lld (mi_gconv_wgrad_plan)", (long long)d->ws_bytes,
             (long long)need);
  a.x = (const __bf16*)d->x, a.dy = (const __bf16*)d->y, a.ws = (float*)d->ws, a.want_bias = d->gbias != nullptr;
  hipStream_t st = (hipStream_t)s;
  int rc;
  switch (o.Cg) {
    case 8: rc = gc_launch_wgrad<8>(a, lds, st); break;
    case 16: rc = gc_launch_wgrad<16>(a, lds, st); break;
    case 24: rc = gc_launch_wgrad<24>(a, lds, st); break;
    default: rc = gc_launch_wgrad<32>(a, lds, st); break;
  }
  if (rc) return rc;
  const int64_t n = nw + (d->gbias ? o.C : 0);
  hipLaunchKernelGGL(gconv_wgrad_reduce_kernel, dim3((unsigned)mi_cdiv64(n, GR_E)), dim3(GR_E * GR_S), 0, st, (const float*)d->ws, d->gw,
                     d->gbias, nw, o.C, a.nsplit);
  MI_CHECK_LAUNCH("gconv_wgrad_reduce_kernel");
  return MI_OK;
}
