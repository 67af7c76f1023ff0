// The inference step and the box head tail of the focal DETR family (SMCA-DETR, Anchor DETR).
//
// mi_focal_topk_postprocess replaces SMCADetr.inference (meta_arch/smca_detr.py:216-264) followed by detector_postprocess, and
// PostProcess of anchor_detr.py: sigmoid over all Q x C logits of an image, the best K of them, their boxes gathered, converted
// and scaled - about a dozen torch calls plus a Python loop per image there, ONE launch for the batch here.
//   One block of 1024 threads per image.  The sigmoid is monotonic, so the selection runs on an order-preserving 32-bit key of
//   the logit (NaN greatest, -0 == +0) and the sigmoid is taken of the K winners only:
//     1. radix select, four 8-bit passes from the top: per-wave LDS histograms (integer counts: the order of their atomic
//        increments cannot show), a 256-bin descending scan by one wave -> the K-th key T, #keys > T, #ties to take;
//     2. compaction in index order without atomics: per (row, wave) ballot counts, one scan, ballot ranks -> the keys > T, then
//        the lowest-index ties, as (key << 32 | ~index) words in LDS;
//     3. the K words are distinct, so each one's output position is the number of larger words (rank by counting: one barrier;
//        a bitonic network of the next power of two is 28 barriers at K = 100 for the same result);
//     4. the K winners read their logit and box again and write score / label / query / box.
//   The keys stay in registers across the passes while Q * C <= 27 * 1024 (300 x 91 = 27 300 does); above that every pass
//   re-reads the logits (L2).  The result is a pure function of the inputs: bit-reproducible, capturable.
//   Built without fma contraction: tests/topk_ref.py restates the box arithmetic in numpy bit for bit.
//
// mi_box_ref_sigmoid_fwd / _bwd: y = sigmoid(x + (px, py, 0, 0)) of the SMCA box head (smca_detr.py:500-503: slice add of the
// decoder's reference points repeated over the levels, then sigmoid) and its backward, dp summed over the levels in a fixed
// order by one thread per (image, query).  The sigmoid and y (1 - y) are evaluated in fp64 from x + p and rounded once.
#include "common.h"

#define TK_THREADS 1024
#define TK_WAVES 16
#define TK_ITEMS 27      // keys per thread held in registers: 27 * 1024 = 27 648 >= 300 * 91
#define TK_MAXK 1024

struct TopkK {
  const float* logits;     // [B][Q][C]
  const float* boxes;      // [B][Q][4] cxcywh
  const int64_t* sizes;    // [B][2] (h, w)
  const int64_t* osizes;   // [B][2] (out_h, out_w) or NULL
  int Q, C, K;
  float* scores;           // [B][K]
  int64_t* labels;         // [B][K]
  int32_t* query;          // [B][K]
  float* out;              // [B][K][4] xyxy
};

// larger float <=> larger key; NaN (either sign) greatest; -0 and +0 the same key
__device__ __forceinline__ unsigned tk_key(float x) {
  unsigned u = __float_as_uint(x);
  if ((u & 0x7fffffffu) > 0x7f800000u) return 0xffffffffu;
  if ((u & 0x7fffffffu) == 0u) u = 0u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// sigmoid and 1 - sigmoid in fp64 without overflow or cancellation: e = exp(-|s|)
__device__ __forceinline__ void sigmoid_d(double s, double& y, double& omy) {
  const double e = exp(-fabs(s));
  const double a = 1.0 / (1.0 + e), c = e / (1.0 + e);
  y = s >= 0.0 ? a : c;
  omy = s >= 0.0 ? c : a;
  if (s != s) y = omy = s;
}

__device__ __forceinline__ float clampf_(float v, float hi) { return v < 0.f ? 0.f : (v > hi ? hi : v); }   // (NaN stays)

template <bool REG>
__global__ __launch_bounds__(TK_THREADS) void focal_topk_kernel(const TopkK p) {
  __shared__ int hist[TK_WAVES][256];
  __shared__ int tot[256];
  __shared__ int wc[2][TK_ITEMS * TK_WAVES];
  __shared__ unsigned long long sk[TK_MAXK];
  __shared__ unsigned s_T;
  __shared__ int s_krem, s_cgt, s_run[2];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const unsigned N = (unsigned)p.Q * (unsigned)p.C;                 // < 2^31
  const unsigned nrows = (N >> 10) + ((N & 1023u) != 0u);
  const float* lg = p.logits + (size_t)b * N;
  const int K = p.K;

  unsigned keys[TK_ITEMS];
  if (REG) {
#pragma unroll
    for (int i = 0; i < TK_ITEMS; ++i) {
      const unsigned idx = (unsigned)i * TK_THREADS + tid;
      keys[i] = idx < N ? tk_key(lg[idx]) : 0u;
    }
  }
  if (tid < 2) s_run[tid] = 0;

  // ---- 1. radix select
  unsigned T = 0u;
  int krem = K, cgt = 0;
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 24 - 8 * pass;
    const unsigned himask = pass == 0 ? 0u : (0xffffffffu << (shift + 8));
    for (int j = tid; j < TK_WAVES * 256; j += TK_THREADS) (&hist[0][0])[j] = 0;
    __syncthreads();
    if (REG) {
#pragma unroll
      for (int i = 0; i < TK_ITEMS; ++i) {
        const unsigned idx = (unsigned)i * TK_THREADS + tid;
        if (idx < N && ((keys[i] ^ T) & himask) == 0u) atomicAdd(&hist[wv][(keys[i] >> shift) & 255u], 1);
      }
    } else {
      for (unsigned r = 0; r < nrows; ++r) {
        const unsigned idx = r * TK_THREADS + tid;
        if (idx < N) {
          const unsigned k = tk_key(lg[idx]);
          if (((k ^ T) & himask) == 0u) atomicAdd(&hist[wv][(k >> shift) & 255u], 1);
        }
      }
    }
    __syncthreads();
    if (tid < 256) {
      int s = 0;
#pragma unroll
      for (int w = 0; w < TK_WAVES; ++w) s += hist[w][tid];
      tot[tid] = s;
    }
    __syncthreads();
    if (wv == 0) {      // lane l owns the bins 255 - 4 l .. 252 - 4 l: a descending scan
      int c[4], s = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) { c[j] = tot[255 - 4 * lane - j]; s += c[j]; }
      int inc = s;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const int v = __shfl_up(inc, o, 64);
        if (lane >= o) inc += v;
      }
      const int exc = inc - s;
      if (exc < krem && krem <= inc) {      // exactly one lane: the prefix class holds at least krem keys
        int a = exc, d = -1, above = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (d < 0 && krem <= a + c[j]) { d = 255 - 4 * lane - j; above = a; }
          a += c[j];
        }
        s_T = T | ((unsigned)d << shift);
        s_cgt = cgt + above;
        s_krem = krem - above;
      }
    }
    __syncthreads();
    T = s_T; cgt = s_cgt; krem = s_krem;
  }
  // T: the K-th largest key; cgt keys are larger (cgt < K); the krem lowest-index keys equal to T complete the K

  // ---- 2. compaction in index order, TK_ITEMS rows of 1024 at a time
  const unsigned long long ltmask = (1ull << lane) - 1ull;
  for (unsigned r0 = 0; r0 < nrows; r0 += TK_ITEMS) {
#pragma unroll
    for (int i = 0; i < TK_ITEMS; ++i) {
      const unsigned idx = (r0 + i) * TK_THREADS + tid;
      const bool valid = (r0 + i) < nrows && idx < N;
      const unsigned k = REG ? keys[i] : (valid ? tk_key(lg[idx]) : 0u);
      const unsigned long long bg = __ballot(valid && k > T), be = __ballot(valid && k == T);
      if (lane == 0) {
        wc[0][i * TK_WAVES + wv] = __popcll(bg);
        wc[1][i * TK_WAVES + wv] = __popcll(be);
      }
    }
    __syncthreads();
    if (wv < 2) {       // wave 0: the keys > T, wave 1: the ties; exclusive scan over (row, wave) + the running base
      int* tab = wc[wv];
      const int base = s_run[wv];
      int c[7], s = 0;
#pragma unroll
      for (int j = 0; j < 7; ++j) {
        const int e = lane * 7 + j;
        c[j] = e < TK_ITEMS * TK_WAVES ? tab[e] : 0;
        s += c[j];
      }
      int inc = s;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const int v = __shfl_up(inc, o, 64);
        if (lane >= o) inc += v;
      }
      int a = base + inc - s;
#pragma unroll
      for (int j = 0; j < 7; ++j) {
        const int e = lane * 7 + j;
        if (e < TK_ITEMS * TK_WAVES) tab[e] = a;
        a += c[j];
      }
      if (lane == 63) s_run[wv] = base + inc;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < TK_ITEMS; ++i) {
      const unsigned idx = (r0 + i) * TK_THREADS + tid;
      const bool valid = (r0 + i) < nrows && idx < N;
      const unsigned k = REG ? keys[i] : (valid ? tk_key(lg[idx]) : 0u);
      const bool gt = valid && k > T, eq = valid && k == T;
      const unsigned long long bg = __ballot(gt), be = __ballot(eq);
      int slot = -1;
      if (gt) slot = wc[0][i * TK_WAVES + wv] + __popcll(bg & ltmask);
      if (eq) {
        const int rk = wc[1][i * TK_WAVES + wv] + __popcll(be & ltmask);
        if (rk < krem) slot = cgt + rk;
      }
      if (slot >= 0 && slot < K) sk[slot] = ((unsigned long long)k << 32) | (unsigned long long)(~idx);
    }
    __syncthreads();
  }

  // ---- 3. + 4. position = number of larger words (key descending, then index ascending); the winners write their outputs
  if (tid >= K) return;
  const unsigned long long my = sk[tid];
  int pos = 0;
  for (int j = 0; j < K; ++j) pos += sk[j] > my ? 1 : 0;
  const unsigned idx = ~(unsigned)(my & 0xffffffffull);
  const unsigned q = idx / (unsigned)p.C, c = idx - q * (unsigned)p.C;
  double y, omy;
  sigmoid_d((double)lg[idx], y, omy);
  const size_t o = (size_t)b * K + pos;
  p.scores[o] = (float)y;
  p.labels[o] = (int64_t)c;
  p.query[o] = (int32_t)q;
  const f32x4 bx = *(const f32x4*)(p.boxes + ((size_t)b * p.Q + q) * 4);
  const int64_t ih = p.sizes[2 * b], iw = p.sizes[2 * b + 1];
  const float wf = (float)iw, hf = (float)ih;
  f32x4 v;
  v[0] = (bx[0] - 0.5f * bx[2]) * wf;
  v[1] = (bx[1] - 0.5f * bx[3]) * hf;
  v[2] = (bx[0] + 0.5f * bx[2]) * wf;
  v[3] = (bx[1] + 0.5f * bx[3]) * hf;
  if (p.osizes) {
    const int64_t oh = p.osizes[2 * b], ow = p.osizes[2 * b + 1];
    const float sx = (float)((double)ow / (double)iw), sy = (float)((double)oh / (double)ih);
    v[0] = clampf_(v[0] * sx, (float)ow);
    v[1] = clampf_(v[1] * sy, (float)oh);
    v[2] = clampf_(v[2] * sx, (float)ow);
    v[3] = clampf_(v[3] * sy, (float)oh);
  }
  *(f32x4*)(p.out + o * 4) = v;
}

extern "C" int mi_focal_topk_postprocess(const float* logits, const float* boxes, const int64_t* sizes_dev,
                                         const int64_t* out_sizes, int B, int Q, int C, int K, float* scores, int64_t* labels,
                                         int32_t* query, float* boxes_xyxy, mi_stream_t s) {
  MI_REQUIRE(logits && boxes && sizes_dev && scores && labels && query && boxes_xyxy, "focal_topk_postprocess: null");
  MI_REQUIRE(B >= 1 && Q >= 1 && C >= 1 && K >= 1, "focal_topk_postprocess: B %d, Q %d, C %d, K %d", B, Q, C, K);
  MI_REQUIRE((int64_t)Q * C < ((int64_t)1 << 31), "focal_topk_postprocess: Q * C = %lld >= 2^31", (long long)Q * C);
  MI_REQUIRE(K <= TK_MAXK, "focal_topk_postprocess: K %d > %d", K, TK_MAXK);
  MI_REQUIRE((int64_t)K <= (int64_t)Q * C, "focal_topk_postprocess: K %d > Q * C = %lld (torch.topk raises there)", K,
             (long long)Q * C);
  TopkK k;
  k.logits = logits; k.boxes = boxes; k.sizes = sizes_dev; k.osizes = out_sizes;
  k.Q = Q; k.C = C; k.K = K;
  k.scores = scores; k.labels = labels; k.query = query; k.out = boxes_xyxy;
  if ((int64_t)Q * C <= (int64_t)TK_ITEMS * TK_THREADS)
    hipLaunchKernelGGL(focal_topk_kernel<true>, dim3(B), dim3(TK_THREADS), 0, (hipStream_t)s, k);
  else
    hipLaunchKernelGGL(focal_topk_kernel<false>, dim3(B), dim3(TK_THREADS), 0, (hipStream_t)s, k);
  MI_CHECK_LAUNCH("focal_topk_postprocess");
  return MI_OK;
}

// ---- the SMCA box head tail
__global__ __launch_bounds__(256) void box_ref_sigmoid_fwd_kernel(const f32x4* __restrict__ x, const f32x2* __restrict__ p,
                                                                  f32x4* __restrict__ y, int L, int BQ) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)L * BQ) return;
  const f32x4 xv = x[i];
  const f32x2 pv = p[i % BQ];
  f32x4 o;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    double yy, om;
    sigmoid_d((double)xv[j] + (j < 2 ? (double)pv[j] : 0.0), yy, om);
    o[j] = (float)yy;
  }
  y[i] = o;
}

__global__ __launch_bounds__(256) void box_ref_sigmoid_bwd_kernel(const f32x4* __restrict__ x, const f32x2* __restrict__ p,
                                                                  const f32x4* __restrict__ dy, f32x4* __restrict__ dx,
                                                                  f32x2* __restrict__ dp, int L, int BQ) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= BQ) return;
  const f32x2 pv = p[r];
  float a0 = 0.f, a1 = 0.f;
  for (int l = 0; l < L; ++l) {           // the levels in ascending order: dp's summation order is fixed
    const int64_t i = (int64_t)l * BQ + r;
    const f32x4 xv = x[i], g = dy[i];
    f32x4 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      double yy, om;
      sigmoid_d((double)xv[j] + (j < 2 ? (double)pv[j] : 0.0), yy, om);
      o[j] = (float)((double)g[j] * yy * om);
    }
    dx[i] = o;
    a0 += o[0];
    a1 += o[1];
  }
  f32x2 d;
  d[0] = a0; d[1] = a1;
  dp[r] = d;
}

static int box_args(const void* x, const void* p, const void* a, const void* c, int L, int B, int Q, const char* what) {
  MI_REQUIRE(x && p && a && c, "%s: null", what);
  MI_REQUIRE(L >= 1 && B >= 1 && Q >= 1 && (int64_t)L * B * Q < ((int64_t)1 << 29), "%s: L %d, B %d, Q %d", what, L, B, Q);
  return MI_OK;
}

extern "C" int mi_box_ref_sigmoid_fwd(const float* x, const float* p, float* y, int L, int B, int Q, mi_stream_t s) {
  if (int rc = box_args(x, p, y, y, L, B, Q, "box_ref_sigmoid_fwd")) return rc;
  const int64_t n = (int64_t)L * B * Q;
  hipLaunchKernelGGL(box_ref_sigmoid_fwd_kernel, dim3((unsigned)mi_cdiv64(n, 256)), dim3(256), 0, (hipStream_t)s, (const f32x4*)x,
                     (const f32x2*)p, (f32x4*)y, L, B * Q);
  MI_CHECK_LAUNCH("box_ref_sigmoid_fwd");
  return MI_OK;
}

extern "C" int mi_box_ref_sigmoid_bwd(const float* x, const float* p, const float* dy, float* dx, float* dp, int L, int B, int Q,
                                      mi_stream_t s) {
  if (int rc = box_args(x, p, dy, dx, L, B, Q, "box_ref_sigmoid_bwd")) return rc;
  MI_REQUIRE(dp, "box_ref_sigmoid_bwd: null");
  hipLaunchKernelGGL(box_ref_sigmoid_bwd_kernel, dim3(mi_cdiv(B * Q, 256)), dim3(256), 0, (hipStream_t)s, (const f32x4*)x,
                     (const f32x2*)p, (const f32x4*)dy, (f32x4*)dx, (f32x2*)dp, L, B * Q);
  MI_CHECK_LAUNCH("box_ref_sigmoid_bwd");
  return MI_OK;
}
