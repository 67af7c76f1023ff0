// SparseInst inference postprocess for a whole batch (the reference: SparseInst.inference, meta_arch/sparseinst.py:169-234 +
// rescoring_mask :24-27 - a Python loop over the images, every step a torch op with an fp32 intermediate in HBM).
//
// Three launches, none of which waits for the host:
//   si_mask_sums    per (image, chunk of SI_CH pixels, query): sum(m * (m > thr)) and sum(m > thr), m = sigmoid(mask), as
//                   partial sums in the workspace - for EVERY query, so the launch does not depend on which are kept
//   si_select       one block per image: score = max_c sqrt(sigmoid(logit) * sigmoid(obj)) (first maximum), keep = score >
//                   cls_thr, kept queries compacted in ascending order, the chunk partials added in sequence (a fixed order:
//                   the scores do not change from run to run), score *= num / (den + 1e-6)
//   si_resize       per output pixel of every kept query the composition bilinear (h, w) -> (Hpad, Wpad), crop to (h_img,
//                   w_img), bilinear -> (Hout, Wout), compared with the mask threshold and written as one byte
// The host reads the B counts back between the second and the third and builds the per-image descriptors from them.
//
// si_resize: a block owns (image, tile of SI_TY x SI_TX output pixels, group of up to SI_QG kept queries).  The source
// pixels its tile can touch form a rectangle (src_index is monotonic): sigmoid is evaluated once per pixel of that rectangle
// and staged in LDS as fp32, query-major with an odd row stride - with the NHWC input the loading lanes run along the kept
// queries (neighbouring channels of one pixel, a 64 .. 256-byte line) and write LDS without bank conflicts; the computing
// lanes run along x of the output.  A rectangle that does not fit SI_LDS_FLOATS / SI_QG pixels (a large total down-scale)
// takes the 16 taps from global memory instead; the entry point decides that per image from the descriptor, and the block
// checks its own rectangle against the budget once more before it stages anything.
#include "common.h"
#include <cstring>

#define SI_CH 256            // pixels per partial sum
#define SI_TX 64
#define SI_TY 16
#define SI_QG 32
#define SI_LDS_FLOATS 8192   // 32 KB: a rectangle of up to 255 source pixels for 32 queries

// ATen area_pixel_compute_source_index (align_corners = False) as csrc/sparseinst_ops.hip restates it
__device__ __forceinline__ void si_src(int o, float scale, int n, int* i0, int* i1, float* l1) {
  float s = scale * ((float)o + 0.5f) - 0.5f;
  if (s < 0.f) s = 0.f;
  const int a = (int)s;
  *i0 = a < n - 1 ? a : n - 1;
  *i1 = a < n - 1 ? a + 1 : n - 1;
  *l1 = s - (float)a;
}
__device__ __forceinline__ float si_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }
__device__ __forceinline__ float si_load(const void* m, int dtype, int64_t off) {
  return dtype == 0 ? ((const float*)m)[off] : (float)((const __bf16*)m)[off];
}

struct SiSumsK {
  const void* masks;
  float* ws;              // [B][nchunk][2][N]
  int64_t sb, sq, sy, sx;
  int dtype, N, h, w, nchunk;
  float thr;
};

__global__ __launch_bounds__(256) void si_mask_sums_kernel(const SiSumsK p) {
  __shared__ float red[2][4][64];
  const int b = blockIdx.y, ch = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int P = p.h * p.w;
  const int p0 = ch * SI_CH, p1 = p0 + SI_CH < P ? p0 + SI_CH : P;
  float* const dst = p.ws + ((int64_t)b * p.nchunk + ch) * 2 * p.N;
  if (p.sq < p.sx) {
    // query-fastest (NHWC): lanes along the queries, the four waves share the chunk's pixels
    for (int q0 = 0; q0 < p.N; q0 += 64) {
      const int q = q0 + lane;
      float num = 0.f, den = 0.f;
      if (q < p.N) {
        for (int i = p0 + wave; i < p1; i += 4) {
          const int y = i / p.w, x = i - y * p.w;
          const float m = si_sigmoid(si_load(p.masks, p.dtype, b * p.sb + q * p.sq + y * p.sy + x * p.sx));
          const float k = m > p.thr ? 1.f : 0.f;
          num += m * k;
          den += k;
        }
      }
      red[0][wave][lane] = num;
      red[1][wave][lane] = den;
      __syncthreads();
      if (wave == 0 && q < p.N) {
        dst[q] = (red[0][0][lane] + red[0][1][lane]) + (red[0][2][lane] + red[0][3][lane]);
        dst[p.N + q] = (red[1][0][lane] + red[1][1][lane]) + (red[1][2][lane] + red[1][3][lane]);
      }
      __syncthreads();
    }
  } else {
    // pixel-fastest (NCHW): a wave per query, lanes along the chunk's pixels
    for (int q = wave; q < p.N; q += 4) {
      float num = 0.f, den = 0.f;
      for (int i = p0 + lane; i < p1; i += 64) {
        const int y = i / p.w, x = i - y * p.w;
        const float m = si_sigmoid(si_load(p.masks, p.dtype, b * p.sb + q * p.sq + y * p.sy + x * p.sx));
        const float k = m > p.thr ? 1.f : 0.f;
        num += m * k;
        den += k;
      }
      num = wave_sum(num);
      den = wave_sum(den);
      if (lane == 0) {
        dst[q] = num;
        dst[p.N + q] = den;
      }
    }
  }
}

struct SiSelectK {
  const float* logits;    // [B][N][C]
  const float* obj;       // [B][N]
  const float* ws;
  int* counts;
  int* kept;
  float* scores;
  int64_t* labels;
  int N, C, nchunk;
  float cls_thr;
};

__global__ __launch_bounds__(256) void si_select_kernel(const SiSelectK p) {
  __shared__ int wcount[4];
  const int b = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int running = 0;
  for (int base = 0; base < p.N; base += 256) {
    const int q = base + tid;
    float best = 0.f;
    int lab = 0;
    bool keep = false;
    if (q < p.N) {
      const float so = si_sigmoid(p.obj[(int64_t)b * p.N + q]);
      const float* const lg = p.logits + ((int64_t)b * p.N + q) * p.C;
      best = sqrtf(si_sigmoid(lg[0]) * so);
      for (int c = 1; c < p.C; ++c) {
        const float s = sqrtf(si_sigmoid(lg[c]) * so);
        if (s > best) {
          best = s;
          lab = c;
        }
      }
      keep = best > p.cls_thr;
    }
    const unsigned long long bal = __ballot(keep);
    if (lane == 0) wcount[wave] = __popcll(bal);
    __syncthreads();
    int pos = running + __popcll(bal & ((1ull << lane) - 1ull));
    int all = 0;
    for (int k = 0; k < 4; ++k) {
      if (k < wave) pos += wcount[k];
      all += wcount[k];
    }
    if (keep) {
      const float* const part = p.ws + (int64_t)b * p.nchunk * 2 * p.N;
      float num = 0.f, den = 0.f;
      for (int ch = 0; ch < p.nchunk; ++ch) {
        num += part[(int64_t)ch * 2 * p.N + q];
        den += part[(int64_t)ch * 2 * p.N + p.N + q];
      }
      const int64_t o = (int64_t)b * p.N + pos;
      p.kept[o] = q;
      p.scores[o] = best * (num / (den + 1e-6f));
      p.labels[o] = lab;
    }
    running += all;
    __syncthreads();
  }
  if (tid == 0) p.counts[b] = running;
}

struct SiImgK {
  int64_t out_off;
  int n, h_img, w_img, Hout, Wout, lds;
};
struct SiResizeK {
  const void* masks;
  const int* kept;        // [B][N]
  uint8_t* out;
  int64_t sb, sq, sy, sx;
  int dtype, N, h, w, Hpad, Wpad, b0;
  float thr;
  SiImgK d[MI_FEED_MAX_IMAGES];
};

// the two source taps of one axis for an OUTPUT index: the outer interpolation's two intermediate indices (clamped to the
// cropped size) and, for each of them, the inner interpolation's two source indices and its weight
struct SiAxis {
  int a0, a1, b0, b1;     // source indices behind the first / the second intermediate sample
  float la, lb, lo;       // inner weights of the two, outer weight
};
__device__ __forceinline__ SiAxis si_axis(int o, float outer, int n_img, float inner, int n_src) {
  SiAxis t;
  int i0, i1;
  si_src(o, outer, n_img, &i0, &i1, &t.lo);
  si_src(i0, inner, n_src, &t.a0, &t.a1, &t.la);
  si_src(i1, inner, n_src, &t.b0, &t.b1, &t.lb);
  return t;
}
__device__ __forceinline__ float si_bilerp(float ly, float lx, float a, float b, float c, float d) {
  const float hy0 = 1.f - ly, wx0 = 1.f - lx;
  return hy0 * (wx0 * a + lx * b) + ly * (wx0 * c + lx * d);
}

template <typename Tap>
__device__ __forceinline__ float si_compose(const SiAxis& Y, const SiAxis& X, Tap tap) {
  const float i00 = si_bilerp(Y.la, X.la, tap(Y.a0, X.a0), tap(Y.a0, X.a1), tap(Y.a1, X.a0), tap(Y.a1, X.a1));
  const float i01 = si_bilerp(Y.la, X.lb, tap(Y.a0, X.b0), tap(Y.a0, X.b1), tap(Y.a1, X.b0), tap(Y.a1, X.b1));
  const float i10 = si_bilerp(Y.lb, X.la, tap(Y.b0, X.a0), tap(Y.b0, X.a1), tap(Y.b1, X.a0), tap(Y.b1, X.a1));
  const float i11 = si_bilerp(Y.lb, X.lb, tap(Y.b0, X.b0), tap(Y.b0, X.b1), tap(Y.b1, X.b0), tap(Y.b1, X.b1));
  return si_bilerp(Y.lo, X.lo, i00, i01, i10, i11);
}

__global__ __launch_bounds__(256) void si_resize_kernel(const SiResizeK p) {
  __shared__ float patch[SI_LDS_FLOATS];
  __shared__ int qs[SI_QG];
  const SiImgK d = p.d[blockIdx.z];
  const int tiles_x = (d.Wout + SI_TX - 1) / SI_TX, tiles_y = (d.Hout + SI_TY - 1) / SI_TY;
  const int j0 = blockIdx.y * SI_QG;
  if ((int)blockIdx.x >= tiles_x * tiles_y || j0 >= d.n) return;
  const int nq = d.n - j0 < SI_QG ? d.n - j0 : SI_QG;
  const int b = p.b0 + blockIdx.z;
  const int tid = threadIdx.x;
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int oy0 = ty * SI_TY, ox0 = tx * SI_TX;
  const int oy1 = (oy0 + SI_TY < d.Hout ? oy0 + SI_TY : d.Hout) - 1, ox1 = (ox0 + SI_TX < d.Wout ? ox0 + SI_TX : d.Wout) - 1;
  const float oys = (float)d.h_img / (float)d.Hout, oxs = (float)d.w_img / (float)d.Wout;
  const float iys = (float)p.h / (float)p.Hpad, ixs = (float)p.w / (float)p.Wpad;

  if (tid < SI_QG) {
    int q = tid < nq ? p.kept[(int64_t)b * p.N + j0 + tid] : -1;
    qs[tid] = (unsigned)q < (unsigned)p.N ? q : -1;      // (a table beyond the counts: that query's masks stay zero)
  }
  // the rectangle of source pixels behind this tile (both index maps are monotonic)
  const SiAxis Ylo = si_axis(oy0, oys, d.h_img, iys, p.h), Yhi = si_axis(oy1, oys, d.h_img, iys, p.h);
  const SiAxis Xlo = si_axis(ox0, oxs, d.w_img, ixs, p.w), Xhi = si_axis(ox1, oxs, d.w_img, ixs, p.w);
  const int sy_lo = Ylo.a0, sy_hi = Yhi.b1, sx_lo = Xlo.a0, sx_hi = Xhi.b1;
  const int ph = sy_hi - sy_lo + 1, pw = sx_hi - sx_lo + 1;
  const int pp = ph * pw, pps = pp | 1;
  const bool lds = d.lds != 0 && ph >= 1 && pw >= 1 && (int64_t)ph * pw < SI_LDS_FLOATS / SI_QG;
  __syncthreads();
  if (lds) {
    const int total = nq * pp;
    const bool qfast = p.sq < p.sx;
    for (int i = tid; i < total; i += 256) {
      int jj, pix;
      if (qfast) {
        pix = i / nq;
        jj = i - pix * nq;
      } else {
        jj = i / pp;
        pix = i - jj * pp;
      }
      const int y = pix / pw, x = pix - y * pw;
      const int q = qs[jj];
      float v = 0.f;
      if (q >= 0) v = si_sigmoid(si_load(p.masks, p.dtype, b * p.sb + q * p.sq + (sy_lo + y) * p.sy + (sx_lo + x) * p.sx));
      patch[jj * pps + pix] = v;
    }
    __syncthreads();
  }

  // a thread = four consecutive pixels of one output row, every query of the group
  const int oy = oy0 + (tid >> 4), oxb = ox0 + (tid & 15) * 4;
  if (oy > oy1 || oxb > ox1) return;
  const SiAxis Y = si_axis(oy, oys, d.h_img, iys, p.h);
  SiAxis X[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) X[e] = si_axis(oxb + e <= ox1 ? oxb + e : ox1, oxs, d.w_img, ixs, p.w);
  const int nvalid = ox1 - oxb + 1 < 4 ? ox1 - oxb + 1 : 4;
  // LDS path: the indices become offsets into the staged rectangle (clamped into it: a no-op unless the per-pixel and the
  // per-tile index maps disagreed), so that a tap is one LDS read at row offset + column offset
  SiAxis Yl = Y, Xl[4];
  if (lds) {
    auto rel = [](int v, int lo, int n) { v -= lo; return v < 0 ? 0 : (v < n ? v : n - 1); };
    Yl.a0 = rel(Y.a0, sy_lo, ph) * pw; Yl.a1 = rel(Y.a1, sy_lo, ph) * pw;
    Yl.b0 = rel(Y.b0, sy_lo, ph) * pw; Yl.b1 = rel(Y.b1, sy_lo, ph) * pw;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      Xl[e] = X[e];
      Xl[e].a0 = rel(X[e].a0, sx_lo, pw); Xl[e].a1 = rel(X[e].a1, sx_lo, pw);
      Xl[e].b0 = rel(X[e].b0, sx_lo, pw); Xl[e].b1 = rel(X[e].b1, sx_lo, pw);
    }
  }
  for (int jj = 0; jj < nq; ++jj) {
    const int q = qs[jj];
    uint32_t bits = 0;
    if (q >= 0) {
      if (lds) {
        const float* const pl = patch + jj * pps;
        auto tap = [&](int y, int x) { return pl[y + x]; };
#pragma unroll
        for (int e = 0; e < 4; ++e) bits |= (si_compose(Yl, Xl[e], tap) > p.thr ? 1u : 0u) << (8 * e);
      } else {
        const int64_t base = b * p.sb + q * p.sq;
        auto tap = [&](int y, int x) { return si_sigmoid(si_load(p.masks, p.dtype, base + y * p.sy + x * p.sx)); };
#pragma unroll 1
        for (int e = 0; e < nvalid; ++e)     // (the axis is recomputed: X[e] with a run-time e would live in scratch)
          bits |= (si_compose(Y, si_axis(oxb + e, oxs, d.w_img, ixs, p.w), tap) > p.thr ? 1u : 0u) << (8 * e);
      }
    }
    uint8_t* const dst = p.out + d.out_off + ((int64_t)(j0 + jj) * d.Hout + oy) * d.Wout + oxb;
    if (nvalid == 4 && ((uintptr_t)dst & 3) == 0) {
      *(uint32_t*)dst = bits;
    } else {
      for (int e = 0; e < nvalid; ++e) dst[e] = (uint8_t)(bits >> (8 * e));
    }
  }
}

static bool si_dims_ok(int B, int N, int h, int w) { return B >= 0 && N >= 1 && h >= 1 && w >= 1; }

extern "C" int64_t mi_sparseinst_infer_ws_bytes(int B, int N, int h, int w) {
  if (!si_dims_ok(B, N, h, w) || (int64_t)h * w > INT32_MAX) return -1;
  const int64_t nchunk = ((int64_t)h * w + SI_CH - 1) / SI_CH;
  return (int64_t)B * nchunk * 2 * N * (int64_t)sizeof(float);
}

static int si_check_masks(const void* masks, int dtype, int64_t sb, int64_t sq, int64_t sy, int64_t sx, const char* who) {
  MI_REQUIRE(masks, "%s: null pointer (masks)", who);
  MI_REQUIRE(dtype == 0 || dtype == 1, "%s: mask dtype %d (0 = fp32, 1 = bf16)", who, dtype);
  MI_REQUIRE(sb >= 0 && sq >= 1 && sy >= 1 && sx >= 1, "%s: mask strides (%lld, %lld, %lld, %lld) must be positive", who,
             (long long)sb, (long long)sq, (long long)sy, (long long)sx);
  return MI_OK;
}

extern "C" int mi_sparseinst_infer_select(const float* logits, const float* obj, const void* masks, int mask_dtype, int64_t sb,
                                          int64_t sq, int64_t sy, int64_t sx, int B, int N, int C, int h, int w, float cls_thr,
                                          float mask_thr, int* counts, int* kept_query, float* scores, int64_t* labels, void* ws,
                                          int64_t ws_bytes, mi_stream_t st) {
  MI_REQUIRE(B >= 0, "sparseinst_infer_select: B = %d", B);
  MI_REQUIRE(N >= 1 && C >= 1 && h >= 1 && w >= 1, "sparseinst_infer_select: N = %d, C = %d, masks %d x %d", N, C, h, w);
  MI_REQUIRE((int64_t)h * w <= INT32_MAX, "sparseinst_infer_select: masks %d x %d exceed 2^31 pixels", h, w);
  MI_REQUIRE(logits && obj && counts && kept_query && scores && labels && ws, "sparseinst_infer_select: null pointer");
  if (si_check_masks(masks, mask_dtype, sb, sq, sy, sx, "sparseinst_infer_select") != MI_OK) return MI_EINVAL;
  MI_REQUIRE(B <= 65535, "sparseinst_infer_select: B = %d exceeds the grid", B);
  MI_REQUIRE(ws_bytes >= mi_sparseinst_infer_ws_bytes(B, N, h, w), "sparseinst_infer_select: workspace of %lld bytes, %lld needed",
             (long long)ws_bytes, (long long)mi_sparseinst_infer_ws_bytes(B, N, h, w));
  MI_REQUIRE(((uintptr_t)ws & 3) == 0, "sparseinst_infer_select: workspace not 4-byte aligned");
  if (B == 0) return MI_OK;
  const int nchunk = (h * w + SI_CH - 1) / SI_CH;
  SiSumsK a;
  a.masks = masks; a.ws = (float*)ws; a.sb = sb; a.sq = sq; a.sy = sy; a.sx = sx;
  a.dtype = mask_dtype; a.N = N; a.h = h; a.w = w; a.nchunk = nchunk; a.thr = mask_thr;
  hipLaunchKernelGGL(si_mask_sums_kernel, dim3(nchunk, B), dim3(256), 0, (hipStream_t)st, a);
  MI_CHECK_LAUNCH("si_mask_sums");
  SiSelectK s;
  s.logits = logits; s.obj = obj; s.ws = (const float*)ws; s.counts = counts; s.kept = kept_query; s.scores = scores;
  s.labels = labels; s.N = N; s.C = C; s.nchunk = nchunk; s.cls_thr = cls_thr;
  hipLaunchKernelGGL(si_select_kernel, dim3(B), dim3(256), 0, (hipStream_t)st, s);
  MI_CHECK_LAUNCH("si_select");
  return MI_OK;
}

// an upper bound of the source rows (columns) behind `tile` consecutive output rows: the outer map moves by n_img / n_out per
// output row and touches one more, the inner one by n_src / n_pad per intermediate row and touches one more
static int si_span_bound(int tile, int n_img, int n_out, int n_src, int n_pad) {
  const double outer = ((double)(tile - 1) * n_img) / n_out + 2.0;
  const double inner = outer * n_src / n_pad + 2.0;
  const int64_t v = (int64_t)inner + 2;
  return v < n_src ? (int)v : n_src;
}

extern "C" int mi_sparseinst_infer_masks(const void* masks, int mask_dtype, int64_t sb, int64_t sq, int64_t sy, int64_t sx, int B,
                                         int N, int h, int w, int Hpad, int Wpad, const int* kept_query,
                                         const mi_sparseinst_infer_desc* descs, float mask_thr, void* out, int64_t out_bytes,
                                         mi_stream_t st) {
  MI_REQUIRE(B >= 0, "sparseinst_infer_masks: B = %d", B);
  MI_REQUIRE(N >= 1 && h >= 1 && w >= 1, "sparseinst_infer_masks: N = %d, masks %d x %d", N, h, w);
  MI_REQUIRE(Hpad >= 1 && Wpad >= 1, "sparseinst_infer_masks: padded shape %d x %d", Hpad, Wpad);
  MI_REQUIRE(kept_query && descs && out, "sparseinst_infer_masks: null pointer");
  if (si_check_masks(masks, mask_dtype, sb, sq, sy, sx, "sparseinst_infer_masks") != MI_OK) return MI_EINVAL;
  MI_REQUIRE(out_bytes >= 0, "sparseinst_infer_masks: out_bytes = %lld", (long long)out_bytes);
  int64_t total = 0;
  for (int b = 0; b < B; ++b) {
    const mi_sparseinst_infer_desc& d = descs[b];
    MI_REQUIRE(d.n >= 0 && d.n <= N, "sparseinst_infer_masks: image %d: %d kept queries of %d", b, d.n, N);
    if (d.n == 0) continue;
    MI_REQUIRE(d.Hout >= 1 && d.Wout >= 1, "sparseinst_infer_masks: image %d: output size %d x %d", b, d.Hout, d.Wout);
    MI_REQUIRE(d.h_img >= 1 && d.w_img >= 1 && d.h_img <= Hpad && d.w_img <= Wpad,
               "sparseinst_infer_masks: image %d: image size %d x %d outside the padded shape %d x %d", b, d.h_img, d.w_img, Hpad, Wpad);
    const int64_t bytes = (int64_t)d.n * d.Hout * d.Wout;
    MI_REQUIRE(d.out_off >= 0 && d.out_off <= out_bytes && bytes <= out_bytes - d.out_off,
               "sparseinst_infer_masks: image %d: %lld bytes at offset %lld exceed the result (%lld bytes)", b, (long long)bytes,
               (long long)d.out_off, (long long)out_bytes);
    const int64_t tiles = (int64_t)mi_cdiv(d.Hout, SI_TY) * mi_cdiv(d.Wout, SI_TX);
    MI_REQUIRE(tiles <= INT32_MAX, "sparseinst_infer_masks: image %d: output size %d x %d exceeds the grid", b, d.Hout, d.Wout);
    total += bytes;
  }
  if (B == 0 || total == 0) return MI_OK;
  for (int b0 = 0; b0 < B; b0 += MI_FEED_MAX_IMAGES) {
    SiResizeK k;
    memset(&k, 0, sizeof(k));
    const int nb = B - b0 < MI_FEED_MAX_IMAGES ? B - b0 : MI_FEED_MAX_IMAGES;
    k.masks = masks; k.kept = kept_query; k.out = (uint8_t*)out; k.sb = sb; k.sq = sq; k.sy = sy; k.sx = sx;
    k.dtype = mask_dtype; k.N = N; k.h = h; k.w = w; k.Hpad = Hpad; k.Wpad = Wpad; k.b0 = b0; k.thr = mask_thr;
    int64_t gt = 0;
    int gq = 0;
    for (int b = 0; b < nb; ++b) {
      const mi_sparseinst_infer_desc& d = descs[b0 + b];
      if (d.n == 0) continue;
      SiImgK& o = k.d[b];
      o.out_off = d.out_off; o.n = d.n; o.h_img = d.h_img; o.w_img = d.w_img; o.Hout = d.Hout; o.Wout = d.Wout;
      const int64_t rect = (int64_t)si_span_bound(SI_TY, d.h_img, d.Hout, h, Hpad) * si_span_bound(SI_TX, d.w_img, d.Wout, w, Wpad);
      o.lds = rect < SI_LDS_FLOATS / SI_QG ? 1 : 0;
      const int64_t tiles = (int64_t)mi_cdiv(d.Hout, SI_TY) * mi_cdiv(d.Wout, SI_TX);
      if (tiles > gt) gt = tiles;
      if (mi_cdiv(d.n, SI_QG) > gq) gq = mi_cdiv(d.n, SI_QG);
    }
    if (gq == 0) continue;
    hipLaunchKernelGGL(si_resize_kernel, dim3((unsigned)gt, gq, nb), dim3(256), 0, (hipStream_t)st, k);
    MI_CHECK_LAUNCH("si_resize");
  }
  return MI_OK;
}
