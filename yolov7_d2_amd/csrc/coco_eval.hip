// COCO AP / AR evaluation on the device: what cocoapi's COCOeval (PythonAPI/pycocotools/cocoeval.py evaluate ->
// accumulate) and common/maskApi.c (bbIou, rleIou, rleDecode, rleFrString) compute, un-vendored and restated
// (tests/cocoeval_ref.py is the loop-form restatement these kernels are compared with, element for element).
//
// Everything is fp64 or integer in the operation order of the originals (this file is built with -ffp-contract=off: a
// contracted da + ga - w * h is not numpy's result), so the precision / recall / scores arrays are equal, not close.
//   mi_coco_box_iou     bbIou: one thread per (detection, ground truth)
//   mi_coco_mask_iou    rleIou on dense masks: bit-pack with a 64-lane ballot, areas by popcount, one wave per pair
//   mi_rle_decode       rleDecode: block scan of the runs, every pixel finds its run
//   mi_coco_match       evaluateImg: one wave per (image, category, area range), lanes = IoU thresholds
//   mi_coco_accumulate  accumulate: one thread per (category, area range, maxDets, IoU threshold)
#include <float.h>
#include <vector>
#include "common.h"

#define CE_T 256

// ------------------------------------------------------------------------------------------------------------- bbIou
__global__ __launch_bounds__(CE_T) void coco_box_iou_kernel(const double* __restrict__ dt, int D, const double* __restrict__ gt,
                                                             int G, const uint8_t* __restrict__ crowd, double* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * CE_T + threadIdx.x;
  if (i >= (int64_t)D * G) return;
  const int d = (int)(i / G), g = (int)(i - (int64_t)d * G);
  const double dx = dt[4 * d], dy = dt[4 * d + 1], dw = dt[4 * d + 2], dh = dt[4 * d + 3];
  const double gx = gt[4 * g], gy = gt[4 * g + 1], gw = gt[4 * g + 2], gh = gt[4 * g + 3];
  const double da = dw * dh, ga = gw * gh;
  double o = 0.0;
  const double w = fmin(dw + dx, gw + gx) - fmax(dx, gx);
  if (w > 0) {
    const double h = fmin(dh + dy, gh + gy) - fmax(dy, gy);
    if (h > 0) {
      const double in = w * h;
      const double u = (crowd && crowd[g]) ? da : da + ga - in;
      o = in / u;
    }
  }
  out[i] = o;
}

extern "C" int mi_coco_box_iou(const double* dt, int D, const double* gt, int G, const uint8_t* gcrowd, double* iou, mi_stream_t st) {
  MI_REQUIRE(D >= 0 && G >= 0, "coco_box_iou: negative size (D %d, G %d)", D, G);
  if (D == 0 || G == 0) return MI_OK;
  MI_REQUIRE(dt && gt && iou, "coco_box_iou: null");
  const int64_t n = (int64_t)D * G;
  MI_REQUIRE(mi_cdiv64(n, CE_T) < (1LL << 31), "coco_box_iou: %d x %d pairs", D, G);
  hipLaunchKernelGGL(coco_box_iou_kernel, dim3((unsigned)mi_cdiv64(n, CE_T)), dim3(CE_T), 0, (hipStream_t)st, dt, D, gt, G, gcrowd, iou);
  MI_CHECK_LAUNCH("coco_box_iou");
  return MI_OK;
}

// ------------------------------------------------------------------------------------------------------------ rleIou
// masks [n][H*W] bytes -> words [n][NW] of 64 pixels each (row-major pixel p is bit p % 64 of word p / 64); the lanes
// beyond H*W vote 0, so the last partial word carries no stray bit.  One wave per word, grid-strided.
__global__ __launch_bounds__(CE_T) void coco_pack_kernel(const uint8_t* __restrict__ masks, int64_t HW, int64_t NW,
                                                          unsigned long long* __restrict__ words) {
  const int lane = threadIdx.x & 63;
  const uint8_t* m = masks + (size_t)blockIdx.y * HW;
  unsigned long long* out = words + (size_t)blockIdx.y * NW;
  for (int64_t w = (int64_t)blockIdx.x * (CE_T / 64) + (threadIdx.x >> 6); w < NW; w += (int64_t)gridDim.x * (CE_T / 64)) {
    const int64_t p = w * 64 + lane;
    const unsigned long long b = __ballot(p < HW && m[p] != 0);
    if (lane == 0) out[w] = b;
  }
}

__device__ __forceinline__ long long wave_sum_ll(long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// one wave per mask: its area
__global__ __launch_bounds__(CE_T) void coco_area_kernel(const unsigned long long* __restrict__ words, int n, int64_t NW,
                                                          int64_t* __restrict__ area) {
  const int lane = threadIdx.x & 63;
  const int k = blockIdx.x * (CE_T / 64) + (threadIdx.x >> 6);
  if (k >= n) return;
  const unsigned long long* a = words + (size_t)k * NW;
  long long c = 0;
  for (int64_t w = lane; w < NW; w += 64) c += __popcll(a[w]);
  c = wave_sum_ll(c);
  if (lane == 0) area[k] = c;
}

// one wave per (detection, ground truth): |a & b|, then maskApi.c rleIou's  if(i==0) u=1; else if(crowd) u=area(dt)
__global__ __launch_bounds__(CE_T) void coco_mask_pair_kernel(const unsigned long long* __restrict__ dw, int D,
                                                               const unsigned long long* __restrict__ gw, int G, int64_t NW,
                                                               const uint8_t* __restrict__ crowd, const int64_t* __restrict__ darea,
                                                               const int64_t* __restrict__ garea, int64_t* __restrict__ inter,
                                                               double* __restrict__ iou) {
  const int lane = threadIdx.x & 63;
  const int64_t pair = (int64_t)blockIdx.x * (CE_T / 64) + (threadIdx.x >> 6);
  if (pair >= (int64_t)D * G) return;
  const int d = (int)(pair / G), g = (int)(pair - (int64_t)d * G);
  const unsigned long long* a = dw + (size_t)d * NW;
  const unsigned long long* b = gw + (size_t)g * NW;
  long long c = 0;
  for (int64_t w = lane; w < NW; w += 64) c += __popcll(a[w] & b[w]);
  c = wave_sum_ll(c);
  if (lane == 0) {
    inter[pair] = c;
    long long u = 1;
    if (c != 0) u = (crowd && crowd[g]) ? darea[d] : darea[d] + garea[g] - c;
    iou[pair] = (double)c / (double)u;
  }
}

extern "C" int64_t mi_coco_mask_iou_ws_bytes(int D, int G, int H, int W) {
  if (D < 0 || G < 0 || H < 1 || W < 1) return -1;
  return ((int64_t)D + G) * (((int64_t)H * W + 63) / 64) * 8;
}

extern "C" int mi_coco_mask_iou(const uint8_t* dmasks, int D, const uint8_t* gmasks, int G, int H, int W, const uint8_t* gcrowd,
                                void* ws, int64_t ws_bytes, int64_t* inter, int64_t* darea, int64_t* garea, double* iou,
                                mi_stream_t st) {
  MI_REQUIRE(D >= 0 && G >= 0 && H >= 1 && W >= 1 && (int64_t)H * W < (1LL << 31), "coco_mask_iou: sizes (D %d, G %d, H %d, W %d)", D,
             G, H, W);
  if (D == 0 && G == 0) return MI_OK;
  const int64_t HW = (int64_t)H * W, NW = (HW + 63) / 64;
  MI_REQUIRE(ws && ws_bytes >= mi_coco_mask_iou_ws_bytes(D, G, H, W) && ((uintptr_t)ws & 7) == 0,
             "coco_mask_iou: workspace of %lld bytes, %lld needed (8-byte aligned)", (long long)ws_bytes,
             (long long)mi_coco_mask_iou_ws_bytes(D, G, H, W));
  MI_REQUIRE((D == 0 || (dmasks && darea)) && (G == 0 || (gmasks && garea)) && (D == 0 || G == 0 || (inter && iou)), "coco_mask_iou: null");
  MI_REQUIRE(D <= 65535 && G <= 65535 && mi_cdiv64((int64_t)D * G, CE_T / 64) < (1LL << 31), "coco_mask_iou: %d x %d pairs", D, G);
  unsigned long long* dwords = (unsigned long long*)ws;
  unsigned long long* gwords = dwords + (size_t)D * NW;
  const unsigned gx = (unsigned)(mi_cdiv64(NW, CE_T / 64) < 1024 ? mi_cdiv64(NW, CE_T / 64) : 1024);
  hipStream_t s = (hipStream_t)st;
  if (D) {
    hipLaunchKernelGGL(coco_pack_kernel, dim3(gx, D), dim3(CE_T), 0, s, dmasks, HW, NW, dwords);
    hipLaunchKernelGGL(coco_area_kernel, dim3(mi_cdiv(D, CE_T / 64)), dim3(CE_T), 0, s, dwords, D, NW, darea);
  }
  if (G) {
    hipLaunchKernelGGL(coco_pack_kernel, dim3(gx, G), dim3(CE_T), 0, s, gmasks, HW, NW, gwords);
    hipLaunchKernelGGL(coco_area_kernel, dim3(mi_cdiv(G, CE_T / 64)), dim3(CE_T), 0, s, gwords, G, NW, garea);
  }
  if (D && G)
    hipLaunchKernelGGL(coco_mask_pair_kernel, dim3((unsigned)mi_cdiv64((int64_t)D * G, CE_T / 64)), dim3(CE_T), 0, s, dwords, D, gwords, G,
                       NW, gcrowd, darea, garea, inter, iou);
  MI_CHECK_LAUNCH("coco_mask_iou");
  return MI_OK;
}

// --------------------------------------------------------------------------------------------------------- rleDecode
// one block per mask.  cum[r] = counts[0] + .. + counts[r] (the END of run r in the column-major sequence); the pixel at
// column-major position p belongs to the first run with cum[r] > p (zero-length runs are passed over), odd runs are ones.
// A mask whose counts do not sum to H*W raises err[mask] and is written as zeros.
__global__ __launch_bounds__(CE_T) void rle_decode_kernel(const uint32_t* __restrict__ counts, const int32_t* __restrict__ nruns,
                                                           int max_runs, int H, int W, uint32_t* __restrict__ cum_ws,
                                                           uint8_t* __restrict__ out, int32_t* __restrict__ err) {
  __shared__ unsigned long long s_sum[CE_T];
  __shared__ unsigned long long s_total;
  const int tid = threadIdx.x;
  const int64_t HW = (int64_t)H * W;
  const uint32_t* c = counts + (size_t)blockIdx.x * max_runs;
  uint32_t* cum = cum_ws + (size_t)blockIdx.x * max_runs;
  uint8_t* o = out + (size_t)blockIdx.x * HW;
  int R = nruns[blockIdx.x];
  const bool bad_r = R < 0 || R > max_runs;
  if (bad_r) R = 0;
  const int per = (R + CE_T - 1) / CE_T;
  const int r0 = tid * per < R ? tid * per : R, r1 = r0 + per < R ? r0 + per : R;
  unsigned long long acc = 0;
  for (int r = r0; r < r1; ++r) acc += c[r];
  s_sum[tid] = acc;
  __syncthreads();
  if (tid == 0) {   // exclusive scan (256 entries: serial is fine)
    unsigned long long a = 0;
    for (int t = 0; t < CE_T; ++t) { const unsigned long long v = s_sum[t]; s_sum[t] = a; a += v; }
    s_total = a;
  }
  __syncthreads();
  const bool ok = !bad_r && s_total == (unsigned long long)HW;   // then every partial sum is <= H*W < 2^31
  if (tid == 0) err[blockIdx.x] = ok ? 0 : 1;
  if (ok) {
    acc = s_sum[tid];
    for (int r = r0; r < r1; ++r) { acc += c[r]; cum[r] = (uint32_t)acc; }
  }
  __syncthreads();
  for (int64_t q = tid; q < HW; q += CE_T) {
    uint8_t v = 0;
    if (ok) {
      const int y = (int)(q / W), x = (int)(q - (int64_t)y * W);
      const uint32_t p = (uint32_t)((int64_t)x * H + y);
      int lo = 0, hi = R - 1;   // first r with cum[r] > p; cum[R - 1] == H*W > p
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (cum[mid] > p) hi = mid; else lo = mid + 1;
      }
      v = (uint8_t)(lo & 1);
    }
    o[q] = v;
  }
}

extern "C" int mi_rle_decode(const uint32_t* counts, const int32_t* nruns, int n, int max_runs, int H, int W, uint32_t* cum_ws,
                             uint8_t* out, int32_t* err, int wait, mi_stream_t st) {
  MI_REQUIRE(n >= 0 && H >= 1 && W >= 1 && (int64_t)H * W < (1LL << 31), "rle_decode: sizes (n %d, H %d, W %d)", n, H, W);
  MI_REQUIRE(max_runs >= 1, "rle_decode: max_runs %d too small", max_runs);
  if (n == 0) return MI_OK;
  MI_REQUIRE(counts && nruns && cum_ws && out && err, "rle_decode: null");
  hipLaunchKernelGGL(rle_decode_kernel, dim3(n), dim3(CE_T), 0, (hipStream_t)st, counts, nruns, max_runs, H, W, cum_ws, out, err);
  MI_CHECK_LAUNCH("rle_decode");
  if (wait) {   // the one waiting form: the per-mask flags come back and a malformed mask is an argument error
    std::vector<int32_t> h(n);
    hipError_t e = hipMemcpyAsync(h.data(), err, sizeof(int32_t) * n, hipMemcpyDeviceToHost, (hipStream_t)st);
    if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)st);
    if (e != hipSuccess) MI_FAIL(MI_ELAUNCH, "rle_decode: %s", hipGetErrorString(e));
    for (int k = 0; k < n; ++k)
      if (h[k]) MI_FAIL(MI_EINVAL, "rle_decode: the counts of mask %d do not sum to H * W = %lld (or its nruns is outside [0, %d])", k,
                        (long long)H * W, max_runs);
  }
  return MI_OK;
}

// host: maskApi.c rleFrString, the inverse of mi_rle_to_string.  Returns the number of runs.
extern "C" int mi_rle_from_string(const char* s, uint32_t* counts, int max_runs) {
  MI_REQUIRE(s && counts && max_runs >= 0, "rle_from_string: args");
  int m = 0;
  size_t p = 0;
  while (s[p]) {
    long x = 0;
    int k = 0, more = 1;
    while (more) {
      if (!s[p]) MI_FAIL(MI_EINVAL, "rle_from_string: the string ends inside a count");
      const char c = (char)(s[p] - 48);
      if (k < 12) x |= (long)(c & 0x1f) << (5 * k);
      more = c & 0x20;
      ++p;
      ++k;
      if (!more && (c & 0x10) && k < 12) x |= -1L << (5 * k);
    }
    if (m > 2) x += (long)counts[m - 2];
    if (m >= max_runs) MI_FAIL(MI_EINVAL, "rle_from_string: max_runs %d too small", max_runs);
    counts[m++] = (uint32_t)x;
  }
  return m;
}

// ------------------------------------------------------------------------------------------------------- evaluateImg
// wave = (cell, area range), cell = image * K + category; lane = IoU threshold.  The cell's detections are the slice
// [det_start[cell], det_start[cell + 1]) of the arrays sorted by (cell, -score, stable), the first max_det of them enter;
// its ground truths the slice of the tables sorted by (cell, annotation order).  cocoapi orders the ground truths by their
// ignore flag with a stable sort and walks them once; here the lane walks the kept ones, then the ignored ones - the same
// sequence - and  `if m>-1 and gtIg[m]==0 and gtIg[gind]==1: break`  is the test in front of the second walk.
__global__ __launch_bounds__(CE_T) void coco_match_kernel(
    const double* __restrict__ iou, const int64_t* __restrict__ det_row, const double* __restrict__ det_area,
    const int64_t* __restrict__ det_start, const int64_t* __restrict__ gt_start, const int32_t* __restrict__ gt_col,
    const double* __restrict__ gt_area, const uint8_t* __restrict__ gt_crowd, const double* __restrict__ iou_thrs, int T,
    const double* __restrict__ area_rng, int A, int max_det, int64_t ncell, int64_t N, int64_t Gt, uint8_t* __restrict__ dtm,
    uint8_t* __restrict__ dtig, uint8_t* __restrict__ gtig, uint8_t* __restrict__ gtm, int32_t* __restrict__ npig) {
  const int lane = threadIdx.x & 63;
  const int64_t wid = (int64_t)blockIdx.x * (CE_T / 64) + (threadIdx.x >> 6);
  if (wid >= ncell * A) return;
  const int64_t cell = wid / A;
  const int a = (int)(wid - cell * A);
  const int64_t ds = det_start[cell], gs = gt_start[cell];
  const int64_t dn = det_start[cell + 1] - ds;
  const int D = (int)(dn < max_det ? dn : max_det), G = (int)(gt_start[cell + 1] - gs);
  const double lo = area_rng[2 * a], hi = area_rng[2 * a + 1];
  long long cnt = 0;
  for (int g = lane; g < G; g += 64) {
    const double ar = gt_area[gs + g];
    const int ig = gt_crowd[gs + g] || ar < lo || ar > hi;
    gtig[(size_t)a * Gt + gs + g] = (uint8_t)ig;
    cnt += !ig;
  }
  cnt = wave_sum_ll(cnt);
  if (lane == 0) npig[cell * A + a] = (int32_t)cnt;
  if (lane >= T || D == 0) return;
  const double thr = iou_thrs[lane];
  uint8_t* gm = gtm + ((size_t)a * T + lane) * Gt + gs;
  uint8_t* om = dtm + ((size_t)a * T + lane) * N + ds;
  uint8_t* oi = dtig + ((size_t)a * T + lane) * N + ds;
  for (int g = 0; g < G; ++g) gm[g] = 0;
  for (int d = 0; d < D; ++d) {
    double best = fmin(thr, 1 - 1e-10);
    int m = -1;
    const double* row = iou + det_row[ds + d];
    for (int pass = 0; pass < 2; ++pass) {
      if (pass == 1 && m > -1) break;
      for (int g = 0; g < G; ++g) {
        const double ar = gt_area[gs + g];
        const int crowd = gt_crowd[gs + g];
        const int ig = crowd || ar < lo || ar > hi;
        if (ig != pass) continue;
        if (gm[g] && !crowd) continue;
        const double v = row[gt_col[gs + g]];
        if (v < best) continue;
        best = v;
        m = g;
      }
      if (pass == 0 && m > -1) break;
    }
    if (m > -1) {
      const double ar = gt_area[gs + m];
      om[d] = 1;
      oi[d] = (uint8_t)(gt_crowd[gs + m] || ar < lo || ar > hi);
      gm[m] = 1;
    } else {
      const double da = det_area[ds + d];
      om[d] = 0;
      oi[d] = (uint8_t)(da < lo || da > hi);
    }
  }
}

extern "C" int mi_coco_match(const double* iou, const int64_t* det_row, const double* det_area, const int64_t* det_start,
                             const int64_t* gt_start, const int32_t* gt_col, const double* gt_area, const uint8_t* gt_crowd,
                             const double* iou_thrs, int T, const double* area_rng, int A, int max_det, int64_t ncell, int64_t N,
                             int64_t Gt, uint8_t* dtm, uint8_t* dtig, uint8_t* gtig, uint8_t* gtm, int32_t* npig, mi_stream_t st) {
  MI_REQUIRE(T >= 1 && T <= 64 && A >= 1 && max_det >= 0 && ncell >= 0 && N >= 0 && Gt >= 0,
             "coco_match: sizes (T %d of at most 64, A %d, max_det %d, cells %lld, N %lld, G %lld)", T, A, max_det, (long long)ncell,
             (long long)N, (long long)Gt);
  if (ncell == 0) return MI_OK;
  MI_REQUIRE(det_start && gt_start && iou_thrs && area_rng && npig, "coco_match: null");
  MI_REQUIRE(N == 0 || (det_row && det_area && dtm && dtig), "coco_match: null detection tables");
  MI_REQUIRE(Gt == 0 || (gt_col && gt_area && gt_crowd && gtig && gtm), "coco_match: null ground-truth tables");
  MI_REQUIRE(N == 0 || Gt == 0 || iou, "coco_match: null IoU");
  const int64_t blocks = mi_cdiv64(ncell * A, CE_T / 64);
  MI_REQUIRE(blocks < (1LL << 31), "coco_match: %lld cells x %d area ranges", (long long)ncell, A);
  hipStream_t s = (hipStream_t)st;
  if (N) {   // detections beyond max_det of their cell, or of no category, keep zeros
    hipMemsetAsync(dtm, 0, (size_t)A * T * N, s);
    hipMemsetAsync(dtig, 0, (size_t)A * T * N, s);
  }
  hipLaunchKernelGGL(coco_match_kernel, dim3((unsigned)blocks), dim3(CE_T), 0, s, iou, det_row, det_area, det_start, gt_start, gt_col,
                     gt_area, gt_crowd, iou_thrs, T, area_rng, A, max_det, ncell, N, Gt, dtm, dtig, gtig, gtm, npig);
  MI_CHECK_LAUNCH("coco_match");
  return MI_OK;
}

// -------------------------------------------------------------------------------------------------------- accumulate
// thread = (category k, area range a, maxDets m, threshold t).  The detections of k are the slice [cat_start[k],
// cat_start[k + 1]) of the arrays sorted by (k, -score, stable over the concatenation order); those with rank (their place
// in their image's score order) < max_dets[m] enter - a stable sort of a subsequence is the subsequence of the stable sort.
// Forward walk: the two counts (integers, so float64(cumsum) is exact) and recall.  Backward walk: tp / fp of every prefix
// by subtraction, pr = tp / (fp + tp + eps), its running maximum from the right, and for each recall threshold - taken in
// descending order, rc is non-decreasing - the first position with rc >= threshold (np.searchsorted side='left').
__global__ __launch_bounds__(CE_T) void coco_accumulate_kernel(
    const uint8_t* __restrict__ dtm, const uint8_t* __restrict__ dtig, const double* __restrict__ score,
    const int32_t* __restrict__ rank, const int64_t* __restrict__ cat_start, const int64_t* __restrict__ npig,
    const int32_t* __restrict__ max_dets, const double* __restrict__ rec_thrs, int T, int R, int K, int A, int M, int64_t N,
    double* __restrict__ precision, double* __restrict__ recall, double* __restrict__ scores) {
  const int64_t id = (int64_t)blockIdx.x * CE_T + threadIdx.x;
  if (id >= (int64_t)K * A * M * T) return;
  const int t = (int)(id % T), m = (int)(id / T % M), a = (int)(id / T / M % A), k = (int)(id / T / M / A);
  const size_t pstride = (size_t)K * A * M, pbase = (size_t)t * R * pstride + ((size_t)k * A + a) * M + m;
  const size_t rix = (((size_t)t * K + k) * A + a) * M + m;
  const long long np_ = npig[k * A + a];
  if (np_ == 0) {
    recall[rix] = -1.0;
    for (int r = 0; r < R; ++r) { precision[pbase + r * pstride] = -1.0; scores[pbase + r * pstride] = -1.0; }
    return;
  }
  const int64_t s0 = cat_start[k], s1 = cat_start[k + 1];
  const int md = max_dets[m];
  const uint8_t* fm = dtm + ((size_t)a * T + t) * N;
  const uint8_t* fi = dtig + ((size_t)a * T + t) * N;
  long long tp = 0, fp = 0, nd = 0;
  for (int64_t j = s0; j < s1; ++j) {
    if (rank[j] >= md) continue;
    const int mt = fm[j], ig = fi[j];
    ++nd;
    tp += (mt && !ig);
    fp += (!mt && !ig);
  }
  const double npd = (double)np_;
  recall[rix] = nd ? (double)tp / npd : 0.0;
  int ri = R - 1;
  const double rc_last = nd ? (double)tp / npd : -1.0;
  for (; ri >= 0 && rec_thrs[ri] > rc_last; --ri) { precision[pbase + ri * pstride] = 0.0; scores[pbase + ri * pstride] = 0.0; }
  double runmax = 0.0;
  for (int64_t j = s1 - 1; j >= s0 && ri >= 0; --j) {
    if (rank[j] >= md) continue;
    const int mt = fm[j], ig = fi[j];
    const double pr = (double)tp / ((double)fp + (double)tp + DBL_EPSILON);
    runmax = pr > runmax ? pr : runmax;
    tp -= (mt && !ig);
    fp -= (!mt && !ig);
    --nd;
    const double rc_prev = nd ? (double)tp / npd : -1.0;
    const double sc = score[j];
    for (; ri >= 0 && rec_thrs[ri] > rc_prev; --ri) { precision[pbase + ri * pstride] = runmax; scores[pbase + ri * pstride] = sc; }
  }
}

extern "C" int mi_coco_accumulate(const uint8_t* dtm, const uint8_t* dtig, const double* score, const int32_t* rank,
                                  const int64_t* cat_start, const int64_t* npig, const int32_t* max_dets, const double* rec_thrs, int T,
                                  int R, int K, int A, int M, int64_t N, double* precision, double* recall, double* scores,
                                  mi_stream_t st) {
  MI_REQUIRE(T >= 1 && R >= 1 && K >= 0 && A >= 1 && M >= 1 && N >= 0, "coco_accumulate: sizes (T %d, R %d, K %d, A %d, M %d, N %lld)", T,
             R, K, A, M, (long long)N);
  if (K == 0) return MI_OK;
  MI_REQUIRE(cat_start && npig && max_dets && rec_thrs && precision && recall && scores, "coco_accumulate: null");
  MI_REQUIRE(N == 0 || (dtm && dtig && score && rank), "coco_accumulate: null detection tables");
  const int64_t n = (int64_t)K * A * M * T;
  MI_REQUIRE(mi_cdiv64(n, CE_T) < (1LL << 31), "coco_accumulate: %lld cells", (long long)n);
  hipLaunchKernelGGL(coco_accumulate_kernel, dim3((unsigned)mi_cdiv64(n, CE_T)), dim3(CE_T), 0, (hipStream_t)st, dtm, dtig, score, rank,
                     cat_start, npig, max_dets, rec_thrs, T, R, K, A, M, N, precision, recall, scores);
  MI_CHECK_LAUNCH("coco_accumulate");
  return MI_OK;
}
