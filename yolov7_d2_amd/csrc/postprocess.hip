// Batched YOLOX eval postprocess (yolov7/utils/boxes.py:171-210) for all B images in one fixed launch sequence: no host
// sync, no allocation, no memset, so it can sit in a captured graph behind the eval forward.  Every stage reproduces what
// the per-image loop (modeling/postprocess.py:_postprocess_per_image, i.e. torch.max + mask + mi_batched_nms + gather)
// computes, bit for bit:
//   pp_candidates_kernel  corners written back in place (cx -/+ w/2 ...), class maximum (first maximal index, NaN
//                         propagates like torch.max), score = obj * cls_conf, candidate iff score >= conf; wave ballots
//                         give each candidate its position inside its 256-anchor block, the block writes its count
//   pp_compact_kernel     stable per-image compaction (ascending anchor order): the block's offset is the sum of the
//                         counts of the image's earlier blocks; the candidate's detection row (x1,y1,x2,y2,obj,conf,cls)
//                         and score land at candidate index off + local position; the image's coordinate maximum (the
//                         nms_max_kernel value) is an atomicMax on an order-preserving integer encoding
//   pp_rank_kernel        per image: the nms_rank_kernel rank (score descending, ties by ascending candidate index),
//                         scattered with the nms_gather_kernel arithmetic; each image picks its own NMS arithmetic the
//                         way mi_batched_nms does (4 n <= 4000: class offsets idx * (max + 1), else class by class)
//   pp_mask_kernel        the nms_mask_kernel IoU bits over every image's upper-triangular 64 x 64 tiles.  The candidate
//                         counts live on the device, so the grid is fixed (PP_MASK_BLOCKS one-wave blocks) and each wave
//                         walks the flattened list of (image, row chunk, column chunk) tiles built from the counts
//   pp_scan_kernel        the nms_scan_kernel greedy scan, one wave per image, B waves in one launch; kept rows go
//                         straight to dets[b][k][7] in keep order, counts[b] = number kept
// Built with -ffp-contract=off like nms.o: the float expressions keep the loop's operation order.
#include "common.h"

#define PP_T 256             // threads per block of the per-anchor kernels
#define PP_MASK_BLOCKS 4096  // fixed grid of the mask kernel (one wave per block)
#define PP_MAX_A 65536       // mi_batched_nms's limit on n
#define PP_SCAN_BATCH 16     // suppression words the scan loads back to back
#define PP_MAX_B 1024        // images per launch (tile offsets of all images sit in the mask kernel's LDS)

namespace {

struct PPWs {
  uint64_t* mask;   // [B][A * nwA]: image b's rows i < n_b at stride nw_b = ceil(n_b / 64)
  float* crec;      // [B][A][4]: score, cls_conf, cls_idx, local position (int bits; -1: not a candidate)
  float* cdet;      // [B][A][7]: candidate detection rows in candidate order
  float* sboxes;    // [B][A][4]: NMS boxes in rank order (offset form: + cls * (max + 1))
  float* scls;      // [B][A]:    class of rank i
  float* cscore;    // [B][A]:    candidate scores
  int32_t* order;   // [B][A]:    order[rank] = candidate index
  int32_t* blkcnt;  // [B][nb]:   candidates per 256-anchor block
  int32_t* ncand;   // [B]
  uint32_t* maxenc; // [B]:       encoded maximum candidate coordinate
};

int64_t pp_ws_bytes(int64_t B, int64_t A) {
  const int64_t nwA = (A + 63) / 64, nb = (A + PP_T - 1) / PP_T;
  return B * (8 * A * nwA + 4 * A * (4 + 7 + 4 + 1 + 1 + 1) + 4 * nb + 8);
}

PPWs pp_carve(void* ws, int B, int A) {
  const size_t nwA = (size_t)mi_cdiv(A, 64), nb = (size_t)mi_cdiv(A, PP_T), BA = (size_t)B * A;
  PPWs w;
  char* p = (char*)ws;
  w.mask = (uint64_t*)p; p += 8 * BA * nwA;
  w.crec = (float*)p; p += 4 * BA * 4;
  w.cdet = (float*)p; p += 4 * BA * 7;
  w.sboxes = (float*)p; p += 4 * BA * 4;
  w.scls = (float*)p; p += 4 * BA;
  w.cscore = (float*)p; p += 4 * BA;
  w.order = (int32_t*)p; p += 4 * BA;
  w.blkcnt = (int32_t*)p; p += 4 * (size_t)B * nb;
  w.ncand = (int32_t*)p; p += 4 * (size_t)B;
  w.maxenc = (uint32_t*)p;
  return w;
}

}  // namespace

// order-preserving float <-> uint32 (NaN is never encoded: the maximum skips it, as fmaxf does)
__device__ __forceinline__ uint32_t pp_enc(float f) {
  const uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float pp_dec(uint32_t e) {
  return __uint_as_float((e & 0x80000000u) ? (e & 0x7fffffffu) : ~e);
}
__device__ __forceinline__ uint64_t pp_uniform64(uint64_t v) {
  return (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v) |
         ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32)) << 32);
}
__device__ __forceinline__ uint64_t pp_lane64(uint64_t v, int k) {
  return (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, k) |
         ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), k) << 32);
}
__device__ __forceinline__ int pp_cdiv(int a, int b) { return (a + b - 1) / b; }
__device__ __forceinline__ float pp_lane_f(float v, int k) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), k));
}

__global__ __launch_bounds__(PP_T) void pp_candidates_kernel(float* __restrict__ pred, int A, int C, int ld, float conf,
                                                             float* __restrict__ crec, int32_t* __restrict__ blkcnt,
                                                             uint32_t* __restrict__ maxenc) {
  __shared__ int s_wcnt[PP_T / 64];
  const int b = blockIdx.y, a = blockIdx.x * PP_T + threadIdx.x, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  bool cand = false;
  float score = 0.f, cmax = 0.f;
  int cidx = 0;
  if (a < A) {
    float* p = pred + ((size_t)b * A + a) * ld;
    const float cx = p[0], cy = p[1], w = p[2], h = p[3];
    p[0] = cx - w / 2;
    p[1] = cy - h / 2;
    p[2] = cx + w / 2;
    p[3] = cy + h / 2;
    // torch.max(dim): first maximal index; a NaN wins and stays
    cmax = p[5];
    for (int c = 1; c < C; ++c) {
      const float v = p[5 + c];
      if (!(cmax != cmax) && (v > cmax || v != v)) {
        cmax = v;
        cidx = c;
      }
    }
    score = p[4] * cmax;
    cand = score >= conf;
  }
  const uint64_t bal = __ballot(cand);
  if (lane == 0) s_wcnt[wv] = __popcll(bal);
  __syncthreads();
  int pos = __popcll(bal & ((1ull << lane) - 1ull));
  for (int q = 0; q < wv; ++q) pos += s_wcnt[q];
  if (a < A) {
    float* r = crec + ((size_t)b * A + a) * 4;
    r[0] = score;
    r[1] = cmax;
    r[2] = (float)cidx;
    r[3] = __int_as_float(cand ? pos : -1);
  }
  if (threadIdx.x == 0) {
    int tot = 0;
    for (int q = 0; q < PP_T / 64; ++q) tot += s_wcnt[q];
    blkcnt[(size_t)b * gridDim.x + blockIdx.x] = tot;
    if (blockIdx.x == 0) maxenc[b] = pp_enc(-INFINITY);   // read only by the next kernels
  }
}

__global__ __launch_bounds__(PP_T) void pp_compact_kernel(const float* __restrict__ pred, int A, int ld,
                                                          const float* __restrict__ crec, const int32_t* __restrict__ blkcnt,
                                                          float* __restrict__ cdet, float* __restrict__ cscore,
                                                          int32_t* __restrict__ ncand, uint32_t* __restrict__ maxenc) {
  __shared__ int s_red[2][PP_T / 64];
  const int b = blockIdx.y, nb = gridDim.x, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int before = 0, tot = 0;
  for (int j = threadIdx.x; j < nb; j += PP_T) {
    const int v = blkcnt[(size_t)b * nb + j];
    tot += v;
    before += j < (int)blockIdx.x ? v : 0;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    before += __shfl_xor(before, o, 64);
    tot += __shfl_xor(tot, o, 64);
  }
  if (lane == 0) {
    s_red[0][wv] = before;
    s_red[1][wv] = tot;
  }
  __syncthreads();
  before = s_red[0][0] + s_red[0][1] + s_red[0][2] + s_red[0][3];
  if (blockIdx.x == 0 && threadIdx.x == 0) ncand[b] = s_red[1][0] + s_red[1][1] + s_red[1][2] + s_red[1][3];
  const int a = blockIdx.x * PP_T + threadIdx.x;
  float m = -INFINITY;
  if (a < A) {
    const float* r = crec + ((size_t)b * A + a) * 4;
    const int lp = __float_as_int(r[3]);
    if (lp >= 0) {
      const size_t ci = (size_t)b * A + before + lp;
      const float* p = pred + ((size_t)b * A + a) * ld;
      float* d = cdet + ci * 7;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        d[q] = p[q];
        m = fmaxf(m, p[q]);
      }
      d[4] = p[4];
      d[5] = r[1];
      d[6] = r[2];
      cscore[ci] = r[0];
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  if (lane == 0 && m != -INFINITY) atomicMax(maxenc + b, pp_enc(m));
}

// mi_batched_nms's arithmetic choice for n candidates: 1 = coordinate offsets (4 n <= 4000), 0 = class by class
__device__ __forceinline__ int pp_mode(int n) { return (4 * (int64_t)n > 4000) ? 0 : 1; }

__global__ __launch_bounds__(PP_T) void pp_rank_kernel(int A, const float* __restrict__ cdet, const float* __restrict__ cscore,
                                                       const int32_t* __restrict__ ncand, const uint32_t* __restrict__ maxenc,
                                                       int32_t* __restrict__ order, float* __restrict__ sboxes,
                                                       float* __restrict__ scls) {
  const int b = blockIdx.y, n = ncand[b];
  if ((int)blockIdx.x * PP_T >= n) return;   // uniform over the block
  const size_t base = (size_t)b * A;
  const float* sc = cscore + base;
  __shared__ float ss[PP_T];
  const int i = blockIdx.x * PP_T + threadIdx.x;
  const float si = i < n ? sc[i] : 0.f;
  int rank = 0;
  for (int j0 = 0; j0 < n; j0 += PP_T) {
    const int j = j0 + threadIdx.x;
    __syncthreads();
    ss[threadIdx.x] = j < n ? sc[j] : -INFINITY;
    __syncthreads();
    const int lim = min(PP_T, n - j0);
    if (i < n)
      for (int t = 0; t < lim; ++t) {
        const float sj = ss[t];
        rank += (sj > si) || (sj == si && (j0 + t) < i);
      }
  }
  if (i >= n) return;
  order[base + rank] = i;
  const float* d = cdet + (base + i) * 7;
  const float idx = d[6];
  float off = 0.f;
  if (pp_mode(n) == 1) off = idx * (pp_dec(maxenc[b]) + 1.0f);
  float* sb = sboxes + (base + rank) * 4;
#pragma unroll
  for (int q = 0; q < 4; ++q) sb[q] = d[q] + off;
  scls[base + rank] = idx;
}

// mask rows of image b: mask + b * A * nwA, row i at stride nw_b; bit k of word (i, cb): candidate cb*64+k (> i) is
// suppressed by candidate i.  Each wave takes tiles t = blockIdx.x, + gridDim.x, ... of the flat list: image by image,
// row chunk by row chunk, column chunks rb .. nw_b - 1.
__global__ __launch_bounds__(64) void pp_mask_kernel(int B, int A, float thr, const float* __restrict__ sboxes,
                                                     const float* __restrict__ scls, const int32_t* __restrict__ ncand,
                                                     uint64_t* __restrict__ mask) {
  extern __shared__ int s_tp[];   // [B + 1]: first tile of each image
  const int lane = threadIdx.x;
  int carry = 0;
  for (int b0 = 0; b0 < B; b0 += 64) {
    const int b = b0 + lane;
    int nwb = 0;
    if (b < B) nwb = pp_cdiv(ncand[b], 64);
    int v = nwb * (nwb + 1) / 2;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int u = __shfl_up(v, o, 64);
      if (lane >= o) v += u;
    }
    if (b < B) s_tp[b + 1] = carry + v;
    carry += __shfl(v, 63, 64);
  }
  if (lane == 0) s_tp[0] = 0;
  __syncthreads();
  const int total = s_tp[B];
  const size_t nwA = (size_t)pp_cdiv(A, 64);
  for (int t = blockIdx.x; t < total; t += gridDim.x) {
    int lo = 0, hi = B - 1;   // the image: last b with s_tp[b] <= t
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (s_tp[mid] <= t) lo = mid; else hi = mid - 1;
    }
    const int b = lo, n = ncand[b], nw = pp_cdiv(n, 64), k = t - s_tp[b];
    // row chunk rb: tiles before row rb = rb * nw - rb * (rb - 1) / 2
    int rb = (int)((2.0 * nw + 1.0 - sqrt((2.0 * nw + 1.0) * (2.0 * nw + 1.0) - 8.0 * k)) * 0.5);
    rb = max(0, min(rb, nw - 1));
    while (rb + 1 < nw && (rb + 1) * nw - (rb + 1) * rb / 2 <= k) ++rb;
    while (rb > 0 && rb * nw - rb * (rb - 1) / 2 > k) --rb;
    const int cb = rb + (k - (rb * nw - rb * (rb - 1) / 2));
    const int mode = (4 * (int64_t)n > 4000) ? 0 : 1;
    const size_t base = (size_t)b * A;
    const float* sb = sboxes + base * 4;
    const float* scl = scls + base;
    const int cj = cb * 64 + lane;
    float c0 = 0.f, c1 = 0.f, c2 = 0.f, c3 = 0.f, cc = 0.f;
    if (cj < n) {
      c0 = sb[cj * 4 + 0]; c1 = sb[cj * 4 + 1]; c2 = sb[cj * 4 + 2]; c3 = sb[cj * 4 + 3];
      cc = scl[cj];
    }
    const int i = rb * 64 + lane;
    float x1 = 0.f, y1 = 0.f, x2 = 0.f, y2 = 0.f, ci = 0.f;
    if (i < n) {
      x1 = sb[i * 4 + 0]; y1 = sb[i * 4 + 1]; x2 = sb[i * 4 + 2]; y2 = sb[i * 4 + 3];
      ci = scl[i];
    }
    const float ai = (x2 - x1) * (y2 - y1);
    const int lim = min(64, n - cb * 64);
    const int kfirst = rb == cb ? lane + 1 : 0;
    uint64_t bits = 0;
    for (int q = 0; q < lim; ++q) {   // q is wave-uniform: the column box comes from lane q's registers
      const float k0 = pp_lane_f(c0, q), k1 = pp_lane_f(c1, q), k2 = pp_lane_f(c2, q), k3 = pp_lane_f(c3, q);
      const float kc = pp_lane_f(cc, q);
      if (i >= n || q < kfirst) continue;
      if (mode == 0 && kc != ci) continue;
      const float xx1 = fmaxf(x1, k0), yy1 = fmaxf(y1, k1);
      const float xx2 = fminf(x2, k2), yy2 = fminf(y2, k3);
      const float w = fmaxf(0.f, xx2 - xx1), h = fmaxf(0.f, yy2 - yy1);
      const float inter = w * h;
      const float aj = (k2 - k0) * (k3 - k1);
      const float ovr = inter / (ai + aj - inter);
      if (ovr > thr) bits |= 1ull << q;
    }
    if (i < n) mask[base * nwA + (size_t)i * nw + cb] = bits;
  }
}

// one wave per image: the nms_scan_kernel greedy scan; kept candidates' rows go to dets in keep order
__global__ __launch_bounds__(64) void pp_scan_kernel(int A, const uint64_t* __restrict__ mask, const int32_t* __restrict__ order,
                                                     const float* __restrict__ cdet, const int32_t* __restrict__ ncand,
                                                     float* __restrict__ dets, int32_t* __restrict__ counts) {
  extern __shared__ uint64_t removed[];   // [nw]
  const int b = blockIdx.x, lane = threadIdx.x, n = ncand[b], nw = pp_cdiv(n, 64);
  const size_t base = (size_t)b * A;
  const uint64_t* mk = mask + base * (size_t)pp_cdiv(A, 64);
  for (int w = lane; w < nw; w += 64) removed[w] = 0;
  __syncthreads();
  int nk = 0;
  for (int c = 0; c < nw; ++c) {
    const int i = c * 64 + lane;
    const uint64_t diag = (i < n) ? mk[(size_t)i * nw + c] : 0ull;
    // the chunk is resolved with wave-uniform values: rem and kept live in scalar registers, lane k's diagonal word
    // is read with v_readlane (k is uniform), not a 64-bit shuffle per step
    uint64_t rem = pp_uniform64(removed[c]);
    if (n - c * 64 < 64) rem |= ~0ull << (n - c * 64);   // lanes beyond n are "removed"
    uint64_t kept = 0;
    for (int k = 0; k < 64; ++k) {
      const uint64_t dk = pp_lane64(diag, k);
      if (!((rem >> k) & 1ull)) {
        kept |= 1ull << k;
        rem |= dk;
      }
    }
    if ((kept >> lane) & 1ull) {
      const int pos = nk + __popcll(kept & ((1ull << lane) - 1ull));
      const float* src = cdet + (base + order[base + i]) * 7;
      float* dst = dets + (base + pos) * 7;
#pragma unroll
      for (int q = 0; q < 7; ++q) dst[q] = src[q];
    }
    nk += __popcll(kept);
    // OR the kept rows into the later words of the removed bitmap (lane-distributed); the rows' words are loaded
    // PP_SCAN_BATCH at a time so their latencies overlap instead of adding up
    for (int w = c + 1 + lane; w < nw; w += 64) {
      const uint64_t* col = mk + (size_t)c * 64 * nw + w;
      uint64_t r = removed[w];
      uint64_t kk = kept;
      while (kk) {
        uint64_t v[PP_SCAN_BATCH];
#pragma unroll
        for (int u = 0; u < PP_SCAN_BATCH; ++u) {
          v[u] = 0;
          if (kk) {
            const int k = __ffsll((long long)kk) - 1;
            kk &= kk - 1;
            v[u] = col[(size_t)k * nw];
          }
        }
#pragma unroll
        for (int u = 0; u < PP_SCAN_BATCH; ++u) r |= v[u];
      }
      removed[w] = r;
    }
    __syncthreads();
  }
  if (lane == 0) counts[b] = nk;
}

extern "C" int64_t mi_yolox_postprocess_ws_bytes(int B, int A, int C) {
  MI_REQUIRE(B >= 0 && B <= PP_MAX_B && A >= 1 && A <= PP_MAX_A && C >= 1,
             "yolox_postprocess_ws_bytes: B %d (0 .. %d), A %d (1 .. %d), C %d (>= 1)", B, PP_MAX_B, A, PP_MAX_A, C);
  return pp_ws_bytes(B, A);
}

extern "C" int mi_yolox_postprocess(float* pred, int B, int A, int C, int ld, float conf_thr, float nms_thr, float* dets,
                                    int32_t* counts, void* ws, int64_t ws_bytes, mi_stream_t st) {
  MI_REQUIRE(pred && dets && counts && ws, "yolox_postprocess: null");
  MI_REQUIRE(B >= 0 && B <= PP_MAX_B, "yolox_postprocess: B %d (0 .. %d per launch)", B, PP_MAX_B);
  MI_REQUIRE(A >= 1 && A <= PP_MAX_A, "yolox_postprocess: A %d (1 .. %d)", A, PP_MAX_A);
  MI_REQUIRE(C >= 1 && ld >= 5 + C, "yolox_postprocess: C %d (>= 1), row length %d (>= 5 + C)", C, ld);
  MI_REQUIRE(ws_bytes >= pp_ws_bytes(B, A), "yolox_postprocess: workspace %lld bytes, %lld needed", (long long)ws_bytes,
             (long long)pp_ws_bytes(B, A));
  MI_REQUIRE(((uintptr_t)ws & 7) == 0, "yolox_postprocess: workspace not 8-byte aligned");
  if (B == 0) return MI_OK;
  hipStream_t s = (hipStream_t)st;
  const PPWs w = pp_carve(ws, B, A);
  const int nb = mi_cdiv(A, PP_T), nwA = mi_cdiv(A, 64);
  hipLaunchKernelGGL(pp_candidates_kernel, dim3(nb, B), dim3(PP_T), 0, s, pred, A, C, ld, conf_thr, w.crec, w.blkcnt,
                     w.maxenc);
  hipLaunchKernelGGL(pp_compact_kernel, dim3(nb, B), dim3(PP_T), 0, s, pred, A, ld, w.crec, w.blkcnt, w.cdet, w.cscore,
                     w.ncand, w.maxenc);
  hipLaunchKernelGGL(pp_rank_kernel, dim3(nb, B), dim3(PP_T), 0, s, A, w.cdet, w.cscore, w.ncand, w.maxenc, w.order,
                     w.sboxes, w.scls);
  hipLaunchKernelGGL(pp_mask_kernel, dim3(PP_MASK_BLOCKS), dim3(64), (B + 1) * sizeof(int), s, B, A, nms_thr, w.sboxes,
                     w.scls, w.ncand, w.mask);
  hipLaunchKernelGGL(pp_scan_kernel, dim3(B), dim3(64), nwA * sizeof(uint64_t), s, A, w.mask, w.order, w.cdet, w.ncand,
                     dets, counts);
  MI_CHECK_LAUNCH("yolox_postprocess");
  return MI_OK;
}
