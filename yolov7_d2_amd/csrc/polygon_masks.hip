// Polygon ground-truth masks rasterised on the device: what the reference's SparseInst does on the host, one instance at a
// time, with pycocotools (meta_arch/sparseinst.py:111-115: BitMasks.from_polygon_masks -> polygons_to_bitmask = frPyObjects,
// merge, decode) - here one launch per batch from the uploaded vertices, bit for bit the same masks.
//
// rleFrPoly in the kernel's terms (all fp64, C casts truncate; this file is compiled with -ffp-contract=off: ys + s * t + 0.5
// as a fused multiply-add rounds differently at exact ties):
//   * vertices are upsampled by 5: X = (int)(5 x + 0.5), Y = (int)(5 y + 0.5); the ring is closed.
//   * an edge is walked along its longer axis from its smaller end (the ends are swapped when it runs backwards) in
//     max(dx, dy) unit steps t; the other coordinate is (int)(start + s * t + 0.5), s = (double)(difference) / max(dx, dy).
//   * two consecutive points whose u differ are a CROSSING of the line between u = m and m + 1, m = min of the two; it
//     counts when m = 5 x + 2 for a column 0 <= x <= w - 1 (that is floor(xd) == xd for xd = (m + 0.5) / 5 - 0.5), at the row
//     ceil(clamp((min(v) + 0.5) / 5 - 0.5, 0, h)) - 0 .. h inclusive.  A crossing is symmetric in its two points, so the
//     direction the original walks the edge in does not matter; consecutive edges join in one point, so crossings belong to
//     one edge and one step; an edge of length zero has no step (its s = 0 / 0 is never formed).
//   * the RLE is the sorted crossings in column-major order, i.e. pixel (y, x) is set iff the number of crossings at or before
//     it is odd.  A closed ring crosses every line an even number of times, so the parity restarts in every column: the
//     fill of a column is the prefix parity of its own h + 1 toggle bits (bit h, the "top of the next column", sets nothing).
//
// A block owns (image, instance, strip of POLY_STRIP columns).  Per ring: every thread takes one edge and drops it unless its
// x-range meets the strip; the surviving edges go through LDS to the waves, one edge per wave, lanes over the steps (over
// the strip's columns for an edge walked along x, where only every fifth step can count).  Crossings are XORed into
// (h + 1) toggle bits per column in LDS; a prefix-XOR with carry turns them into the ring's fill, which is ORed into the
// instance's plane (the union of merge).  The plane leaves row-major, four pixels per store.  No global scratch, no global
// atomics; XOR and OR commute, so the bytes do not depend on the order the waves arrive in.
#include "common.h"
#include <cstring>

#define POLY_STRIP 64
#define POLY_LIST 256      // edges looked at per pass = threads per block

struct PolyImgK {
  const double* verts;
  const int* ring_off;
  const int* inst_off;
  uint8_t* out;
  int M, h, w, pad_;
};
struct PolyK {
  PolyImgK j[MI_FEED_MAX_IMAGES];
};

__global__ __launch_bounds__(256) void polygon_masks_kernel(const PolyK p) {
  extern __shared__ uint32_t plane[];             // [2][POLY_STRIP][nwp]: toggles of the ring, fill of the instance
  __shared__ int elist[POLY_LIST][4];             // surviving edges (xs, ys, xe, ye), ends already in walking order
  __shared__ int ecount;
  const PolyImgK jb = p.j[blockIdx.z];
  const int inst = blockIdx.y;
  const int c0 = blockIdx.x * POLY_STRIP;
  if (inst >= jb.M || c0 >= jb.w) return;
  const int h = jb.h, w = jb.w;
  const int nc = w - c0 < POLY_STRIP ? w - c0 : POLY_STRIP;
  const int nw = (h + 1 + 31) >> 5, nwp = nw | 1;      // odd stride: the columns of a word fall into different banks
  uint32_t* const tog = plane;
  uint32_t* const acc = plane + POLY_STRIP * nwp;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int i = tid; i < 2 * POLY_STRIP * nwp; i += 256) plane[i] = 0;
  if (tid == 0) ecount = 0;
  __syncthreads();
  // crossings of this strip lie on the lines m = 5 x + 2, x = c0 .. c0 + nc - 1
  const int mlo = 5 * c0 + 2, mhi = 5 * (c0 + nc - 1) + 2;

  for (int r = jb.inst_off[inst]; r < jb.inst_off[inst + 1]; ++r) {
    const int v0 = jb.ring_off[r], k = jb.ring_off[r + 1] - v0;
    const double* const xy = jb.verts + 2 * (int64_t)v0;
    for (int base = 0; base < k; base += POLY_LIST) {
      const int e = base + tid;
      if (e < k) {
        const int e1 = e + 1 < k ? e + 1 : 0;
        int xs = (int)(5.0 * xy[2 * e] + 0.5), ys = (int)(5.0 * xy[2 * e + 1] + 0.5);
        int xe = (int)(5.0 * xy[2 * e1] + 0.5), ye = (int)(5.0 * xy[2 * e1 + 1] + 0.5);
        const int dx = abs(xe - xs), dy = abs(ye - ys);
        if ((dx >= dy && xs > xe) || (dx < dy && ys > ye)) {
          int t = xs; xs = xe; xe = t;
          t = ys; ys = ye; ye = t;
        }
        // (the truncating cast can put a point of negative coordinate one unit beside the segment: two units of margin)
        const int lo = (xs < xe ? xs : xe) - 2, hi = (xs < xe ? xe : xs) + 2;
        if ((dx | dy) != 0 && hi >= mlo && lo <= mhi) {
          const int at = atomicAdd(&ecount, 1);
          elist[at][0] = xs; elist[at][1] = ys; elist[at][2] = xe; elist[at][3] = ye;
        }
      }
      __syncthreads();
      const int ne = ecount;
      for (int i = wave; i < ne; i += 4) {
        const int xs = elist[i][0], ys = elist[i][1], xe = elist[i][2], ye = elist[i][3];
        const int dx = abs(xe - xs), dy = abs(ye - ys);
        if (dx >= dy) {
          // walked along x (xs <= xe): u = xs + t, so the line m is crossed by the step t = m - xs -> t + 1, 0 <= t < dx
          const double s = (double)(ye - ys) / dx;
          if (lane < nc) {
            const int t = mlo + 5 * lane - xs;
            if (t >= 0 && t < dx) {
              const int va = (int)(ys + s * t + 0.5), vb = (int)(ys + s * (t + 1) + 0.5);
              double yd = (double)(va < vb ? va : vb);
              yd = (yd + 0.5) / 5.0 - 0.5;
              if (yd < 0) yd = 0; else if (yd > h) yd = h;
              const int yi = (int)ceil(yd);
              atomicXor(&tog[lane * nwp + (yi >> 5)], 1u << (yi & 31));
            }
          }
        } else {
          // walked along y (ys < ye): v = ys + t, u = (int)(xs + s t + 0.5) moves by at most one per step
          const double s = (double)(xe - xs) / dy;
          for (int t = lane; t < dy; t += 64) {
            const int ua = (int)(xs + s * t + 0.5), ub = (int)(xs + s * (t + 1) + 0.5);
            if (ua == ub) continue;
            const int m = ua < ub ? ua : ub;
            if (m < mlo || m > mhi || (m - 2) % 5 != 0) continue;
            double yd = (double)(ys + t);          // min(v) of the two points
            yd = (yd + 0.5) / 5.0 - 0.5;
            if (yd < 0) yd = 0; else if (yd > h) yd = h;
            const int yi = (int)ceil(yd);
            atomicXor(&tog[((m - 2) / 5 - c0) * nwp + (yi >> 5)], 1u << (yi & 31));
          }
        }
      }
      __syncthreads();
      if (tid == 0) ecount = 0;
      __syncthreads();
    }
    // toggles -> fill: bit y of a column = parity of its toggles 0 .. y (prefix-XOR inside the word, carry between words)
    if (tid < nc) {
      uint32_t carry = 0;
      for (int q = 0; q < nw; ++q) {
        uint32_t v = tog[tid * nwp + q];
        v ^= v << 1; v ^= v << 2; v ^= v << 4; v ^= v << 8; v ^= v << 16;
        v ^= carry;
        carry = (v >> 31) ? 0xffffffffu : 0u;
        acc[tid * nwp + q] |= v;
        tog[tid * nwp + q] = 0;
      }
    }
    __syncthreads();
  }

  // the strip leaves row-major: a thread = 4 consecutive columns of one row
  uint8_t* const out = jb.out + (int64_t)inst * h * w;
  const bool vec = (w & 3) == 0 && ((uintptr_t)jb.out & 3) == 0;
  const int g = tid & 15;
  for (int y = tid >> 4; y < h; y += 16) {
    const int q = y >> 5, sh = y & 31;
    uint32_t b[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) b[e] = (acc[(g * 4 + e) * nwp + q] >> sh) & 1u;      // (columns >= nc stayed zero)
    uint8_t* const dst = out + (int64_t)y * w + c0 + g * 4;
    if (vec) {
      if (g * 4 < nc) *(uint32_t*)dst = b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24);
    } else {
      for (int e = 0; e < 4 && g * 4 + e < nc; ++e) dst[e] = (uint8_t)b[e];
    }
  }
}

extern "C" int mi_polygon_masks(const mi_poly_job* jobs, int B, mi_stream_t st) {
  MI_REQUIRE(jobs && B >= 1, "polygon_masks: args");
  int maxM = 0, maxW = 0, maxH = 0;
  for (int b = 0; b < B; ++b) {
    const mi_poly_job& j = jobs[b];
    MI_REQUIRE(j.M >= 0, "polygon_masks: image %d: %d instances", b, j.M);
    if (j.M == 0) continue;
    MI_REQUIRE(j.h >= 1 && j.w >= 1, "polygon_masks: image %d: %d x %d", b, j.h, j.w);
    MI_REQUIRE(j.M <= 65535, "polygon_masks: image %d: %d instances exceed the grid", b, j.M);
    MI_REQUIRE(j.h <= MI_POLY_MAX_H, "polygon_masks: image %d: height %d exceeds the LDS plan (%d rows)", b, j.h, MI_POLY_MAX_H);
    MI_REQUIRE(j.verts && j.ring_off && j.inst_off && j.ring_off_host && j.inst_off_host && j.out,
               "polygon_masks: image %d: null pointer", b);
    MI_REQUIRE(j.inst_off_host[0] == 0 && j.ring_off_host[0] == 0, "polygon_masks: image %d: offsets start at 0", b);
    for (int i = 0; i < j.M; ++i)
      MI_REQUIRE(j.inst_off_host[i + 1] > j.inst_off_host[i], "polygon_masks: image %d: instance %d has no ring", b, i);
    for (int r = 0; r < j.inst_off_host[j.M]; ++r)
      MI_REQUIRE(j.ring_off_host[r + 1] - j.ring_off_host[r] >= 3, "polygon_masks: image %d: ring %d has %d vertices (< 3)", b, r,
                 j.ring_off_host[r + 1] - j.ring_off_host[r]);
    if (j.M > maxM) maxM = j.M;
    if (j.w > maxW) maxW = j.w;
    if (j.h > maxH) maxH = j.h;
  }
  if (maxM == 0) return MI_OK;
  for (int b0 = 0; b0 < B; b0 += MI_FEED_MAX_IMAGES) {
    PolyK k;
    memset(&k, 0, sizeof(k));
    const int nb = B - b0 < MI_FEED_MAX_IMAGES ? B - b0 : MI_FEED_MAX_IMAGES;
    int gm = 0, gw = 0, gh = 0;
    for (int b = 0; b < nb; ++b) {
      const mi_poly_job& j = jobs[b0 + b];
      k.j[b].verts = j.verts; k.j[b].ring_off = j.ring_off; k.j[b].inst_off = j.inst_off; k.j[b].out = (uint8_t*)j.out;
      k.j[b].M = j.M; k.j[b].h = j.h; k.j[b].w = j.w;
      if (j.M == 0) continue;
      if (j.M > gm) gm = j.M;
      if (j.w > gw) gw = j.w;
      if (j.h > gh) gh = j.h;
    }
    if (gm == 0) continue;
    // the planes are sized for the tallest image of the launch (a block indexes them with its own image's stride)
    const size_t lds = (size_t)2 * POLY_STRIP * (((gh + 1 + 31) >> 5) | 1) * sizeof(uint32_t);
    hipLaunchKernelGGL(polygon_masks_kernel, dim3((gw + POLY_STRIP - 1) / POLY_STRIP, gm, nb), dim3(256), lds, (hipStream_t)st, k);
    MI_CHECK_LAUNCH("polygon_masks");
  }
  return MI_OK;
}
