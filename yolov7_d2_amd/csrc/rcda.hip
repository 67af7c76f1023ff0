// Row-column decoupled attention (Anchor DETR's MultiheadRCDA core), forward + backward, on the gfx950 matrix cores.
//
//   A_row[q, w] = softmax over w of scale * Qr[q] . Kr[w]   (mask_row[w] = 1: -inf)          per (batch, head), head_dim = 32
//   A_col[q, h] = softmax over h of scale * Qc[q] . Kc[h]   (mask_col[h] = 1: -inf)
//   O[q, :]     = sum over (h, w) of A_col[q, h] * A_row[q, w] * V[h, w, :]
//
// (yolov7/modeling/backbone/layers/row_column_decoupled_attention.py:184-257).  The reference forms the [B * heads, L, W, 32]
// partial sum over h in HBM (77 MB per layer at B 4, L 900, 25 x 42) and keeps it for the backward; here the product of the two
// softmaxes P[q, (h, w)] = A_col A_row is the weight matrix of an attention with H * W keys that never leaves registers: it is
// formed per h from the two normalised rows, rounded to bf16 once and multiplied into V[h] on the matrix cores.
//
// Layouts (batch first, as the module's inputs are): q_row, q_col, o, dout bf16 [B][L] rows; k_row bf16 [B][W] rows, k_col
// bf16 [B][H] rows (the projected key means); v bf16 [B][H][W] rows; a row has E = heads * 32 channels at its row stride, head n
// owns channels [32 n, 32 n + 32).  mask_row uint8 [B][W], mask_col uint8 [B][H], 1 = padded.  lse_row, lse_col fp32
// [B][heads][L] in BASE-2 units: log2 of the sum over live keys of exp2(score * scale * log2(e)); -inf for a query whose keys
// are all padded (its weights are 0: O = 0, no gradient).
//
// MFMA plan (v_mfma_f32_16x16x32_bf16; head_dim 32 = one k step of a score product), the fragment layouts of mha.hip:
//   scores     S^T tile = K rows (A: [16 keys][32 d]) x Q^T (B)  -> lane (t = query, g) holds keys 16 a + 4 g + r: a softmax row
//              needs two cross-lane steps, and two such tiles are the A fragment (8 key slots of 32) of the next product
//   forward    O += P_h (A: [16 q][32 w slots]) x V[h] (B: transpose read of a row-major LDS tile), for every h
//   backward   T^T tile = V[h] rows (A) x dO^T (B) in the same lane layout as A_row: dA_row += A_col[h] T, dA_col[h] = A_row . T
//              dQ = dS (A) x K (B, transpose read);  dK = dS^T (A, from the workspace) x Q (B);  dV[h] = P_h^T (A) x dO (B)
// A wave owns 16 queries (forward, query side of the backward), 16 keys (dK) or 16 columns w of a few rows h (dV).  Every sum
// over queries runs in a fixed order: no atomics, two runs give the same bits.
#include <stdlib.h>
#include <string.h>
#include "common.h"
#include "mfma_tile.h"   // tile_off, frag_rows, frag_cols: the LDS tile and fragment layouts shared with mha.hip

#define RC_D 32
#define RC_MAX 96              // served map side: H, W <= 96 (a dilated C5 map at 800 x 1333 is 50 x 84)
#define RC_NT (RC_MAX / 16)    // score tiles of 16 keys per softmax row
#define RC_VROWS 192           // rows of V per LDS buffer: HC = RC_VROWS / (32 ceil(W / 32)) map rows h per chunk
#define RC_LOG2E 1.44269504088896341f

typedef mi_rcda_desc RcK;

__device__ __forceinline__ f32x4 rc_mfma(bf16x8 a, bf16x8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }
__device__ __forceinline__ float rc_sum_g(float v) {   // sum over the four lane groups g of a query / key t, in a fixed order
  v += __shfl_xor(v, 16, 64);
  v += __shfl_xor(v, 32, 64);
  return v;
}

// One softmax row per query of the wave: keys = the n rows of kb (bf16, row stride ldk, this head's 32 channels at kb), mask
// (n bytes or NULL).  x = score * sc2 in the exp2 domain, -inf for a padded key or a key >= n.
//   FROM_LSE = false: a = exp2(x - max) / sum, *lse = max + log2(sum)   (-inf and a = 0 when no key is live)
//   FROM_LSE = true : a = exp2(x - *lse)                                  (*lse = +inf: a row that weighs nothing)
// lane (t = query, g): a[i][r] belongs to key 16 i + 4 g + r; entries of tiles >= nt are 0.
template <bool FROM_LSE>
__device__ __forceinline__ void rc_probs(const __bf16* kb, int ldk, int n, int nt, const uint8_t* mask, bf16x8 qf, int t, int g,
                                         float sc2, float (&a)[RC_NT][4], float* lse) {
  float m = -INFINITY;
#pragma unroll
  for (int i = 0; i < RC_NT; ++i) {
    if (i < nt) {
      const int row = 16 * i + t;
      const bf16x8 kf = *(const bf16x8*)(kb + (size_t)(row < n ? row : n - 1) * ldk + g * 8);
      const f32x4 s = rc_mfma(kf, qf, f32x4{0.f, 0.f, 0.f, 0.f});
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int key = 16 * i + 4 * g + r;
        const bool dead = key >= n || (mask && mask[key < n ? key : n - 1]);
        a[i][r] = dead ? -INFINITY : s[r] * sc2;
        m = fmaxf(m, a[i][r]);
      }
    } else {
#pragma unroll
      for (int r = 0; r < 4; ++r) a[i][r] = -INFINITY;
    }
  }
  if constexpr (FROM_LSE) {
    const float l = *lse;
#pragma unroll
    for (int i = 0; i < RC_NT; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) a[i][r] = a[i][r] == -INFINITY ? 0.f : __builtin_amdgcn_exp2f(a[i][r] - l);
  } else {
    m = fmaxf(m, __shfl_xor(m, 16, 64));
    m = fmaxf(m, __shfl_xor(m, 32, 64));
    float l = 0.f;
#pragma unroll
    for (int i = 0; i < RC_NT; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        a[i][r] = a[i][r] == -INFINITY ? 0.f : __builtin_amdgcn_exp2f(a[i][r] - m);
        l += a[i][r];
      }
    l = rc_sum_g(l);
    const float inv = l > 0.f ? 1.f / l : 0.f;
#pragma unroll
    for (int i = 0; i < RC_NT; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) a[i][r] *= inv;
    *lse = l > 0.f ? m + log2f(l) : -INFINITY;
  }
}

// V of (batch b, head) streams through LDS in chunks of HC map rows; a map row is nW32 tiles of 32 columns (columns >= W and
// rows >= H repeat the last one: finite values whose weight is exactly 0).  256 threads, 3 pieces of 16 bytes each.
struct RcVStage {
  const __bf16* src[3];   // this thread's pieces of chunk 0 (rows clamped), advanced by HC map rows per chunk
  int hh[3], off[3];      // map row inside the chunk and LDS byte offset
  u32x4 reg[3];
  const __bf16* vb;
  int H, W, ldv, HC;
  __device__ __forceinline__ void init(const RcK& p, int b, int head, int nW32, int HC_, int tid) {
    H = p.H; W = p.W; ldv = p.ldv; HC = HC_;
    vb = (const __bf16*)p.v + (size_t)b * p.H * p.W * p.ldv + head * RC_D;
    const int WP = 32 * nW32;
#pragma unroll
    for (int u = 0; u < 3; ++u) {
      int idx = tid + u * 256;
      const int last = HC * WP * 4 - 1;
      idx = idx < last ? idx : last;
      const int row = idx >> 2, piece = idx & 3;
      hh[u] = row / WP;
      const int w = row - hh[u] * WP;
      off[u] = (row >> 5) * 2048 + tile_off(row & 31, piece);
      src[u] = vb + (size_t)(w < W ? w : W - 1) * ldv + piece * 8;
    }
  }
  __device__ __forceinline__ void load(int c) {
#pragma unroll
    for (int u = 0; u < 3; ++u) {
      int h = c * HC + hh[u];
      h = h < H ? h : H - 1;
      reg[u] = *(const u32x4*)(src[u] + (size_t)h * W * ldv);
    }
  }
  __device__ __forceinline__ void store(char* buf) const {
#pragma unroll
    for (int u = 0; u < 3; ++u) *(u32x4*)(buf + off[u]) = reg[u];
  }
};

// ------------------------------------------------------------------ key means
// mean_row[b][w][:] = mean over h of key_row[b][h][w][:], mean_col[b][h][:] = mean over w of key_col[b][h][w][:]: fp32 sums in
// index order, one division, one rounding.  A thread owns 8 channels of one output row.
__global__ __launch_bounds__(256) void rc_key_mean_kernel(const __bf16* kr, const __bf16* kc, __bf16* mr, __bf16* mc, int B, int H,
                                                          int W, int E) {
  const int E8 = E >> 3;
  const long long nrow = kr ? (long long)B * W * E8 : 0, ncol = kc ? (long long)B * H * E8 : 0;
  long long i = blockIdx.x * 256LL + threadIdx.x;
  if (i >= nrow + ncol) return;
  const bool col = i >= nrow;
  if (col) i -= nrow;
  const int c8 = (int)(i % E8);
  const long long rowi = i / E8;               // b * W + w  or  b * H + h
  const int n = col ? W : H;
  const __bf16* src;
  size_t step;
  if (col) {
    src = kc + (size_t)rowi * W * E + c8 * 8;
    step = E;
  } else {
    const long long b = rowi / W, w = rowi % W;
    src = kr + ((size_t)b * H * W + w) * E + c8 * 8;
    step = (size_t)W * E;
  }
  float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int k = 0; k < n; ++k) {
    const bf16x8 x = *(const bf16x8*)(src + k * step);
#pragma unroll
    for (int e = 0; e < 8; ++e) s[e] += (float)x[e];
  }
  bf16x8 o;
#pragma unroll
  for (int e = 0; e < 8; ++e) o[e] = (__bf16)(s[e] / (float)n);
  *(bf16x8*)((col ? mc : mr) + (size_t)rowi * E + c8 * 8) = o;
}

// ------------------------------------------------------------------ forward
__global__ __launch_bounds__(256) void rc_fwd_kernel(const RcK p) {
  __shared__ __attribute__((aligned(16))) char Vs[2][RC_VROWS * 64];
  __shared__ float Ac[4][RC_MAX * 16];      // per wave: A_col[h][query t]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int t = lane & 15, g = lane >> 4;
  const int bh = blockIdx.y, b = bh / p.heads, head = bh % p.heads;
  const int q0 = blockIdx.x * 64 + wave * 16, myq = q0 + t;
  const int nWt = (p.W + 15) >> 4, nHt = (p.H + 15) >> 4, nW32 = (p.W + 31) >> 5;
  const int HC = RC_VROWS / (32 * nW32), nchunks = (p.H + HC - 1) / HC;
  const float sc2 = p.scale * RC_LOG2E;
  RcVStage vs;
  vs.init(p, b, head, nW32, HC, tid);
  vs.load(0);
  bf16x8 qr = {}, qc = {};
  if (myq < p.L) {
    const size_t rb = ((size_t)b * p.L + myq) * p.ldq + head * RC_D + g * 8;
    qr = *(const bf16x8*)((const __bf16*)p.q_row + rb);
    qc = *(const bf16x8*)((const __bf16*)p.q_col + rb);
  }
  float arow[RC_NT][4], acol[RC_NT][4], lr, lc;
  rc_probs<false>((const __bf16*)p.k_row + (size_t)b * p.W * p.ldk + head * RC_D, p.ldk, p.W, nWt,
                  p.mask_row ? p.mask_row + (size_t)b * p.W : nullptr, qr, t, g, sc2, arow, &lr);
  rc_probs<false>((const __bf16*)p.k_col + (size_t)b * p.H * p.ldk + head * RC_D, p.ldk, p.H, nHt,
                  p.mask_col ? p.mask_col + (size_t)b * p.H : nullptr, qc, t, g, sc2, acol, &lc);
  if (g == 0 && myq < p.L) {
    p.lse_row[(size_t)bh * p.L + myq] = lr;
    p.lse_col[(size_t)bh * p.L + myq] = lc;
  }
#pragma unroll
  for (int i = 0; i < RC_NT; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) Ac[wave][(16 * i + 4 * g + r) * 16 + t] = acol[i][r];
  vs.store(Vs[0]);
  f32x4 acc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};   // [d group]: lane (t = d, g): queries 4g + r
  for (int c = 0; c < nchunks; ++c) {
    __syncthreads();   // chunk c is visible; the other buffer is no longer read
    const char* V = Vs[c & 1];
    if (c + 1 < nchunks) vs.load(c + 1);
    for (int hh = 0; hh < HC; ++hh) {
      const int h = c * HC + hh;
      if (h >= p.H) break;
      const float ah = Ac[wave][h * 16 + t];
#pragma unroll
      for (int t2 = 0; t2 < RC_NT / 2; ++t2) {
        if (t2 < nW32) {
          bf16x8 pf;
#pragma unroll
          for (int e = 0; e < 8; ++e) pf[e] = (__bf16)(ah * arow[2 * t2 + (e >> 2)][e & 3]);
          const char* T = V + (hh * nW32 + t2) * 2048;
#pragma unroll
          for (int j = 0; j < 2; ++j) acc[j] = rc_mfma(pf, frag_cols(T, j, t, g), acc[j]);
        }
      }
    }
    if (c + 1 < nchunks) vs.store(Vs[(c + 1) & 1]);
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int qq = q0 + 4 * g + r;
    if (qq < p.L) {
      __bf16* op = (__bf16*)p.o + ((size_t)b * p.L + qq) * p.ldo + head * RC_D;
      op[t] = (__bf16)acc[0][r];
      op[16 + t] = (__bf16)acc[1][r];
    }
  }
}

// ------------------------------------------------------------------ backward, query side
// Recomputes A_row, A_col from the saved lse, streams V as the forward does and forms T = dO . V[h, w] tile by tile:
//   dA_row[q, w] += A_col[q, h] T      dA_col[q, h] = sum over w of A_row[q, w] T
// delta = sum over w of A_row dA_row (= dO . O of the exact output, the same number for both softmaxes), dS = A (dA - delta).
// Writes dQr = scale dS_row Kr, dQc = scale dS_col Kc and dS_row^T, dS_col^T (bf16 [B heads][W or H][Lp]) for the key side.
__global__ __launch_bounds__(256) void rc_bwd_q_kernel(const RcK p, __bf16* wsr, __bf16* wsc, int Lp) {
  __shared__ __attribute__((aligned(16))) char Vs[2][RC_VROWS * 64];
  __shared__ __attribute__((aligned(16))) char Krs[RC_MAX * 64], Kcs[RC_MAX * 64];
  __shared__ float Ac[4][RC_MAX * 16];      // per wave: A_col[h][query t], overwritten by dA_col[h][t] once h is done
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int t = lane & 15, g = lane >> 4;
  const int bh = blockIdx.y, b = bh / p.heads, head = bh % p.heads;
  const int q0 = blockIdx.x * 64 + wave * 16, myq = q0 + t;
  const int nWt = (p.W + 15) >> 4, nHt = (p.H + 15) >> 4, nW32 = (p.W + 31) >> 5, nH32 = (p.H + 31) >> 5;
  const int HC = RC_VROWS / (32 * nW32), nchunks = (p.H + HC - 1) / HC;
  const float sc2 = p.scale * RC_LOG2E;
  const __bf16* krb = (const __bf16*)p.k_row + (size_t)b * p.W * p.ldk + head * RC_D;
  const __bf16* kcb = (const __bf16*)p.k_col + (size_t)b * p.H * p.ldk + head * RC_D;
  RcVStage vs;
  vs.init(p, b, head, nW32, HC, tid);
  vs.load(0);
  // Kr, Kc as LDS tiles for the transpose reads of dQ (rows past the last key are zero)
  for (int idx = tid; idx < RC_MAX * 4; idx += 256) {
    const int row = idx >> 2, piece = idx & 3;
    u32x4 a = {0u, 0u, 0u, 0u}, c = {0u, 0u, 0u, 0u};
    if (row < p.W) a = *(const u32x4*)(krb + (size_t)row * p.ldk + piece * 8);
    if (row < p.H) c = *(const u32x4*)(kcb + (size_t)row * p.ldk + piece * 8);
    const int o = (row >> 5) * 2048 + tile_off(row & 31, piece);
    *(u32x4*)(Krs + o) = a;
    *(u32x4*)(Kcs + o) = c;
  }
  bf16x8 qr = {}, qc = {}, dof = {};
  float lr = INFINITY, lc = INFINITY;     // (a query past L or with no live key weighs nothing)
  if (myq < p.L) {
    const size_t rb = ((size_t)b * p.L + myq) * p.ldq + head * RC_D + g * 8;
    qr = *(const bf16x8*)((const __bf16*)p.q_row + rb);
    qc = *(const bf16x8*)((const __bf16*)p.q_col + rb);
    dof = *(const bf16x8*)((const __bf16*)p.dout + ((size_t)b * p.L + myq) * p.ldo + head * RC_D + g * 8);
    lr = p.lse_row[(size_t)bh * p.L + myq];
    lc = p.lse_col[(size_t)bh * p.L + myq];
    if (lr == -INFINITY || lc == -INFINITY) lr = lc = INFINITY;
  }
  float arow[RC_NT][4], acol[RC_NT][4], dar[RC_NT][4];
  rc_probs<true>(krb, p.ldk, p.W, nWt, p.mask_row ? p.mask_row + (size_t)b * p.W : nullptr, qr, t, g, sc2, arow, &lr);
  rc_probs<true>(kcb, p.ldk, p.H, nHt, p.mask_col ? p.mask_col + (size_t)b * p.H : nullptr, qc, t, g, sc2, acol, &lc);
#pragma unroll
  for (int i = 0; i < RC_NT; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      Ac[wave][(16 * i + 4 * g + r) * 16 + t] = acol[i][r];
      dar[i][r] = 0.f;
    }
  vs.store(Vs[0]);
  for (int c = 0; c < nchunks; ++c) {
    __syncthreads();
    const char* V = Vs[c & 1];
    if (c + 1 < nchunks) vs.load(c + 1);
    for (int hh = 0; hh < HC; ++hh) {
      const int h = c * HC + hh;
      if (h >= p.H) break;
      const float ah = Ac[wave][h * 16 + t];
      float part = 0.f;
#pragma unroll
      for (int i = 0; i < RC_NT; ++i) {
        if (i < nWt) {
          // T^T tile: V[h] rows (A: 16 columns w x 32 d) x dO^T (B) -> lane (t = query, g): w = 16 i + 4 g + r
          const f32x4 T = rc_mfma(frag_rows(V + (hh * nW32 + (i >> 1)) * 2048, i & 1, t, g), dof, f32x4{0.f, 0.f, 0.f, 0.f});
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            dar[i][r] += ah * T[r];
            part += arow[i][r] * T[r];      // (arow = 0 exactly for columns >= W and padded ones)
          }
        }
      }
      part = rc_sum_g(part);
      Ac[wave][h * 16 + t] = part;          // dA_col[q = t][h]; all four g write the same value
    }
    if (c + 1 < nchunks) vs.store(Vs[(c + 1) & 1]);
  }
  __syncthreads();   // Krs / Kcs (when the loop ran one chunk: staged by other waves) and this wave's dA_col
  float delta = 0.f;
#pragma unroll
  for (int i = 0; i < RC_NT; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) delta += arow[i][r] * (arow[i][r] != 0.f ? dar[i][r] : 0.f);
  delta = rc_sum_g(delta);
  // dS in place: arow <- dS_row, acol <- dS_col
#pragma unroll
  for (int i = 0; i < RC_NT; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      arow[i][r] = arow[i][r] != 0.f ? arow[i][r] * (dar[i][r] - delta) : 0.f;
      const float dac = Ac[wave][(16 * i + 4 * g + r) * 16 + t];
      acol[i][r] = acol[i][r] != 0.f ? acol[i][r] * (dac - delta) : 0.f;
    }
  // dS^T to the workspace for the key side: [bh][key][Lp], queries >= L hold 0
  if (myq < Lp) {
#pragma unroll
    for (int i = 0; i < RC_NT; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int key = 16 * i + 4 * g + r;
        if (key < p.W) wsr[((size_t)bh * p.W + key) * Lp + myq] = (__bf16)arow[i][r];
        if (key < p.H) wsc[((size_t)bh * p.H + key) * Lp + myq] = (__bf16)acol[i][r];
      }
  }
  // dQr = scale dS_row Kr, dQc = scale dS_col Kc
  f32x4 ar[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}}, ac[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
  for (int t2 = 0; t2 < RC_NT / 2; ++t2) {
    bf16x8 fr, fc;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      fr[e] = (__bf16)arow[2 * t2 + (e >> 2)][e & 3];
      fc[e] = (__bf16)acol[2 * t2 + (e >> 2)][e & 3];
    }
    if (t2 < nW32) {
#pragma unroll
      for (int j = 0; j < 2; ++j) ar[j] = rc_mfma(fr, frag_cols(Krs + t2 * 2048, j, t, g), ar[j]);
    }
    if (t2 < nH32) {
#pragma unroll
      for (int j = 0; j < 2; ++j) ac[j] = rc_mfma(fc, frag_cols(Kcs + t2 * 2048, j, t, g), ac[j]);
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int qq = q0 + 4 * g + r;
    if (qq < p.L) {
      const size_t o = ((size_t)b * p.L + qq) * p.ldq + head * RC_D;
      __bf16 *dr = (__bf16*)p.dq_row + o, *dc = (__bf16*)p.dq_col + o;
      dr[t] = (__bf16)(ar[0][r] * p.scale);
      dr[16 + t] = (__bf16)(ar[1][r] * p.scale);
      dc[t] = (__bf16)(ac[0][r] * p.scale);
      dc[16 + t] = (__bf16)(ac[1][r] * p.scale);
    }
  }
}

// ------------------------------------------------------------------ backward, key side: dKr = scale dS_row^T Qr, dKc likewise
// A block owns 16 keys of one (batch, head): blockIdx.x < nWt: rows of k_row, else rows of k_col.  Its 8 waves take the 32-query
// steps round robin; the eight partial tiles are summed in wave order.
__global__ __launch_bounds__(512) void rc_bwd_k_kernel(const RcK p, const __bf16* wsr, const __bf16* wsc, int Lp) {
  __shared__ float Red[8][2][64][4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int t = lane & 15, g = lane >> 4;
  const int bh = blockIdx.y, b = bh / p.heads, head = bh % p.heads;
  const int nWt = (p.W + 15) >> 4;
  const bool col = (int)blockIdx.x >= nWt;
  const int key0 = 16 * (col ? blockIdx.x - nWt : blockIdx.x), n = col ? p.H : p.W;
  const int mykey = key0 + t < n ? key0 + t : n - 1;
  const __bf16* ds = (col ? wsc : wsr) + ((size_t)bh * n + mykey) * Lp;
  const __bf16* qb = (const __bf16*)(col ? p.q_col : p.q_row) + (size_t)b * p.L * p.ldq + head * RC_D;
  f32x4 acc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
  for (int c = wave; c * 32 < Lp; c += 8) {
    // k slot (g, e) = query 32 c + 8 g + e in both operands
    const bf16x8 a = *(const bf16x8*)(ds + c * 32 + 8 * g);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      bf16x8 qf;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int q = c * 32 + 8 * g + e;
        qf[e] = qb[(size_t)(q < p.L ? q : p.L - 1) * p.ldq + 16 * j + t];   // (dS = 0 for queries >= L)
      }
      acc[j] = rc_mfma(a, qf, acc[j]);
    }
  }
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int r = 0; r < 4; ++r) Red[wave][j][lane][r] = acc[j][r];
  __syncthreads();
  if (wave == 0) {
    __bf16* dk = (__bf16*)(col ? p.dk_col : p.dk_row) + (size_t)b * n * p.ldk + head * RC_D;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int kk = key0 + 4 * g + r;     // lane (t = d, g): key rows 4g + r
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        float s = Red[0][j][lane][r];
#pragma unroll
        for (int w = 1; w < 8; ++w) s += Red[w][j][lane][r];
        if (kk < n) dk[(size_t)kk * p.ldk + 16 * j + t] = (__bf16)(s * p.scale);
      }
    }
  }
}

// ------------------------------------------------------------------ backward, dV[h, w, :] = sum over q of A_col[q, h] A_row[q, w] dO[q, :]
// A block owns 16 columns w and 32 map rows h of one (batch, head); each of its 8 waves 4 of those rows.  Queries stream in
// steps of 32: Qr, Qc, dO tiles and the two lse rows go to LDS, waves 0 and 1 recompute A_col^T [32 h][32 q] into an LDS table,
// every wave recomputes its A_row^T tile (lane = column w, slots = queries) and multiplies P_h^T into dO on the matrix cores.
__global__ __launch_bounds__(512) void rc_bwd_v_kernel(const RcK p) {
  __shared__ __attribute__((aligned(16))) char Qr[2048], Qc[2048], Do[2048];
  __shared__ __attribute__((aligned(16))) float Lr[32], Lc[32], Tab[32][32];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int t = lane & 15, g = lane >> 4;
  const int bh = blockIdx.y, b = bh / p.heads, head = bh % p.heads;
  const int nWt = (p.W + 15) >> 4;
  const int w0 = 16 * ((int)blockIdx.x % nWt), h0 = 32 * ((int)blockIdx.x / nWt);
  const float sc2 = p.scale * RC_LOG2E;
  // B operands of the score tiles: this lane's key row (clamped; a padded or out-of-range key weighs 0)
  const int myw = w0 + t, myh = h0 + 16 * (wave & 1) + t;
  const bool deadw = myw >= p.W || (p.mask_row && p.mask_row[(size_t)b * p.W + myw]);
  const bool deadh = myh >= p.H || (p.mask_col && p.mask_col[(size_t)b * p.H + (myh < p.H ? myh : p.H - 1)]);
  const bf16x8 krf = *(const bf16x8*)((const __bf16*)p.k_row + ((size_t)b * p.W + (myw < p.W ? myw : p.W - 1)) * p.ldk + head * RC_D + g * 8);
  const bf16x8 kcf = *(const bf16x8*)((const __bf16*)p.k_col + ((size_t)b * p.H + (myh < p.H ? myh : p.H - 1)) * p.ldk + head * RC_D + g * 8);
  f32x4 acc[4][2];
#pragma unroll
  for (int i = 0; i < 4; ++i) acc[i][0] = acc[i][1] = f32x4{0.f, 0.f, 0.f, 0.f};
  // staging: threads 0..383 one 16-byte piece of Qr / Qc / dO, threads 384..447 one lse word
  const int which = tid >> 7, row = (tid & 127) >> 2, piece = tid & 3;
  u32x4 reg = {0u, 0u, 0u, 0u};
  float lreg = 0.f;
  auto load = [&](int c) {
    const int q = c * 32 + row;
    const int qc = q < p.L ? q : p.L - 1;
    if (which < 3) {
      const __bf16* src = which == 0 ? (const __bf16*)p.q_row : which == 1 ? (const __bf16*)p.q_col : (const __bf16*)p.dout;
      reg = *(const u32x4*)(src + ((size_t)b * p.L + qc) * (which == 2 ? p.ldo : p.ldq) + head * RC_D + piece * 8);
    } else if (tid < 448) {
      const int ql = c * 32 + (tid & 31);
      const float* ls = (tid & 32) ? p.lse_col : p.lse_row;
      lreg = ql < p.L ? ls[(size_t)bh * p.L + ql] : INFINITY;
    }
  };
  auto store = [&]() {
    if (which < 3) *(u32x4*)((which == 0 ? Qr : which == 1 ? Qc : Do) + tile_off(row, piece)) = reg;
    else if (tid < 448) ((tid & 32) ? Lc : Lr)[tid & 31] = lreg == -INFINITY ? INFINITY : lreg;   // (a dead query weighs nothing)
  };
  const int nsteps = (p.L + 31) >> 5;
  load(0);
  for (int c = 0; c < nsteps; ++c) {
    __syncthreads();          // the tiles and the table of step c - 1 are no longer read
    store();
    if (c + 1 < nsteps) load(c + 1);
    __syncthreads();          // tiles visible
    if (wave < 2) {
      // A_col^T: Qc tile rows (A: 16 queries) x Kc^T (B: lane (t = h, g)) -> lane (t = h, g): queries 16 a + 4 g + r
#pragma unroll
      for (int a = 0; a < 2; ++a) {
        const f32x4 s = rc_mfma(frag_rows(Qc, a, t, g), kcf, f32x4{0.f, 0.f, 0.f, 0.f});
        const f32x4 lr4 = *(const f32x4*)(&Lr[16 * a + 4 * g]), lc4 = *(const f32x4*)(&Lc[16 * a + 4 * g]);
        f32x4 o;
#pragma unroll
        for (int r = 0; r < 4; ++r) o[r] = (deadh || lr4[r] == INFINITY) ? 0.f : __builtin_amdgcn_exp2f(s[r] * sc2 - lc4[r]);
        *(f32x4*)(&Tab[16 * (wave & 1) + t][16 * a + 4 * g]) = o;
      }
    }
    // A_row^T of this block's 16 columns: lane (t = w, g): slot e = query 16 (e >> 2) + 4 g + (e & 3)
    float ar[8];
#pragma unroll
    for (int a = 0; a < 2; ++a) {
      const f32x4 s = rc_mfma(frag_rows(Qr, a, t, g), krf, f32x4{0.f, 0.f, 0.f, 0.f});
      const f32x4 lr4 = *(const f32x4*)(&Lr[16 * a + 4 * g]), lc4 = *(const f32x4*)(&Lc[16 * a + 4 * g]);
#pragma unroll
      for (int r = 0; r < 4; ++r) ar[4 * a + r] = (deadw || lc4[r] == INFINITY) ? 0.f : __builtin_amdgcn_exp2f(s[r] * sc2 - lr4[r]);
    }
    const bf16x8 d0 = frag_cols(Do, 0, t, g), d1 = frag_cols(Do, 1, t, g);
    __syncthreads();          // table visible
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int hl = 4 * wave + i;
      const f32x4 c0 = *(const f32x4*)(&Tab[hl][4 * g]), c1 = *(const f32x4*)(&Tab[hl][16 + 4 * g]);
      bf16x8 pf;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        pf[e] = (__bf16)(c0[e] * ar[e]);
        pf[4 + e] = (__bf16)(c1[e] * ar[4 + e]);
      }
      acc[i][0] = rc_mfma(pf, d0, acc[i][0]);
      acc[i][1] = rc_mfma(pf, d1, acc[i][1]);
    }
  }
  // lane (t = d, g): columns w0 + 4g + r
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int h = h0 + 4 * wave + i;
    if (h >= p.H) continue;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int w = w0 + 4 * g + r;
      if (w < p.W) {
        __bf16* dv = (__bf16*)p.dv + (((size_t)b * p.H + h) * p.W + w) * p.ldv + head * RC_D;
        dv[t] = (__bf16)acc[i][0][r];
        dv[16 + t] = (__bf16)acc[i][1][r];
      }
    }
  }
}

// ------------------------------------------------------------------ entries
static bool rc_al16(const void* q) { return ((uintptr_t)q & 15) == 0; }

static int rc_check_geometry(const mi_rcda_desc* d, const char* who) {
  MI_REQUIRE(d, "%s: null descriptor", who);
  MI_REQUIRE(d->B > 0 && d->heads > 0 && d->L > 0 && d->H > 0 && d->W > 0, "%s: B %d / heads %d / L %d / H %d / W %d must be positive",
             who, d->B, d->heads, d->L, d->H, d->W);
  MI_REQUIRE(d->E == d->heads * RC_D, "%s: E %d must be heads * %d (heads %d)", who, d->E, RC_D, d->heads);
  MI_REQUIRE(d->H <= RC_MAX && d->W <= RC_MAX, "%s: map %d x %d above the served size %d x %d", who, d->H, d->W, RC_MAX, RC_MAX);
  MI_REQUIRE((long long)d->B * d->heads < 65536, "%s: B * heads too large", who);
  MI_REQUIRE((long long)d->B * d->L * (long long)(d->ldq > d->ldo ? d->ldq : d->ldo) < (1LL << 40), "%s: L too large", who);
  return MI_OK;
}

static int rc_check_common(const mi_rcda_desc* d, const char* who) {
  int rc = rc_check_geometry(d, who);
  if (rc) return rc;
  MI_REQUIRE(d->ldq >= d->E && d->ldk >= d->E && d->ldv >= d->E && d->ldo >= d->E && d->ldq % 8 == 0 && d->ldk % 8 == 0 &&
                 d->ldv % 8 == 0 && d->ldo % 8 == 0,
             "%s: row strides ldq %d / ldk %d / ldv %d / ldo %d (>= E, multiples of 8)", who, d->ldq, d->ldk, d->ldv, d->ldo);
  MI_REQUIRE(d->q_row && d->q_col && d->k_row && d->k_col && d->v && d->lse_row && d->lse_col, "%s: null operand", who);
  MI_REQUIRE(rc_al16(d->q_row) && rc_al16(d->q_col) && rc_al16(d->k_row) && rc_al16(d->k_col) && rc_al16(d->v) &&
                 ((uintptr_t)d->lse_row & 3) == 0 && ((uintptr_t)d->lse_col & 3) == 0,
             "%s: operands must be 16-byte aligned", who);
  return MI_OK;
}

extern "C" int mi_rcda_desc_size(void) { return (int)sizeof(mi_rcda_desc); }

extern "C" int mi_rcda_key_mean(const void* key_row, const void* key_col, void* mean_row, void* mean_col, int B, int H, int W, int E,
                                mi_stream_t st) {
  MI_REQUIRE(B > 0 && H > 0 && W > 0 && E > 0, "rcda_key_mean: B %d / H %d / W %d / E %d must be positive", B, H, W, E);
  MI_REQUIRE(E % 8 == 0, "rcda_key_mean: E %d must be a multiple of 8", E);
  MI_REQUIRE(key_row || key_col, "rcda_key_mean: null (neither key map given)");
  MI_REQUIRE((!key_row || mean_row) && (!key_col || mean_col), "rcda_key_mean: null output");
  MI_REQUIRE(rc_al16(key_row) && rc_al16(key_col) && rc_al16(mean_row) && rc_al16(mean_col), "rcda_key_mean: operands must be 16-byte aligned");
  const long long n = (long long)B * (E / 8) * ((key_row ? W : 0) + (key_col ? H : 0));
  MI_REQUIRE(n < (1LL << 31) * 256, "rcda_key_mean: too large");
  hipLaunchKernelGGL(rc_key_mean_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)st, (const __bf16*)key_row,
                     (const __bf16*)key_col, (__bf16*)mean_row, (__bf16*)mean_col, B, H, W, E);
  MI_CHECK_LAUNCH("rcda_key_mean");
  return MI_OK;
}

extern "C" int mi_rcda_fwd(const mi_rcda_desc* d, mi_stream_t st) {
  int rc = rc_check_common(d, "rcda_fwd");
  if (rc) return rc;
  MI_REQUIRE(d->o, "rcda_fwd: null output");
  MI_REQUIRE(rc_al16(d->o), "rcda_fwd: output must be 16-byte aligned");
  hipLaunchKernelGGL(rc_fwd_kernel, dim3(mi_cdiv(d->L, 64), d->B * d->heads), dim3(256), 0, (hipStream_t)st, *d);
  MI_CHECK_LAUNCH("rcda_fwd");
  return MI_OK;
}

static int rc_lp(int L) { return (L + 31) / 32 * 32; }

extern "C" int64_t mi_rcda_bwd_ws_bytes(const mi_rcda_desc* d) {
  int rc = rc_check_geometry(d, "rcda_bwd_ws_bytes");
  if (rc) return rc;
  return (int64_t)d->B * d->heads * (d->W + d->H) * rc_lp(d->L) * 2;
}

extern "C" int mi_rcda_bwd(const mi_rcda_desc* d, mi_stream_t st) {
  int rc = rc_check_common(d, "rcda_bwd");
  if (rc) return rc;
  MI_REQUIRE(d->dout && d->dq_row && d->dq_col && d->dk_row && d->dk_col && d->dv && d->ws, "rcda_bwd: null operand");
  MI_REQUIRE(rc_al16(d->dout) && rc_al16(d->dq_row) && rc_al16(d->dq_col) && rc_al16(d->dk_row) && rc_al16(d->dk_col) && rc_al16(d->dv) &&
                 rc_al16(d->ws),
             "rcda_bwd: operands must be 16-byte aligned");
  const int64_t need = mi_rcda_bwd_ws_bytes(d);
  MI_REQUIRE(d->ws_bytes >= need, "rcda_bwd: workspace %lld bytes < %lld", (long long)d->ws_bytes, (long long)need);
  const int Lp = rc_lp(d->L), BH = d->B * d->heads;
  __bf16* wsr = (__bf16*)d->ws;
  __bf16* wsc = wsr + (size_t)BH * d->W * Lp;
  hipStream_t s = (hipStream_t)st;
  hipLaunchKernelGGL(rc_bwd_q_kernel, dim3(mi_cdiv(d->L, 64), BH), dim3(256), 0, s, *d, wsr, wsc, Lp);
  MI_CHECK_LAUNCH("rcda_bwd_q");
  hipLaunchKernelGGL(rc_bwd_k_kernel, dim3(mi_cdiv(d->W, 16) + mi_cdiv(d->H, 16), BH), dim3(512), 0, s, *d, (const __bf16*)wsr,
                     (const __bf16*)wsc, Lp);
  MI_CHECK_LAUNCH("rcda_bwd_k");
  hipLaunchKernelGGL(rc_bwd_v_kernel, dim3(mi_cdiv(d->W, 16) * mi_cdiv(d->H, 32), BH), dim3(512), 0, s, *d);
  MI_CHECK_LAUNCH("rcda_bwd_v");
  return MI_OK;
}
