/*
 * mi355_det.h — C-ABI of libmi355det.so: the MI355X (gfx950) hot path of
 * yolov7_d2's YOLOX data-parallel training step.
 *
 * Every entry point is `extern "C"`, takes plain device pointers + sizes and a
 * hipStream_t (passed as void*), never allocates, frees or synchronises, and
 * returns 0 on success or a negative MI_E* code for an argument error detected
 * BEFORE any launch.  The caller (PyTorch caching allocator, or any other
 * runtime) owns every buffer including workspaces.
 *
 * Each function names the reference interface it replaces (file:line relative
 * to lucasjinreal/yolov7_d2).  The reference has no native code of its own on
 * this path: these replace the ATen/cuDNN/torchvision calls the reference
 * reaches through torch.
 *
 * Layout conventions
 *   activations : bf16, NHWC ("channels_last"); a tensor is (ptr, ld) where ld is
 *                 the element stride between consecutive pixels, so a channel
 *                 slice of a concat buffer is just (ptr + c0, ld_of_buffer).
 *   conv weights: fp32 OIHW masters (the nn.Parameter layout of the reference);
 *                 mi_pack_conv_weight() produces the bf16 k8-major images the
 *                 conv kernels read: [tap][K/8][CoutPad][8].
 *   head preds  : fp32 [B][A][5+ncls] exactly as yolox_head.py:238-241 flattens.
 */
#ifndef MI355_DET_H
#define MI355_DET_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MI_OK 0
#define MI_EINVAL (-1)   /* bad argument (shape / alignment / unsupported config) */
#define MI_ELAUNCH (-2)  /* hipGetLastError() != success after a launch          */
#define MI_ENODEV (-3)   /* no HIP device                                          */

typedef void* mi_stream_t; /* hipStream_t */

/* ---- library ---------------------------------------------------------- */
int mi_version(void);
/* number of visible HIP devices (0 => every compute entry returns MI_ENODEV) */
int mi_device_count(void);
const char* mi_last_error(void);

/* ---- convolution (implicit GEMM on MFMA, im2col-free, LDS halo tile) ---
 * replaces nn.Conv2d fwd/dgrad inside BaseConv (layers/wrappers.py:60-83) and
 * the biased 1x1 prediction convs (head/yolox_head.py:103-129).
 * One descriptor covers: 1x1, 3x3 s1, 3x3 s2 forward; their data gradients
 * (s2 dgrad = 4 parity-class launches with out_stride 2) via the tap table. */
#define MI_CONV_ACCUM 1    /* y += result (gradient fan-in)                  */
#define MI_CONV_OUT_F32 2  /* y is fp32 (prediction maps), else bf16         */
#define MI_CONV_RELU 8     /* y = max(result + bias, 0): the ReLU behind a Conv2d + FrozenBatchNorm2d of detectron2's ResNet
                              (forward, bf16 output, no MI_CONV_ACCUM / statistics); tile kernel only              */
#define MI_CONV_RELUMASK 16 /* y = result where aux > 0, else 0; aux = bn_y (bf16 NHWC, the shape of y, pixel stride bn_ldy): the
                              OUTPUT of the ReLU this data gradient flows back through - ReLU backward in the epilogue     */
#define MI_CONV_ADDRELU 32  /* y = max(bf16(result + bias) + aux, 0) rounded as mi_ew_bf16 op 7: conv3 + shortcut + ReLU of a
                              bottleneck block (detectron2 BottleneckBlock.forward) in the epilogue; aux = bn_y           */
#define MI_CONV_BNBWD 4    /* data-gradient launch that also reduces the BatchNorm backward sums of the layer that
                              PRODUCED its output tensor: stats_acc += (sum dz, sum dz*xhat) per channel with
                              dz = y_out * act'(bn_y*scale+shift), xhat = (bn_y-mean)*invstd - replaces the
                              mi_bn_act_bwd_reduce pass over (da, y) of that layer (bf16 staged outputs only) */
#define MI_MAX_TAPS 16 /* 3x3 = 9; 16 = the 7x7 stride-2 ResNet stem as a 4x4 conv over the 2x2 space-to-depth image */
#define MI_BN_SLOTS 16     /* max accumulator slots per channel (slot = pixel tile % nslots); callers pick
                              nslots per layer: more slots = less same-address atomic traffic in the conv
                              epilogue, fewer = a shorter statistics prologue in the BN kernels */

typedef struct mi_conv_desc {
  const void* x;   /* bf16 NHWC input view, >= K8*8 channels readable        */
  const void* w;   /* packed bf16 [n_wslabs][K8][CoutPad][8]                  */
  void* y;         /* output view                                             */
  const float* bias;    /* [Cout] or NULL                                     */
  double* stats_acc;    /* [stats_slots][CoutPad][2] fp64 (sum, sumsq) accumulators, atomically added
                           (caller zeroes them once per step), or NULL             */
  int32_t ldx, ldy;
  int32_t y_nstride;        /* elements between images of y; 0 => outH*outW*ldy */
  int32_t N, H, W;          /* input dims                                     */
  int32_t outH, outW;       /* real output tensor dims                        */
  int32_t gridH, gridW;     /* output sub-grid iterated (==outH,outW if out_stride==1) */
  int32_t in_stride;        /* input pixel  = grid*in_stride  + tap offset    */
  int32_t out_stride, out_oy, out_ox; /* output pixel = grid*out_stride + off */
  int32_t K8;               /* padded input channels / 8                      */
  int32_t Cout, CoutPad;
  int32_t ntaps;
  int32_t tap_dy[MI_MAX_TAPS], tap_dx[MI_MAX_TAPS], tap_w[MI_MAX_TAPS];
  int32_t flags;
  int32_t TH, TW;           /* pixel tile; 0 => chosen by the launcher        */
  int32_t KC, BN;           /* k-chunk / cout tile; 0 => chosen by launcher   */
  int32_t stats_slots;      /* 1..MI_BN_SLOTS accumulator slots (0 => MI_BN_SLOTS) */
  int32_t TPS;              /* taps multiplied per main-loop step (divides ntaps); 0 => chosen by launcher */
  /* MI_CONV_BNBWD only: raw conv output of the producing layer (bf16 NHWC, same N x outH x outW x Cout as y),
   * its BatchNorm scale / shift / mean / invstd [Cout] and activation (1 = SiLU, 0 = none) */
  const void* bn_y;
  const float* bn_scale;
  const float* bn_shift;
  const float* bn_mean;
  const float* bn_invstd;
  int32_t bn_ldy, bn_act;
  /* BatchNorm(train) + activation of the INPUT, applied by this launch ("BN in the consumer", csrc/conv_bn.h): x is the
   * RAW output of the producing convolution and xf a DEVICE record (mi_bnx) with that layer's accumulators, parameters and
   * the activated tensor `a`; the launch derives scale / shift itself, transforms the tiles it fetched in LDS and - when
   * xf_write - stores a for the tensor's later readers, records scale / shift / mean / invstd and updates the running
   * statistics: mi_bn_act_fwd(x -> a) followed by this convolution on a, bit for bit, in one launch.  Forward
   * convolutions with stats_acc on the streaming 1x1 / weight-stationary 3x3 kernels only (mi_conv2d returns MI_EINVAL
   * otherwise); jobs of one launch that read the same x share the record and exactly one of them sets xf_write. */
  const void* xf;
  int32_t xf_write, xf_C;   /* xf_C: the record's channel count (== K8 * 8) */
} mi_conv_desc;

/* device record behind mi_conv_desc.xf (host-built, uploaded by the caller; all pointers are device pointers) */
typedef struct mi_bnx {
  const void* res_unused; void* a;
  const float* gamma; const float* beta; float* rmean; float* rvar; int64_t* nbt;
  float* scale; float* shift; float* mean; float* invstd;
  int32_t ldres_unused, lda, act, pad0_;
  double inv_count, unbias;
  float eps, momentum;
  const double* acc;        /* the producer's fp64 (sum, sumsq) accumulators [nslots][sld / 2][2] */
  int32_t sld, nslots, C, pad1_;
} mi_bnx;

int mi_conv2d(const mi_conv_desc* d, mi_stream_t s);
/* fills TH/TW/KC/BN/TPS if zero; returns number of pixel tiles or <0 */
int mi_conv2d_plan(mi_conv_desc* d);
/* the kernel family mi_conv2d runs for this descriptor: 0 tile kernel (conv_igemm), 1 mi_conv1x1_stream, 2 mi_conv3x3_ws;
 * -1 when the descriptor carries an input BatchNorm (xf) and neither 1 nor 2 applies (mi_conv2d would refuse it) */
int mi_conv2d_route(const mi_conv_desc* d);

/* several independent convolutions in ONE launch (the FPN levels of the head: the 40x40 / 20x20 launches are
 * latency-bound alone).  All jobs run the template configuration chosen for the job with the most output pixels, so
 * their K must be a multiple of its k-chunk, CoutPad of its cout tile, and they must agree on ntaps-divisibility and
 * on MI_CONV_ACCUM / MI_CONV_BNBWD.  _plan() writes the device job table into table_host (caller uploads it; NULL / 0
 * to query meta->table_bytes); _run() launches it. */
#define MI_CONV_MAX_GROUP 8
typedef struct mi_conv_group {
  int32_t njobs, nblocks, lds_bytes;
  int32_t KC, BN, TPIX, TPS, EPI;
  int64_t starts_off, table_bytes;
  int64_t priv[288];        /* KC == -1: the jobs are 1x1 convolutions of one input and run as ONE streaming launch
                               (mi_conv1x1_stream); KC == -2: 3x3 K -> K convolutions as ONE weight-stationary launch
                               (mi_conv3x3_ws); the launch record lives here, no device table is read */
} mi_conv_group;
int mi_conv2d_group_plan(const mi_conv_desc* descs, int n, void* table_host, int64_t table_cap, mi_conv_group* meta);
int mi_conv2d_group_run(const mi_conv_group* meta, const void* table_dev, mi_stream_t s);

/* streaming 1x1 convolution (csrc/conv1x1_stream.h): n >= 1 bf16 1x1 stride-1 convolutions that read the SAME input
 * view (x, ldx, N, H, W, K8 equal; K in {32, 64, 128, 256, 512}; Cout == CoutPad, a multiple of 32; all with stats_acc,
 * all with MI_CONV_ACCUM, or all plain) as one persistent launch: weights stay in registers, the input is read once,
 * BatchNorm statistics leave as one set of atomics per block.  Round 6: descriptors with an fp32 bias, MI_CONV_RELU,
 * MI_CONV_ADDRELU or MI_CONV_RELUMASK (the same flags for all n; bn_y / bn_ldy = the second tensor) are served too, and -
 * for the launches without statistics - pixel counts N * H * W that are no multiple of the pixel tile (>= 8192 pixels) and
 * ONE convolution with more than 512 output channels (a multiple of 512: 512 at a time).  Replaces the 1x1 nn.Conv2d forward / data
 * gradient of CSPLayer / Bottleneck / SPP / head stems (layers/wrappers.py:60-83,150-197).  mi_conv2d and
 * mi_conv2d_group_plan take this path by themselves for eligible descriptors (MI_CONV_STREAM=0 disables that);
 * this entry returns MI_EINVAL instead of falling back. */
int mi_conv1x1_stream(const mi_conv_desc* descs, int n, mi_stream_t s);

/* weight-stationary 3x3 convolution (csrc/conv3x3_ws.h): 1..8 bf16 3x3 stride-1 convolutions with Cin == Cout == K in
 * {32, 64, 128} (the same K for all; their own tensors and shapes), no bias, all plain / all with stats_acc / all
 * MI_CONV_ACCUM, as ONE launch of persistent blocks: each wave keeps its 32 output channels x 9 taps x K of weights in
 * registers, only the input halo tiles move (LDS-DMA, double-buffered).  Forward and data gradient (any tap order) of
 * Bottleneck conv2 and of the YOLOXHead cls / reg towers (layers/wrappers.py:105-123, head/yolox_head.py:73-102).
 * mi_conv2d and mi_conv2d_group_plan take this path by themselves (MI_CONV_WS=0 disables that); this entry returns
 * MI_EINVAL instead of falling back. */
int mi_conv3x3_ws(const mi_conv_desc* descs, int n, mi_stream_t s);

/* weight gradient: g[co][ci][tap] (fp32 OIHW, the nn.Parameter gradient layout; overwritten, or += if
 * `accumulate`) = sum_pixels dy[p][co] * x[p*stride + tap][ci].  replaces conv wgrad of the same modules.
 * Split-K over pixel tiles with a caller-owned fp32 workspace (no atomics: the split partials are summed
 * in a fixed order, so the result is bit-reproducible); mi_conv2d_wgrad_plan() returns the bytes needed. */
typedef struct mi_wgrad_desc {
  const void* x;  /* bf16 NHWC input view  (CinPad channels readable)        */
  const void* dy; /* bf16 NHWC out-grad view (CoutPad channels readable)     */
  float* gw;      /* fp32 [Cout][Cin][ntaps]                                  */
  void* ws;       /* split-K workspace, 16-byte aligned                       */
  int64_t ws_bytes;
  int32_t ldx, ldy;
  int32_t N, H, W, outH, outW;
  int32_t stride;
  int32_t Cin, Cout;        /* real channel counts written to gw              */
  int32_t CinPad, CoutPad;  /* readable (zero-padded) channels, CinPad%16==0, CoutPad%32==0 */
  int32_t ntaps;            /* 1, 9 or 16 (MI_MAX_TAPS: the ResNet stem's 4x4 table); any (tap_dy, tap_dx) per tap */
  int32_t tap_dy[MI_MAX_TAPS], tap_dx[MI_MAX_TAPS];
  int32_t accumulate;
  int32_t TH, TW, splitk, cfg_tp, cfg_ns; /* 0 => chosen by launcher (pixel tile, split-K, tile pixels, LDS stages) */
  const float* row_scale; /* NULL, or fp32 [Cout]: gw[co] (+)= row_scale[co] * dW[co] - the gradient of a weight whose
                           * image carried a folded per-Cout factor (mi_pack_conv_weight_scaled), applied to the fp32
                           * sum in the split-K reduction */
  float* gbias;           /* NULL, or fp32 [Cout]: the BIAS gradient = column sums of dy over all pixels, written by the
                           * same two launches (the blocks of input-channel tile 0 add up the dy rows they stream, the
                           * split-K reduction adds the splits in a fixed order) instead of a separate column-sum launch;
                           * mi_conv2d_wgrad only (single layers: nn.Linear / biased nn.Conv2d of DETR and SparseInst);
                           * mi_conv2d_wgrad_plan then returns the workspace INCLUDING nsplit * CoutPad floats for it */
} mi_wgrad_desc;
int mi_conv2d_wgrad(const mi_wgrad_desc* d, mi_stream_t s);
/* workspace bytes mi_conv2d_wgrad needs for this descriptor (pointers may be NULL), or <0 */
int64_t mi_conv2d_wgrad_plan(const mi_wgrad_desc* d);

/* grouped form: all layers of a step in one grid per tile configuration + one reduce grid (weight gradients are
 * not consumed before the optimizer step, so they can all run at the end of backward; each layer keeps its own
 * out-gradient buffer).  _plan() lays out per-layer workspaces from ws_base, writes the device job table into
 * table_host (caller uploads it; pass NULL/0 to query sizes) and fills *meta; _run() launches it. */
#define MI_WGRAD_MAX_GROUPS 32
typedef struct mi_wgrad_group {
  int32_t ngroups, nred, red_blocks, pad_;
  struct {
    int32_t cfg[6];
    int32_t njobs, nblocks, lds_bytes, pad_;
    int64_t job_off, starts_off;
  } g[MI_WGRAD_MAX_GROUPS];
  int64_t red_off, red_starts_off, table_bytes, ws_bytes;
} mi_wgrad_group;
int mi_conv2d_wgrad_group_plan(const mi_wgrad_desc* descs, int n, void* ws_base, void* table_host,
                               int64_t table_cap, mi_wgrad_group* meta);
int mi_conv2d_wgrad_group_run(const mi_wgrad_group* meta, const void* table_dev, mi_stream_t s);
/* (round 6) jobs of a group may carry gbias: the bias gradient (column sums of dy) then leaves with the group's launches -
 * partial rows behind the job's split slabs, summed in a fixed order by extra blocks of the reduce grid.  Used by the
 * per-layer grouped weight gradients of the transformer / ResNet blocks (yolov7_d2_amd/ops.py WgradBatch). */
/* asynchronous host -> device copy of a job table on stream s (hipMemcpyAsync; `src_pinned` must be page-locked and must
 * stay unchanged while a captured graph that recorded this copy can replay) */
int mi_upload_async(void* dst_dev, const void* src_pinned, int64_t nbytes, mi_stream_t s);

/* OIHW fp32 master -> packed bf16 images.  wf: forward [KH*KW][CinPad/8][CoutPad][8];
 * wd: dgrad  [KH*KW][CoutPadK/8][CinPadN][8] (roles swapped).  Either may be NULL. */
int mi_pack_conv_weight(const float* w_oihw, int Cout, int Cin, int KH, int KW,
                        void* wf, int CinPad, int CoutPad,
                        void* wd, int CoutPadK, int CinPadN, mi_stream_t s);

/* the same with a per-output-channel fp32 factor folded in before the bf16 rounding: detectron2's Conv2d(norm =
 * FrozenBatchNorm2d) as the reference's DETR / SparseInst backbones build it (W * scale[co]; un-vendored d2
 * layers/batch_norm.py FrozenBatchNorm2d + layers/wrappers.py Conv2d) without a folded fp32 copy of the weight */
int mi_pack_conv_weight_scaled(const float* w_oihw, const float* cout_scale, int Cout, int Cin, int KH, int KW,
                               void* wf, int CinPad, int CoutPad,
                               void* wd, int CoutPadK, int CinPadN, mi_stream_t s);
/* out[r][:] = g[r][:] * scale[r], fp32 [rows][rowlen]: the weight gradient of such a layer (dW = scale[co] * dW') */
int mi_scale_rows_f32(const float* g, const float* scale, float* out, int rows, int rowlen, mi_stream_t s);

/* all layers of a step in ONE launch: jobs_dev is a device array of njobs records (same meaning as the
 * arguments of mi_pack_conv_weight) */
typedef struct mi_pack_job {
  const float* w;
  void* wf;
  void* wd;
  int32_t Cout, Cin, KK, CinPad, CoutPad, CoutPadK, CinPadN;
  int32_t blk0; /* first block of this job in the flat launch: filled by mi_pack_jobs_layout */
  const float* scale; /* NULL, or fp32 [Cout] folded into both images as mi_pack_conv_weight_scaled does (W * scale[co]) */
} mi_pack_job;
/* validates the (host) job table, fills blk0 and returns the number of blocks of the flat launch (<0 on error) */
int mi_pack_jobs_layout(mi_pack_job* jobs_host, int njobs);
/* kk_max: the largest tap count (KK) of the table: sizes the kernel's LDS tile */
int mi_pack_conv_weights_batch(const mi_pack_job* jobs_dev, int njobs, int total_blocks, int kk_max, mi_stream_t s);

/* ---- grouped 3x3 convolution (csrc/conv_grouped.hip) ---------------------------------
 * nn.Conv2d(C, C, 3, stride, padding = 1, groups = G) with square groups of Cg = C / G in {8, 16, 24, 32} channels: the 3x3
 * of a RegNet X / Y block (backbone/regnet.py; group widths 8 / 16 / 24) and of ResNeXt (32).  Served: 3x3, padding 1,
 * dilation 1, stride 1 or 2, G >= 1; anything else returns MI_EINVAL naming the quantity, before any launch and before any
 * pointer is looked at.
 * x and y are bf16 NHWC views with pixel strides ldx, ldy >= C (multiples of 8; base pointers 16-byte aligned): group g owns
 * channels [g * Cg, (g + 1) * Cg), channels >= C of a pixel are never read and never written.  Ho = (H - 1) / stride + 1.
 *   forward          y[n][oy][ox][g*Cg+co] = bf16(bias[g*Cg+co] + sum over (r, s, ci) of
 *                        x[n][oy*stride-1+r][ox*stride-1+s][g*Cg+ci] * w[g*Cg+co][ci][r][s]),  x = 0 outside the map;
 *                    fp32 accumulation on the matrix cores, fp32 bias (may be NULL), one rounding at the store.
 *   data gradient    the exact adjoint: reads y (= dy) and the data-gradient image, writes EVERY pixel of x (= dx) itself
 *                    (no zero fill by the caller, also where a stride-2 layer's taps do not reach).
 *   weight gradient  gw[g*Cg+co][ci][r][s] fp32 (the parameter's layout [C][Cg][3][3]), overwritten; gbias (may be NULL):
 *                    fp32 [C] column sums of dy from the same launches.  Split over pixel tiles into a caller-owned
 *                    workspace, the partials summed in a fixed order by a second launch: no atomics, bit-reproducible.
 * One launch per pass over all groups (the weight gradient: one + its reduction).
 * mi_gconv_pack_weight: fp32 [C][Cg][3][3] -> the forward and the data-gradient bf16 image (either may be NULL), each
 * mi_gconv_weight_image_bytes(C, Cg) bytes, rounded to nearest even as mi_pack_conv_weight does.  An image is the kernels'
 * MFMA fragment order [G][MT][NK][64 lanes][8] with MT = ceil(Cg / 16), NK = ceil(9 * Cg / 32): entry (g, mt, m, lane, j) has
 * row = mt*16 + (lane & 15), octet q = 4*m + (lane >> 4), tap t = q / (Cg/8), k = (q % (Cg/8))*8 + j and holds
 * w[g*Cg+row][k][t/3][t%3] (forward) or w[g*Cg+k][row][2-t/3][2-t%3] (data gradient); zero where row >= Cg or q >= 9*Cg/8. */
typedef struct mi_gconv_desc {
  void* x;            /* the layer's input side: x (forward, weight gradient: read) or dx (data gradient: written)  */
  void* y;            /* the layer's output side: y (forward: written) or dy (both gradients: read)                 */
  const void* w;      /* packed image: the forward image (forward), the data-gradient image (data gradient)          */
  const float* bias;  /* forward: fp32 [C] or NULL                                                                    */
  float* gw;          /* weight gradient: fp32 [C][Cg][3][3]                                                          */
  float* gbias;       /* weight gradient: fp32 [C] or NULL                                                            */
  void* ws;           /* weight gradient: workspace, 16-byte aligned                                                  */
  int64_t ws_bytes;   /* >= mi_gconv_wgrad_plan()                                                                     */
  int32_t ldx, ldy;
  int32_t N, H, W;    /* the layer's input map; the output map is Ho x Wo                                             */
  int32_t Cin, Cout, G;
  int32_t kh, kw, stride, padding, dilation;
  int32_t rsv_;
} mi_gconv_desc;
int mi_gconv_desc_size(void);   /* sizeof(mi_gconv_desc) as compiled (binding self-check) */
int64_t mi_gconv_weight_image_bytes(int C, int Cg);
int mi_gconv_pack_weight(const float* w, int C, int Cg, void* wf, void* wd, mi_stream_t s);
int mi_gconv_fwd(const mi_gconv_desc* d, mi_stream_t s);
int mi_gconv_dgrad(const mi_gconv_desc* d, mi_stream_t s);
/* workspace bytes of mi_gconv_wgrad for this descriptor (pointers may be NULL), or < 0; *nsplit (may be NULL) receives the
 * number of split partials: the bytes are nsplit * (C * Cg * 9 + C) * 4 */
int64_t mi_gconv_wgrad_plan(const mi_gconv_desc* d, int32_t* nsplit);
int mi_gconv_wgrad(const mi_gconv_desc* d, mi_stream_t s);

/* ---- row-column decoupled attention (csrc/rcda.hip) ----------------------------------
 * The attention core of Anchor DETR's MultiheadRCDA (backbone/layers/row_column_decoupled_attention.py), head_dim 32:
 *   A_row[b,n,q,:] = softmax over w of scale * q_row[b,q,n,:] . k_row[b,w,n,:]   (-inf where mask_row[b][w])
 *   A_col[b,n,q,:] = softmax over h of scale * q_col[b,q,n,:] . k_col[b,h,n,:]   (-inf where mask_col[b][h])
 *   o[b,q,n,:]     = sum over h, w of A_col[b,n,q,h] * A_row[b,n,q,w] * v[b,h,w,n,:]
 * bf16 operands, fp32 accumulation and softmax statistics; the weight A_col * A_row is rounded to bf16 once.  All tensors are
 * batch first: q_row, q_col, dq_* [B][L] rows (row stride ldq), k_row, dk_row [B][W] rows and k_col, dk_col [B][H] rows (ldk:
 * the projected means over H / W of the key maps), v, dv [B][H][W] rows (ldv), o, dout [B][L] rows (ldo); a row holds
 * E = heads * 32 channels, head n in [32 n, 32 n + 32).  Strides are >= E and multiples of 8, base pointers 16-byte aligned.
 * mask_row uint8 [B][W], mask_col uint8 [B][H] (1 = padded; either may be NULL).  lse_row, lse_col: fp32 [B][heads][L],
 * written by the forward and read by the backward, in base-2 units (log2 of the sum of exp2(score * scale * log2 e)); -inf for
 * a query whose row or column keys are all padded: its output is 0 and it contributes no gradient.
 * Served: H, W <= 96, any L >= 1.  Anything else returns MI_EINVAL naming the quantity, before any launch.
 * The backward writes every element of dq_row, dq_col, dk_row, dk_col, dv; its sums over queries run in a fixed order (no
 * atomics: bit-reproducible).  ws: mi_rcda_bwd_ws_bytes() bytes of scratch (the two softmax gradients, bf16, for the key-side
 * reduction).  No entry allocates, reads back or synchronises: every call can be captured into a graph.
 * mi_rcda_key_mean: mean_row[b][w][:] = mean over h of key_row[b][h][w][:], mean_col[b][h][:] = mean over w of
 * key_col[b][h][w][:] (bf16 [B][H][W][E] contiguous in, fp32 sums in index order, one rounding), both in one launch; either
 * pair may be NULL. */
typedef struct mi_rcda_desc {
  const void* q_row;
  const void* q_col;
  const void* k_row;
  const void* k_col;
  const void* v;
  const uint8_t* mask_row;
  const uint8_t* mask_col;
  void* o;              /* forward: written                                           */
  float* lse_row;       /* forward: written; backward: read                           */
  float* lse_col;
  const void* dout;     /* backward only from here                                    */
  void* dq_row;
  void* dq_col;
  void* dk_row;
  void* dk_col;
  void* dv;
  void* ws;
  int64_t ws_bytes;     /* >= mi_rcda_bwd_ws_bytes()                                  */
  int32_t B, heads, L, H, W, E;
  int32_t ldq, ldk, ldv, ldo;
  float scale;          /* head_dim^-0.5 in the module                                */
  int32_t rsv_;
} mi_rcda_desc;
int mi_rcda_desc_size(void);   /* sizeof(mi_rcda_desc) as compiled (binding self-check) */
int mi_rcda_key_mean(const void* key_row, const void* key_col, void* mean_row, void* mean_col, int B, int H, int W, int E,
                     mi_stream_t s);
int mi_rcda_fwd(const mi_rcda_desc* d, mi_stream_t s);
/* workspace bytes of mi_rcda_bwd for this geometry (pointers may be NULL), or < 0 */
int64_t mi_rcda_bwd_ws_bytes(const mi_rcda_desc* d);
int mi_rcda_bwd(const mi_rcda_desc* d, mi_stream_t s);

/* ---- SMCA: attention with a Gaussian-like spatial prior (csrc/mha.hip, the PRIOR instantiations) ------------
 * The cross-attention of SMCA-DETR's decoder (backbone/smcadetr_backbone.py:285-315, layers/smca_attention.py:277-278),
 * head_dim 32, operands as mi_mha_*_ld (bf16 [L][B][E] sequence-first, mask uint8 [B][Lk], lse fp32 [B][H][Lq]):
 *   logit[q][key] = scale * Q[q].K[key] + (mask[key] ? -inf : 0) + G[q][key]
 *   G[q][key]     = -| a dx^2 + b dy^2 + c dx^2 dy^2 | * inv_smooth,   dx = px - key % map_w,  dy = py - key / map_w
 *   O = dropout(softmax(logit)) V
 * point: fp32 [Lq][B][H][2] = (px, py); coef: fp32 [Lq][B][H][3] = (a, b, c), both contiguous; Lk == map_h * map_w.
 * The prior is evaluated in registers: no [B*H, Lq, Lk] tensor exists.  The backward also writes dpoint / dcoef (fp32, the
 * operands' shapes; d|x|/dx = sign(x), 0 at 0): row sums of the score gradient taken inside the dQ kernel in a fixed order
 * (no atomics, no workspace: bit-reproducible).  A fully padded query row gives O = 0, lse = -inf and zero gradients.
 * The dropout element index is mi_mha_dropout_mask's.  o_f32 (may be NULL): fp32 copy of O, written by the forward and read
 * by the backward's delta.  delta: fp32 [B][H][Lq] scratch of the backward.  Argument errors (null pointers, E != 32 H,
 * Lk != map_h * map_w, misaligned operands, Lq * Lk >= 2^32, drop_p outside [0, 1), inv_smooth not finite and positive)
 * return MI_EINVAL before any launch.  No entry allocates, reads back or synchronises. */
typedef struct mi_smca_desc {
  const void* q;
  const void* k;
  const void* v;
  const uint8_t* mask;  /* may be NULL                                                */
  const float* point;
  const float* coef;
  void* o;
  float* o_f32;         /* may be NULL                                                */
  float* lse;
  const void* dout;     /* backward only from here                                    */
  float* delta;
  void* dq;
  void* dk;
  void* dv;
  float* dpoint;
  float* dcoef;
  uint64_t seed;
  int32_t B, H, Lq, Lk, E;
  int32_t ldq, ldk;     /* row strides of q / dq and k / dk (>= E, multiples of 8)    */
  int32_t map_h, map_w;
  int32_t rsv_;
  float scale;          /* head_dim^-0.5 in the module                                */
  float inv_smooth;     /* 1 / smooth                                                 */
  float drop_p;
  float rsv2_;
} mi_smca_desc;
int mi_smca_desc_size(void);   /* sizeof(mi_smca_desc) as compiled (binding self-check) */
int mi_smca_fwd(const mi_smca_desc* d, mi_stream_t s);
int mi_smca_bwd(const mi_smca_desc* d, mi_stream_t s);

/* ---- depthwise 3x3 convolution ------------------------------------------------
 * the `dconv` of DWConv (backbone/layers/wrappers.py:86-102: BaseConv(C, C, ksize, stride, groups=C); the reference
 * builds it with ksize 3 everywhere, darknetx.py:113-160): NHWC bf16, pad 1, stride 1 or 2, C % 8 == 0.
 * w: the fp32 parameter tensor [C][1][3][3] (rounded to bf16 in the kernel like every conv operand).
 * fwd: y = dwconv(x); stats_acc (may be NULL): fp64 [nslots][rup(C,32)][2] (sum, sumsq) accumulators of the following
 *      BatchNorm, added to atomically exactly as the dense conv's epilogue does (caller zeroes them once per step).
 * dgrad: dx (+)= dwconv^T(dy).  wgrad: dw[C][1][3][3] fp32 = correlation(x, dy), overwritten, deterministic
 *      (block partials in ws, mi_dwconv3x3_wgrad_ws_bytes(C) bytes, summed in a fixed order). */
int mi_dwconv3x3_fwd(const void* x, int ldx, const float* w, void* y, int ldy, int N, int H, int W, int C, int stride,
                     int outH, int outW, double* stats_acc, int nslots, mi_stream_t s);
int mi_dwconv3x3_dgrad(const void* dy, int lddy, const float* w, void* dx, int lddx, int N, int H, int W, int C,
                       int stride, int outH, int outW, int accumulate, mi_stream_t s);
int64_t mi_dwconv3x3_wgrad_ws_bytes(int C);
int mi_dwconv3x3_wgrad(const void* x, int ldx, const void* dy, int lddy, int N, int H, int W, int C, int stride,
                       int outH, int outW, float* ws, int64_t ws_bytes, float* dw, mi_stream_t s);

/* ---- BatchNorm(train) + SiLU (+ residual) -----------------------------
 * replaces nn.BatchNorm2d + nn.SiLU of BaseConv (wrappers.py:76-80) and the
 * Bottleneck add (wrappers.py:119-123). */
/* the same BatchNorm pass of several independent layers in ONE launch (FPN levels of the head).
 * kind 0 = mi_bn_act_fwd, 1 = mi_bn_act_bwd_reduce, 2 = mi_bn_act_bwd_apply, 3 = mi_bn_act_bwd_fused; the fields of a job mean what the
 * arguments of those calls mean (acc = stats_acc / dacc).  All jobs share `act`. */
#define MI_BN_MAX_GROUP 8
typedef struct mi_bn_job {
  const void* y; const void* res; void* a;
  const void* da; void* dy; void* dres;
  double* acc;
  const float* gamma; const float* beta; float* rmean; float* rvar; int64_t* nbt;
  float* scale; float* shift; float* mean; float* invstd; float* dgamma; float* dbeta;
  int64_t npix, count;
  int32_t ldy, ldres, lda, ldda, lddy, lddres, dres_accum, C, nslots, nblk, act, pad_;
  float eps, momentum;
  uint32_t* bar; /* kind 3: the layer's barrier words (see mi_bn_act_bwd_fused) */
} mi_bn_job;
typedef struct mi_bn_group {
  int32_t kind, njobs, nblocks, act;
  int64_t starts_off, table_bytes;
} mi_bn_group;
int mi_bn_group_plan(int kind, const mi_bn_job* jobs, int n, void* table_host, int64_t table_cap, mi_bn_group* meta);
int mi_bn_group_run(const mi_bn_group* meta, const void* table_dev, mi_stream_t s);

/* eval mode: scale/shift from running statistics */
int mi_bn_eval_affine(const float* gamma, const float* beta, const float* running_mean,
                      const float* running_var, float eps, int C, float* scale, float* shift,
                      mi_stream_t s);
/* a = act(y*scale+shift) (+res); act: 1 silu, 0 identity.
 * train mode (stats_acc != NULL): scale/shift are first derived, in the kernel prologue, from the fp64
 * accumulators the conv epilogue filled ([nslots][C][2], `count` elements per channel); scale/shift/mean/
 * invstd [C] are written for the backward pass and the running statistics are updated exactly as
 * nn.BatchNorm2d does (momentum, unbiased running variance, num_batches_tracked).
 * eval mode (stats_acc == NULL): scale/shift are inputs (mi_bn_eval_affine). */
int mi_bn_act_fwd(const void* y, int ldy, const double* stats_acc, int nslots, int64_t count, const float* gamma,
                  const float* beta, float eps, float momentum, float* running_mean, float* running_var,
                  int64_t* num_batches_tracked, float* scale, float* shift, float* mean, float* invstd,
                  const void* res, int ldres, void* a, int lda, int64_t npix, int C, int act, mi_stream_t s);
/* pass 1: per-channel sums of dz and dz*xhat over pixels, atomically added to dacc[nslots][C][2] (fp64,
 * caller zeroes once per step); nblk = number of blocks to launch */
int mi_bn_act_bwd_reduce(const void* da, int ldda, const void* y, int ldy, const float* scale,
                         const float* shift, const float* mean, const float* invstd,
                         double* dacc, int nslots, int nblk, int64_t npix, int C, int act, mi_stream_t s);
/* pass 2: dy = gamma*invstd*(dz - c1 - xhat*c2), c1/c2 from dacc (prologue); writes dgamma/dbeta (overwrite);
 * optional dres (+)= da */
int mi_bn_act_bwd_apply(const void* da, int ldda, const void* y, int ldy, const float* scale,
                        const float* shift, const float* mean, const float* invstd,
                        const float* gamma, const double* dacc, int nslots, int64_t count, float* dgamma,
                        float* dbeta,
                        void* dy, int lddy, void* dres, int lddres, int dres_accum, int64_t npix, int C, int act,
                        mi_stream_t s);
/* both backward passes in ONE launch: every block stays resident, keeps its share of (da, y) in registers across a
 * grid-wide barrier and writes dy from them - 3 tensor passes instead of 5 (layers beyond the register capacity stream the
 * excess twice, as the two-pass form does).  Same arguments and results as reduce + apply; dacc must be zero on entry.
 * barrier_words: MI_BN_BAR_WORDS x uint32 of device memory (256-byte aligned) owned by this layer, zero before the first
 * use, not shared between launches that may run concurrently ([2] != 0 afterwards means a wait gave up: the launch was
 * not fully resident).
 * Must not run concurrently with another fused launch on the same device (both would wait for blocks that cannot start). */
#define MI_BN_BAR_GROUPS 16
#define MI_BN_BAR_WORDS (64 * (1 + 2 * MI_BN_BAR_GROUPS))
/* resident-block budget of the fused launches: 0 = everything the device runs at once (default); a data-parallel
 * trainer leaves headroom for the collective's kernels.  Returns the budget in effect. */
int mi_bn_fused_set_capacity(int blocks);
int mi_bn_act_bwd_fused(const void* da, int ldda, const void* y, int ldy, const float* scale, const float* shift,
                        const float* mean, const float* invstd, const float* gamma, double* dacc, int nslots,
                        int64_t count, float* dgamma, float* dbeta, void* dy, int lddy, void* dres, int lddres,
                        int dres_accum, int64_t npix, int C, int act, uint32_t* barrier_words, mi_stream_t s);

/* ---- train-mode BatchNorm + ReLU with a normed or plain residual (csrc/bn_relu.hip) ---------------
 * The layers and the block tail of a RegNet / ResNet block whose norms use batch statistics (backbone/regnet.py builds
 * detectron2's RegNet with norm = "SyncBN" and ReLU):  a = act(BN1(y1)),  a = act(BN1(y1) + BN2(y2))  (projection block
 * tail) or  a = act(BN1(y1) + res)  (identity block tail), one launch each, ONE rounding at the store.
 * Every tensor is a bf16 NHWC view (pointer, pixel stride) read and written in 16-byte pieces: C % 8 == 0, 0 < C <= 2048, every
 * leading dimension a multiple of 8 and >= C, base pointers 16-byte aligned; anything else returns MI_EINVAL naming the
 * quantity before any launch.  Channels [C, ld) of a row are never read and never written.
 * Statistics are the fp64 slot accumulators [nslots][roundup(C, 32)][2] of the conv epilogue and of mi_bn_act_fwd (the caller
 * zeroes them; nslots outside 1 .. MI_BN_SLOTS means MI_BN_SLOTS); block sums are fp32, added with fp64 atomics.
 *
 * mi_bn_stats: adds the per-channel (sum x, sum x^2) of a map into acc (slot = block % nslots) - for producers without a
 * statistics epilogue (mi_gconv_fwd).  Channels >= C of a slot and slots >= nslots are untouched.
 *
 * mi_bn_relu_norm: one norm operand.  Forward, train mode (acc != NULL): the prologue sums the slots in slot order and derives
 * scale / shift / mean / invstd; block 0 publishes them and updates running_mean / running_var / num_batches_tracked (each may
 * be NULL) exactly as mi_bn_act_fwd does.  Eval mode (acc == NULL): scale / shift are inputs (mi_bn_eval_affine).  Backward:
 * mean / invstd / gamma are inputs, dacc [nslots][roundup(C, 32)][2] receives (sum dz, sum dz * xhat) (zero on entry), dy / lddy
 * the operand's gradient, dgamma / dbeta (may be NULL) fp32 [C], overwritten.
 *
 * mi_bn_relu_desc: n1 is mandatory; n2 (n2.y != NULL) and res are optional and exclude each other.
 *   forward         a = bf16(act(y1 * scale1 + shift1 [+ y2 * scale2 + shift2 | + (float)res])), act = max(., 0) when relu, fp32
 *   backward        dz = da where the saved output a > 0, else 0 (relu == 0: dz = da; a is then not read and may be NULL)
 *     reduce        dacc_k += (sum dz, sum dz * xhat_k), xhat_k = (y_k - mean_k) * invstd_k, da and a read once for both operands
 *     apply         finalises the sums in its prologue (fixed slot order) and writes
 *                   dy_k = gamma_k * invstd_k * (dz - c1_k - xhat_k * c2_k), c = sums / count; dgamma_k = sum dz * xhat_k,
 *                   dbeta_k = sum dz; dres (may be NULL) = dz, or += dz when `accumulate`.  dz is recomputed from (da, a) -
 *                   except in the residual form with dres given and accumulate == 0: there REDUCE already writes dres = dz (it
 *                   is the residual's gradient) and apply reads it back instead of (da, a), 7 tensor passes instead of 8; dres
 *                   must then not alias da or a, and nothing may write it between the two launches. */
typedef struct mi_bn_relu_norm {
  const void* y;             /* raw convolution output; NULL in n2: operand absent                              */
  const double* acc;         /* forward: statistics accumulators, NULL = eval mode                              */
  const float* gamma;
  const float* beta;
  float* running_mean;
  float* running_var;
  int64_t* num_batches_tracked;
  float* scale;
  float* shift;
  float* mean;
  float* invstd;
  double* dacc;              /* backward: (sum dz, sum dz * xhat) accumulators                                  */
  void* dy;                  /* backward, apply: gradient of y                                                   */
  float* dgamma;
  float* dbeta;
  int64_t count;             /* elements per channel behind the statistics (N * H * W)                          */
  int32_t ldy, lddy, nslots, rsv_;
  float eps, momentum;
} mi_bn_relu_norm;
typedef struct mi_bn_relu_desc {
  mi_bn_relu_norm n1, n2;
  const void* res;           /* forward: plain residual or NULL                                                 */
  void* a;                   /* forward: output; backward: the saved output (read)                              */
  const void* da;            /* backward: gradient of a                                                          */
  void* dres;                /* backward, apply: gradient of res or NULL                                         */
  int64_t npix;
  int32_t ldres, lda, ldda, lddres;
  int32_t C, relu, accumulate, rsv_;
} mi_bn_relu_desc;
int mi_bn_relu_desc_size(void);   /* sizeof(mi_bn_relu_desc) as compiled (binding self-check) */
int mi_bn_stats(const void* x, int ldx, int64_t npix, int C, double* acc, int nslots, mi_stream_t s);
int mi_bn_relu_fwd(const mi_bn_relu_desc* d, mi_stream_t s);
int mi_bn_relu_bwd_reduce(const mi_bn_relu_desc* d, mi_stream_t s);
int mi_bn_relu_bwd_apply(const mi_bn_relu_desc* d, mi_stream_t s);

/* ---- data movement ops -------------------------------------------------- */
/* Focus space-to-depth (wrappers.py:202-220) fused with fp32 NCHW -> bf16 NHWC and 12->16 ch pad */
int mi_focus_pack(const float* img_nchw, int N, int H, int W, void* out, int ldo, mi_stream_t s);
/* same from the uint8 NCHW image of the data loader (preprocess_image's .type(torch.float), yolox.py:96-99, fused) */
int mi_focus_pack_u8(const uint8_t* img_nchw, int N, int H, int W, void* out, int ldo, mi_stream_t s);
/* nn.Upsample(2,"nearest") (yolo_pafpn.py:28) into a concat slice, and its gradient */
int mi_upsample2x_fwd(const void* x, int ldx, void* y, int ldy, int N, int H, int W, int C,
                      mi_stream_t s);
int mi_upsample2x_bwd(const void* dy, int lddy, void* dx, int lddx, int accumulate, int N, int H,
                      int W, int C, mi_stream_t s);
/* SPP max-pools k=5,9,13 s1 (wrappers.py:150-153): three outputs + argmax codes; idx: 6*N*H*W*C bytes
 * (separable argmax: 3 planes of vertical codes, 3 of horizontal codes); H*W <= 512 for the backward */
int mi_spp_pool_fwd(const void* x, int ldx, void* y5, void* y9, void* y13, int ldy, uint8_t* idx,
                    int N, int H, int W, int C, mi_stream_t s);
int mi_spp_pool_bwd(const void* dy5, const void* dy9, const void* dy13, int lddy,
                    const uint8_t* idx, void* dx, int lddx, int accumulate, int N, int H, int W,
                    int C, mi_stream_t s);
/* nn.MaxPool2d(kernel_size=3, stride=2, padding=1) of detectron2's ResNet stem (BasicStem.forward; d2 upstream), bf16
 * NHWC views, C %% 8 == 0.  outH = (H + 1) / 2.  Backward routes each output gradient to the FIRST maximum of its
 * window in row-major order (ATen's tie rule): dx (+)= sum over the <= 4 windows that contain the pixel. */
int mi_maxpool3x3s2_fwd(const void* x, int ldx, void* y, int ldy, int N, int H, int W, int C, mi_stream_t s);
/* the same pooling recording, per output element, the window position (0..8, row-major) of its first maximum in
 * code[N][Ho][Wo][C] (uint8, 8-byte aligned), and the backward that reads the codes instead of re-deriving them from x:
 * identical results (torch's MaxPool2d gradient goes to the first maximum), a twentieth of the time on the stem's map */
int mi_maxpool3x3s2_fwd_idx(const void* x, int ldx, void* y, int ldy, uint8_t* code, int N, int H, int W, int C, mi_stream_t s);
int mi_maxpool3x3s2_bwd_idx(const uint8_t* code, const void* dy, int lddy, void* dx, int lddx, int accumulate, int N, int H,
                            int W, int C, mi_stream_t s);
int mi_maxpool3x3s2_bwd(const void* x, int ldx, const void* dy, int lddy, void* dx, int lddx, int accumulate, int N,
                        int H, int W, int C, mi_stream_t s);
/* nn.AvgPool2d(2, 2, ceil_mode=True, count_include_pad=False) in front of a ResNet-vd projection shortcut
 * (yolov7/modeling/backbone/resnetvd.py:157-182 downsample_avg), bf16 NHWC views, C %% 8 == 0, pixel strides multiples of 8,
 * 16-byte aligned pointers.  outH = (H + 1) / 2, outW = (W + 1) / 2.  Forward: the fp32 sum, in row-major window order, of
 * the 1, 2 or 4 inputs inside the map, divided by that count, rounded once to bf16.  Backward: EVERY input pixel (iy, ix)
 * is written: dx = dy[iy / 2][ix / 2] / count (+ the value already in dx when accumulate != 0, added in fp32), rounded once
 * to bf16, then zeroed where mask <= 0 when mask != NULL (mask: the ReLU output the pooled map was taken from; the bits of
 * mi_ew_bf16 op 2 applied afterwards). */
int mi_avgpool2x2s2_fwd(const void* x, int ldx, void* y, int ldy, int N, int H, int W, int C, mi_stream_t s);
int mi_avgpool2x2s2_bwd(const void* dy, int lddy, void* dx, int lddx, const void* mask, int ldmask, int accumulate, int N,
                        int H, int W, int C, mi_stream_t s);
/* ---- deformable 3x3 convolution, staged (csrc/deform_conv.hip): detectron2's DeformConv, unmodulated, one deformable
 * group, groups 1.  bf16 NHWC maps, C %% 32 == 0.  offset: bf16 NHWC with pixel stride ldoff >= 18, read where the offset
 * convolution wrote it; for tap t = i*3 + j channel 2t is the row offset, 2t + 1 the column offset.  Sample point of output
 * pixel (ho, wo): h = ho*stride - pad + i*dil + off_h (w alike); it counts only if h > -1 && w > -1 && h < H && w < W, the cell
 * is floor(h), floor(h) + 1, a corner outside [0, H-1] x [0, W-1] contributes zero, interpolation in fp32.
 * Served: stride 1 or 2, pad 1, dil 1 (outH = (H - 1) / stride + 1); anything else returns MI_EINVAL and launches nothing.
 * mi_deform_im2col: col[N*outH*outW][9*C] bf16, tap-major with the C channels of a tap contiguous; the convolution is then the
 *   1x1 convolution of col with the weight permuted to [Cout][tap][C] (mi_conv2d).
 * mi_deform_col2im: from dcol (the 1x1 data gradient, col's layout), x and offset: d_offset[N][outH][outW][32] bf16 (fp32 sums
 *   over C; channels 18..31 written as zero; a sample at an integer coordinate takes the right-hand difference) and
 *   dx32[N][H][W][C] += dcol * corner weight with fp32 atomics (clear it with mi_deform_zero_f32 first).  grid_max: NULL, or
 *   a device float holding max |dcol| (mi_deform_absmax into a zeroed float): every addend is then rounded to a multiple of
 *   2^(e - 16), 2^e >= that maximum, so that the additions are exact and the sums do not depend on the order the atomics
 *   arrive in (bit-reproducible dx; up to 256 addends of the largest magnitude per element).
 * mi_deform_dx_finish: dx = bf16(dx32), zeroed where mask <= 0 when mask != NULL (mask: the ReLU output x was; mi_ew_bf16 op 2). */
int mi_deform_im2col(const void* x, int ldx, const void* offset, int ldoff, void* col, int N, int H, int W, int C, int stride,
                     int pad, int dil, mi_stream_t s);
int mi_deform_col2im(const void* dcol, const void* x, int ldx, const void* offset, int ldoff, float* dx32, void* d_offset,
                     const float* grid_max, int N, int H, int W, int C, int stride, int pad, int dil, mi_stream_t s);
int mi_deform_absmax(const void* v, int64_t n, float* out, mi_stream_t s);
int mi_deform_zero_f32(float* p, int64_t n, mi_stream_t s);
int mi_deform_dx_finish(const float* dx32, const void* mask, int ldmask, void* dx, int lddx, int64_t npix, int C, mi_stream_t s);
/* generic strided bf16 NHWC copy / accumulate (dst (+)= src) */
int mi_copy_bf16(const void* src, int lds_, void* dst, int ldd, int accumulate, int64_t npix, int C,
                 mi_stream_t s);
/* column sums of a bf16 NHWC view -> fp32 [C] (bias gradient of the prediction convs) */
int mi_colsum_bf16(const void* x, int ldx, int64_t npix, int C, float* out, int accumulate, float* ws,
                   mi_stream_t s);
/* the same for any channel count (a multiple of 8 readable) in one launch pair; ws: mi_colsum_wide_ws_bytes(C) bytes.
 * Bias gradients of nn.Linear in the transformer (backbone/detr_backbone.py:140-230: 256 .. 2048 output channels). */
int64_t mi_colsum_wide_ws_bytes(int C);
int mi_colsum_bf16_wide(const void* x, int ldx, int64_t npix, int C, float* out, int accumulate, float* ws, mi_stream_t s);
/* the same over the SQUARES of the values (fp32 products): column norms^2 */
int mi_colsumsq_bf16_wide(const void* x, int ldx, int64_t npix, int C, float* out, int accumulate, float* ws, mi_stream_t s); /* ws: >= 128*128 floats of scratch (two-stage, fixed summation order) */

/* ---- YOLOX head: decode + SimOTA + losses ---------------------------------
 * replaces YOLOXHead.get_output_and_grid / get_losses / get_assignments /
 * get_in_boxes_info / dynamic_k_matching (head/yolox_head.py:226-669),
 * bboxes_iou and IOUloss (utils/boxes.py:57-81,125-168). */
typedef struct mi_yolox_loss_desc {
  const float* preds;   /* [B][A][5+ncls] raw head outputs (xy,wh undecoded; logits)        */
  const float* labels;  /* [B][max_labels][5] (cls,cx,cy,w,h), zero rows = padding          */
  const float* anchors; /* [A][3] (grid_x, grid_y, stride)                                   */
  int32_t B, A, ncls, max_labels;
  int32_t gmax;         /* upper bound on valid labels per image (<= max_labels)             */
  /* workspaces (caller-owned) */
  float* cost;          /* [B][gmax][A]                                                       */
  float* iou;           /* [B][gmax][A]                                                       */
  uint8_t* match;       /* unused since round 2 (the match matrix became a per-anchor counter); may be NULL       */
  int32_t* ngt;         /* [B]                                                                */
  /* assignment outputs */
  uint8_t* fg;          /* [B][A] final foreground mask                                       */
  int32_t* matched_gt;  /* [B][A] index of matched gt or -1                                   */
  float* matched_iou;   /* [B][A]                                                             */
  float* partial;       /* [nblk][4] block partial sums (iou, obj, cls, nfg); nblk = B*ceil(A/256) */
  float* out;           /* [8]: total, 5*iou, obj, cls, l1, num_fg/num_gt, num_fg, num_gt */
  /* head.use_l1 (yolox_head.py:131, switched on by the meta-arch after INPUT.MOSAIC_AND_MIXUP.DISABLE_AT_ITER,
   * meta_arch/yolox.py:105-118): adds sum|raw_reg - get_l1_target| / num_fg to the total; 0 = the default */
  int32_t use_l1, rsv_;
  float* partial_l1;    /* [nblk] (use_l1 only) */
  /* the YOLOv6 head's form of this loss (ComputeLoss, head/yolov6_head.py:315-754) differs in constants only; a zero
   * selects the YOLOX value: centre radius 2.5, SimOTA cost weights cls 1 / iou 3, box-loss weight 5 */
  float center_radius, cls_weight, iou_weight, reg_weight;
  int32_t iou_type;     /* box loss: 0 IOUloss "iou" (1 - iou^2); 1..4 IOUlossV6 giou / diou / ciou / siou, eps 1e-7 */
  int32_t rsv2_;
} mi_yolox_loss_desc;
int mi_yolox_loss_fwd(const mi_yolox_loss_desc* d, mi_stream_t s);
/* gradient wrt raw preds; gw[4] = upstream grads of (total, 5*iou, obj, cls) on device (+ gw[4] = of l1 iff use_l1).
 * dpreds fp32 [B][A][5+ncls] and/or bf16 per-level NHWC maps (see plan builder). */
int mi_yolox_loss_bwd(const mi_yolox_loss_desc* d, const float* gw, float* dpreds, mi_stream_t s);
/* extract channels [c0, c0+nc) of dpreds fp32 [B][A][nch] for anchors a0..a0+HW into a bf16
 * NHWC map dst [B][HW][ld] (channels >= nc zero-filled): the out-gradient of one prediction conv. */
int mi_yolox_split_dpreds(const float* dpreds, int B, int A, int nch, int a0, int HW, int c0, int nc,
                          void* dst, int ld, mi_stream_t s);
/* bias gradients of all prediction convs (nn.Conv2d bias of yolox_head.py:103-129) in two launches:
 * out[c] = sum_b sum_{a0 <= a < a0+HW} dpreds[b][a][c0 + c]; jobs is a HOST array (<= 16);
 * ws: 16*512*128 floats of scratch = 16 slabs; a call uses (distinct (a0, HW) levels) x ceil(nch / 128) of them
 * (3 levels: nch <= 640, i.e. up to 635 classes) */
typedef struct mi_bias_job {
  float* out;
  int32_t a0, HW, c0, nc;
} mi_bias_job;
int mi_yolox_bias_grads(const float* dpreds, int B, int A, int nch, const mi_bias_job* jobs, int njobs, float* ws,
                        mi_stream_t s);
/* the out-gradient maps of ALL prediction convs in one launch (the per-conv form is mi_yolox_split_dpreds):
 * dst[b][pix][0..ld) (bf16, ld % 8 == 0) = dpreds[b][a0 + pix][c0 .. c0 + nc), pad channels zero. */
typedef struct mi_split_job {
  void* dst;
  int32_t a0, HW, c0, nc, ld, rsv_;
} mi_split_job;
int mi_yolox_split_dpreds_batch(const float* dpreds, int B, int A, int nch, const mi_split_job* jobs, int njobs,
                                mi_stream_t s);
/* mi_yolox_loss_bwd + mi_yolox_split_dpreds_batch + mi_yolox_bias_grads in ONE pass over the gradient: every value is
 * computed once and written as the bf16 out-gradient map of its prediction conv, into per-block column sums and - only when
 * dpreds is not NULL (tests / diagnostics) - as fp32 dpreds [B][A][5 + ncls]; per-block column sums (bias gradients; a second small launch adds the blocks).  The split jobs must tile [A][5 + ncls]
 * exactly (each job = the box columns, the objectness column or class columns of one level); every bias job must name the
 * (a0, HW, c0, nc) of one split job.  ws: scratch of ws_floats floats (>= njobs * max ld; 16 * 512 * 128 serves all plans). */
int mi_yolox_loss_bwd_fused(const mi_yolox_loss_desc* d, const float* gw, float* dpreds, const mi_split_job* split_jobs,
                            int nsplit, const mi_bias_job* bias_jobs, int nbias, float* ws, int64_t ws_floats, mi_stream_t s);
/* eval decode (yolox_head.py:247-272): in-place on preds; obj/cls sigmoid applied */
int mi_yolox_decode(float* preds, const float* anchors, int B, int A, int ncls, mi_stream_t s);
/* the ONNX-export layout of decode_outputs (yolox_head.py:263-269) from the decoded predictions:
 * out [B][A][6+ncls] = (xy, wh, conf, argmax(prob) as float - first maximum, prob) */
int mi_yolox_onnx_layout(const float* decoded, float* out, int B, int A, int ncls, mi_stream_t s);

/* ---- DETR set matching (config 4) --------------------------------------------------
 * replaces HungarianMatcher.forward (utils/detr_utils.py:37-91): matching cost
 * C = w_bbox*L1(cdist) + w_class*(-softmax(logits)[label]) + w_giou*(-GIoU) per image, then
 * scipy.optimize.linear_sum_assignment (detr_utils.py:89) - which the reference runs on the CPU.
 * logits [B][Q][NC], boxes [B][Q][4] cxcywh, tgt_labels int64 [T], tgt_boxes [T][4] cxcywh,
 * tgt_off int32 [B+1] (targets of image b = [tgt_off[b], tgt_off[b+1])), gmax >= max targets per image.
 * cost (workspace / output) fp32 [B][Q][gmax]; match_q / match_t int64 [B][gmax]: the first nmatch[b] =
 * min(Q, G_b) entries are the (query, target) pairs sorted by query index, exactly what scipy returns.
 * Q, gmax <= 1024. */
int mi_hungarian_match(const float* logits, const float* boxes, const int64_t* tgt_labels,
                       const float* tgt_boxes, const int32_t* tgt_off, int B, int Q, int NC, int gmax,
                       float w_class, float w_bbox, float w_giou, float* cost, int64_t* match_q,
                       int64_t* match_t, int32_t* nmatch, mi_stream_t s);
/* the assignment alone on a caller-provided cost matrix (same layout) */
int mi_lsap(const float* cost, const int32_t* tgt_off, int B, int Q, int gmax, int64_t* match_q,
            int64_t* match_t, int32_t* nmatch, mi_stream_t s);

/* DETR set-prediction losses for the match indices above, forward + backward.
 * replaces SetCriterion.loss_labels / loss_cardinality / loss_boxes (modeling/meta_arch/detr.py:504-556) and their
 * autograd backward.  NC = num_classes + 1 (last class = no-object, weight eos_coef); num_boxes as detr.py:615-619
 * computes it (host).  losses[8] = loss_ce, class_error, cardinality_error, loss_bbox, loss_giou, sum of CE weights,
 * matched pairs, 0.  rowstate: caller workspace of B*Q*16 floats, written by fwd and read by bwd.
 * bwd: gw[3] on device = upstream gradients of (loss_ce, loss_bbox, loss_giou); dlogits [B][Q][NC], dboxes [B][Q][4].
 * B <= 256. */
typedef struct mi_detr_loss_desc {
  const float* logits;
  const float* boxes;
  const int64_t* tgt_labels;
  const float* tgt_boxes;
  const int32_t* tgt_off;
  const int64_t* match_q;
  const int64_t* match_t;
  const int32_t* nmatch;
  int32_t B, Q, NC, gmax;
  float eos_coef, num_boxes;
  float* losses;
  float* rowstate;
} mi_detr_loss_desc;
int mi_detr_set_loss_fwd(const mi_detr_loss_desc* d, mi_stream_t s);
int mi_detr_set_loss_bwd(const mi_detr_loss_desc* d, const float* gw, float* dlogits, float* dboxes, mi_stream_t s);

/* ---- focal set matching and criterion (SMCA-DETR, Anchor DETR) ------------------------
 * mi_hungarian_match_focal replaces HungarianMatcherSMCA.forward / HungarianMatcherAnchorDETR.forward
 * (utils/detr_utils.py:119-176, 202-262 - the same computation): mi_hungarian_match with the sigmoid focal class cost
 * p = sigmoid(logits[label]), cost_class = alpha (1 - p)^2 (-log(p + 1e-8)) - (1 - alpha) p^2 (-log(1 - p + 1e-8))
 * (the reference fixes alpha = 0.25, gamma = 2).  NC = number of channels (no no-object channel).  Same layouts and limits
 * (Q, gmax <= 1024).  nmatch[b] = -1 for an image with a NaN / inf cost (scipy raises ValueError there); such an image is
 * not assigned and its match_q / match_t rows are left as they were. */
int mi_hungarian_match_focal(const float* logits, const float* boxes, const int64_t* tgt_labels,
                             const float* tgt_boxes, const int32_t* tgt_off, int B, int Q, int NC, int gmax,
                             float w_class, float w_bbox, float w_giou, float alpha, float* cost, int64_t* match_q,
                             int64_t* match_t, int32_t* nmatch, mi_stream_t s);
/* The set criterion of those two models for the match indices above, forward + backward.
 * replaces SetCriterion.loss_labels / loss_cardinality / loss_boxes of modeling/meta_arch/smca_detr.py:546-613 and
 * anchor_detr.py:570-631 and their autograd backward: sigmoid focal loss (detr_seg.py:207-270, gamma 2) over the NC
 * channels, target 1 only at a matched row's label, summed / num_boxes; alpha < 0 = no alpha weighting.
 * losses[8] = loss_ce, class_error (100 without a pair), cardinality_error (mean over images of |#rows whose arg max is
 * not channel NC - 1, minus G_b|: the reference's convention on this head), loss_bbox, loss_giou, 0, matched pairs, 0.
 * rowstate: caller workspace of B*Q*16 floats, written by fwd and read by bwd.
 * bwd: gw[3] on device = upstream gradients of (loss_ce, loss_bbox, loss_giou); dlogits [B][Q][NC], dboxes [B][Q][4]
 * (exactly 0 in rows without a match).  B <= 256. */
typedef struct mi_focal_loss_desc {
  const float* logits;
  const float* boxes;
  const int64_t* tgt_labels;
  const float* tgt_boxes;
  const int32_t* tgt_off;
  const int64_t* match_q;
  const int64_t* match_t;
  const int32_t* nmatch;
  int32_t B, Q, NC, gmax;
  float alpha, num_boxes;
  float* losses;
  float* rowstate;
} mi_focal_loss_desc;
int mi_focal_set_loss_fwd(const mi_focal_loss_desc* d, mi_stream_t s);
int mi_focal_set_loss_bwd(const mi_focal_loss_desc* d, const float* gw, float* dlogits, float* dboxes, mi_stream_t s);
/* sizeof(mi_focal_loss_desc) as compiled into the library (binding self-check; mi_abi_sizeof's id list is closed) */
int mi_focal_loss_desc_sizeof(void);

/* ---- focal top-k postprocess and the SMCA box head tail (SMCA-DETR, Anchor DETR) ------------------------
 * mi_focal_topk_postprocess replaces SMCADetr.inference (meta_arch/smca_detr.py:216-264) + detector_postprocess, and
 * PostProcess of anchor_detr.py, for the whole batch in one launch (one block per image).
 * logits fp32 [B][Q][C]; boxes fp32 [B][Q][4] normalised cxcywh; sizes_dev int64 [B][2] = (h, w) of each image on the device;
 * out_sizes int64 [B][2] = (out_h, out_w) on the device, or NULL.  Per image the K entries with the largest logit win (the
 * sigmoid is monotonic), ties towards the lower flat index q * C + c, -0 == +0, NaN greatest (as torch.topk), +-inf ordinary.
 * Output position 0 is the best; positions descend by (logit, then ascending index).  scores [B][K] = sigmoid(logit),
 * labels int64 [B][K] = idx % C, query int32 [B][K] = idx / C, boxes_xyxy [B][K][4] =
 * (cx - 0.5 w, cy - 0.5 h, cx + 0.5 w, cy + 0.5 h) * (w_img, h_img, w_img, h_img); with out_sizes then * (float) (out_w / w_img),
 * (float) (out_h / h_img) (quotients in double, as detector_postprocess forms them) and clamped to [0, out_w] x [0, out_h].
 * No float atomics, a pure function of its inputs.  Refused (MI_EINVAL, nothing launched): K > Q * C (torch.topk raises),
 * K > 1024, Q * C >= 2^31. */
int mi_focal_topk_postprocess(const float* logits, const float* boxes, const int64_t* sizes_dev, const int64_t* out_sizes,
                              int B, int Q, int C, int K, float* scores, int64_t* labels, int32_t* query, float* boxes_xyxy,
                              mi_stream_t s);
/* y[l][b][q][:] = sigmoid(x[l][b][q][:] + (p[b][q][0], p[b][q][1], 0, 0)): the SMCA box head (smca_detr.py:500-503); x, y fp32
 * [L][B][Q][4], p fp32 [B][Q][2] broadcast over the L decoder levels.
 * bwd: dx = dy * y * (1 - y) with y recomputed from x + p; dp[b][q][j] = sum over l ascending of dx[l][b][q][j] in fp32, one
 * thread per (b, q): no atomics, bit-reproducible. */
int mi_box_ref_sigmoid_fwd(const float* x, const float* p, float* y, int L, int B, int Q, mi_stream_t s);
int mi_box_ref_sigmoid_bwd(const float* x, const float* p, const float* dy, float* dx, float* dp, int L, int B, int Q, mi_stream_t s);

/* ---- multi-head attention core (DETR, config 4) -------------------------------------
 * O = softmax(scale * Q K^T + key_padding_mask) V per (batch, head); head_dim = 32 (DETR: 256 = 8 x 32).
 * replaces the attention inside nn.MultiheadAttention as called by the transformer layers
 * (modeling/backbone/detr_backbone.py:140,155-157,200-202,222-230).  Tensors are bf16 [L][B][E] (sequence first,
 * E = H*32: the layout nn.MultiheadAttention's in-projection produces; = NHWC "pixel l*B+b, channel h*32+d", so
 * the projections are 1x1 convolutions of this library).  key_padding_mask uint8 [B][Lk] (1 = ignore) or NULL;
 * lse fp32 [B][H][Lq] is saved for the backward; delta_ws: fp32 [B][H][Lq] scratch.  No attention-weight dropout. */
int mi_mha_fwd(const void* q, const void* k, const void* v, const uint8_t* key_padding_mask, void* o, float* lse,
               int B, int H, int Lq, int Lk, int E, float scale, mi_stream_t s);
int mi_mha_bwd(const void* q, const void* k, const void* v, const uint8_t* key_padding_mask, const void* o,
               const float* lse, const void* dout, float* delta_ws, void* dq, void* dk, void* dv, int B, int H,
               int Lq, int Lk, int E, float scale, mi_stream_t s);
/* the same with attention-weight dropout (nn.MultiheadAttention(dropout=p) in training mode, detr_backbone.py:140):
 * survivors scaled by 1/(1-p); the keep mask is a pure function of (seed, ((b*H+h)*Lq+q)*Lk+key), recomputed by the
 * backward - pass the SAME p and seed to both.  mi_mha_dropout_mask writes that mask (uint8 [B][H][Lq][Lk]) for tests. */
int mi_mha_fwd_dropout(const void* q, const void* k, const void* v, const uint8_t* key_padding_mask, void* o, float* lse,
                       int B, int H, int Lq, int Lk, int E, float scale, float drop_p, uint64_t seed, mi_stream_t s);
int mi_mha_bwd_dropout(const void* q, const void* k, const void* v, const uint8_t* key_padding_mask, const void* o,
                       const float* lse, const void* dout, float* delta_ws, void* dq, void* dk, void* dv, int B, int H,
                       int Lq, int Lk, int E, float scale, float drop_p, uint64_t seed, mi_stream_t s);
int mi_mha_dropout_mask(uint8_t* out, int B, int H, int Lq, int Lk, float drop_p, uint64_t seed, mi_stream_t s);
/* the same again with an fp32 copy of the output, o_f32 [Lq][B][E] (NULL = the forms above): the forward writes it, the
 * backward takes delta = rowsum(dO o O) from it.  dS = P o (dP - delta) cancels to a few percent of its operands whenever
 * the values of a row's keys are alike (every attention of a freshly initialised DETR); the 2^-9 rounding of a bf16 O is
 * coherent over the row and leaves that difference as a 30 - 80 % error of dq (measured on device operands, tools/
 * attn_bwd_error.py: dq rel 0.78 -> 0.0014).  4 bytes per output element, read once by the backward. */
int mi_mha_fwd_dropout_o32(const void* q, const void* k, const void* v, const uint8_t* key_padding_mask, void* o, float* o_f32,
                           float* lse, int B, int H, int Lq, int Lk, int E, float scale, float drop_p, uint64_t seed,
                           mi_stream_t s);
int mi_mha_bwd_dropout_o32(const void* q, const void* k, const void* v, const uint8_t* key_padding_mask, const void* o,
                           const float* o_f32, const float* lse, const void* dout, float* delta_ws, void* dq, void* dk,
                           void* dv, int B, int H, int Lq, int Lk, int E, float scale, float drop_p, uint64_t seed,
                           mi_stream_t s);
/* and with row strides for q / dq (ldq) and k / dk (ldk), in elements, >= E: a self-attention whose query and key are the
 * same tensor (the encoder layers and the decoder's self-attention, detr_backbone.py:155-157,222-224: q = k = x + pos) takes
 * q and k from ONE [T, 2E] projection (k = q + E, ldq = ldk = 2E) and hands dq | dk back the same way - one projection, one
 * data-gradient and one weight-gradient launch instead of two each.  v, o, dout, dv, o_f32 keep row stride E. */
int mi_mha_fwd_dropout_ld(const void* q, int ldq, const void* k, int ldk, const void* v, const uint8_t* key_padding_mask,
                          void* o, float* o_f32, float* lse, int B, int H, int Lq, int Lk, int E, float scale, float drop_p,
                          uint64_t seed, mi_stream_t s);
int mi_mha_bwd_dropout_ld(const void* q, int ldq, const void* k, int ldk, const void* v, const uint8_t* key_padding_mask,
                          const void* o, const float* o_f32, const float* lse, const void* dout, float* delta_ws, void* dq,
                          void* dk, void* dv, int B, int H, int Lq, int Lk, int E, float scale, float drop_p, uint64_t seed,
                          mi_stream_t s);
/* elementwise dropout of a bf16 tensor (F.dropout of detr_backbone.py:147-150,163-167,...): out[i] = keep(seed, i) ?
 * x[i] / (1-p) : 0; applying it with the same (p, seed) to the output gradient IS the backward. n %% 8 == 0. */
int mi_dropout_bf16(const void* x, void* out, int64_t n, float drop_p, uint64_t seed, mi_stream_t s);
/* out = res + dropout(x): the residual add that follows every F.dropout of the transformer layers
 * (detr_backbone.py:163,167,235,239,243: `src = src + self.dropout1(src2)`) in the same pass; the dropped value is rounded
 * to bf16 before the fp32 add, so the result equals mi_dropout_bf16 followed by mi_ew_bf16(op 0) bit for bit.  res NULL:
 * mi_dropout_bf16. */
int mi_dropout_add_bf16(const void* x, const void* res, void* out, int64_t n, float drop_p, uint64_t seed, mi_stream_t s);
/* The post-norm residual of the transformer layers in one pass (detr_backbone.py:163-168,235-243:
 * `src = self.norm1(src + self.dropout1(src2))`): sum_out = bf16(res + dropout(x)) - the bits mi_dropout_add_bf16 writes -
 * and y / mean / rstd = mi_layernorm_fwd(sum_out).  mi_layernorm_bwd_dropout is mi_layernorm_bwd that ALSO writes
 * dx_drop = dropout(dx) with the forward's (p, seed): the gradient of the dropped branch (dx itself is the residual's).
 * dx_drop NULL: mi_layernorm_bwd. */
int mi_dropout_add_layernorm_fwd(const void* x, const void* res, void* sum_out, const float* gamma, const float* beta, void* y,
                                 float* mean, float* rstd, int T, int E, float eps, float drop_p, uint64_t seed, mi_stream_t s);
int mi_layernorm_bwd_dropout(const void* x, const void* dy, const float* gamma, const float* mean, const float* rstd, void* dx,
                             void* dx_drop, float* dgamma, float* dbeta, float* ws, int T, int E, float drop_p, uint64_t seed,
                             mi_stream_t s);
/* A step captured as a hipGraph bakes its seeds into the kernel arguments.  With a device word registered here every
 * dropout kernel launched afterwards (mi_dropout_bf16, mi_mha_*_dropout, forward and backward alike) uses seed + *dev_word,
 * read at RUN time: advance the word once per replay (after the backward) and every replay draws fresh masks while the
 * backward of a step still recomputes its own forward's.  NULL (default) switches it off.  Process-global, not per stream. */
int mi_dropout_seed_offset(const uint64_t* dev_word);

/* ---- row-wise ops of DETR's transformer layers (detr_backbone.py:135-278) -------------------
 * nn.LayerNorm(E) forward / backward over bf16 [T][E] token rows (fp32 gamma/beta/mean/rstd), eps 1e-5;
 * E %% 64 == 0, E <= 1024; ws (backward): fp32 [ceil(T/16)][E][2].  mi_ew_bf16: op 0 out = a + b (residual),
 * op 1 out = relu(a), op 2 out = a * (b > 0) (ReLU backward: a = dy, b = forward output), op 3 out = sigmoid(a),
 * op 4 out = a * b * (1 - b) (sigmoid backward: a = dy, b = forward output); op 5 / 6 swish and its backward; op 7 out =
 * relu(a + b) (the tail of a ResNet bottleneck, bit-identical to op 0 followed by op 1); n %% 8 == 0. */
int mi_layernorm_fwd(const void* x, const float* gamma, const float* beta, void* y, float* mean, float* rstd, int T,
                     int E, float eps, mi_stream_t s);
int mi_layernorm_bwd(const void* x, const void* dy, const float* gamma, const float* mean, const float* rstd, void* dx,
                     float* dgamma, float* dbeta, float* ws, int T, int E, mi_stream_t s);
int mi_ew_bf16(const void* a, const void* b, void* out, int64_t n, int op, mi_stream_t s);

/* ---- IoU-family regression losses (CIoU / DIoU / GIoU / SIoU / IoU) with gradient ------
 * replaces IOUlossV6.__call__ + its autograd backward (utils/boxes.py:666-752; YOLOv6 head, yolov6_head.py:346,512):
 * loss[n] = 1 - iou_variant(pred[n], target[n]) (reduction "none"), dpred[n][4] = dloss[n] * d loss / d pred
 * (dloss NULL => ones; CIoU's alpha is a constant for the gradient, as under torch.no_grad()).
 * pred/target fp32 [n][4] in (cx,cy,w,h) (box_xyxy 0) or (x1,y1,x2,y2); iou_type: 0 iou, 1 giou, 2 diou, 3 ciou, 4 siou */
int mi_iou_loss_v6(const float* pred, const float* target, int n, int iou_type, int box_xyxy, float eps,
                   const float* dloss, float* loss, float* dpred, mi_stream_t s);

/* IOUloss of the YOLOX head as a standalone op (utils/boxes.py:125-168): boxes (cx,cy,w,h) fp32 [n][4];
 * loss_type 0 "iou" (1 - iou^2), 1 "giou" (1 - clamp(giou, -1, 1)); loss[n] (reduction "none") and
 * dpred[n][4] = dloss[n] * d loss / d pred (dloss NULL => ones).  Either output may be NULL. */
int mi_yolox_iou_loss(const float* pred, const float* target, int n, int loss_type, const float* dloss, float* loss,
                      float* dpred, mi_stream_t s);
/* pairwise IoU matrix out[N][M]: bboxes_iou (utils/boxes.py:57-81) and pairwise_bbox_iou (utils/boxes.py:755-779);
 * boxes (cx,cy,w,h) (box_xyxy 0) or (x1,y1,x2,y2) */
int mi_pairwise_bbox_iou(const float* box1, const float* box2, int N, int M, int box_xyxy, float* out, mi_stream_t s);

/* ---- BiFPN neck (neck/bifpn.py:184-395, build_resnet_bifpn_backbone) -------------------
 * GroupNorm = detectron2 get_norm("GN") = nn.GroupNorm(32, C) (MODEL.BIFPN.NORM default): NHWC bf16, x [N][HW][ldx],
 * C % 8 == 0, C % G == 0 (C / G need not be a multiple of 8), eps as nn.GroupNorm (1e-5).  mean_rstd [N][G][2] is written
 * by fwd and read by bwd; ws: mi_groupnorm_ws_bytes(N, C) bytes of scratch (zeroed inside).  bwd overwrites dgamma / dbeta. */
int64_t mi_groupnorm_ws_bytes(int N, int C);
int mi_groupnorm_fwd(const void* x, int ldx, int N, int HW, int C, int G, const float* gamma, const float* beta, float eps,
                     void* y, int ldy, float* mean_rstd, double* ws, mi_stream_t s);
int mi_groupnorm_bwd(const void* dy, int lddy, const void* x, int ldx, int N, int HW, int C, int G, const float* gamma,
                     const float* mean_rstd, void* dx, int lddx, float* dgamma, float* dbeta, double* ws, mi_stream_t s);
/* nn.MaxPool2d(2, 2) of ResampleFeatureMap (bifpn.py:151-155), floor mode; bwd recomputes the arg-max from x (first
 * maximum in row-major window order); with odd H / W the caller zero-fills dx first */
int mi_maxpool2x2_fwd(const void* x, int ldx, void* y, int ldy, int N, int H, int W, int C, mi_stream_t s);
int mi_maxpool2x2_bwd(const void* x, int ldx, const void* dy, int lddy, void* dx, int lddx, int N, int H, int W, int C,
                      mi_stream_t s);
/* FpnCombine "fastattn" (bifpn.py:221-236): out = sum_i x_i * relu(w_i) / (sum relu(w) + 1e-4) over nin = 2 or 3
 * contiguous bf16 tensors of n elements (n % 8 == 0); bwd: dx_i (dxs[i] may be NULL) and d edge_weights [nin]
 * (deterministic: per-block partials in ws, mi_fastattn_ws_bytes() bytes) */
int64_t mi_fastattn_ws_bytes(void);
int mi_fastattn_fwd(const void* const* xs, int nin, const float* edge_weights, void* out, int64_t n, mi_stream_t s);
int mi_fastattn_bwd(const void* const* xs, int nin, const float* edge_weights, const void* g, void* const* dxs, float* dedge,
                    float* ws, int64_t n, mi_stream_t s);

/* ---- input pipeline: mosaic + random_perspective + pad on the GPU ---------------
 * replaces, for a whole batch, the cv2.resize / canvas paste of MyDatasetMapper2.__call__ (data/dataset_mapper.py:523-598),
 * the cv2.warpAffine of random_perspective (data/transforms/data_augment.py:67-75) and the pad-to-batch with 114 of
 * YOLOX.preprocess_image (meta_arch/yolox.py:95-130).  uint8, OpenCV's fixed-point INTER_LINEAR arithmetic.
 * paste job: source image src [h0][w0][3] (HWC) resized to rw x rh; canvas[y1a:y2a, x1a:x2a] = resized[y1b.., x1b..]
 *            (canvas row pitch cw pixels, pre-filled with 114 by the caller).
 * warp job:  out[c][y][x] (planes of Hp x Wp bytes, y < h, x < w) = INTER_LINEAR sample of the ch x cw canvas at
 *            minv * (x, y, 1)  (minv: the INVERTED 2x3 matrix, row-major; taps outside the canvas read `border`).
 * mi_mosaic_jobs_layout validates both (host) tables and fills blk0; returns max(blocks of the paste launch, blocks of the
 * warp launch); the launches take the device copies of the tables and their own block counts. */
typedef struct mi_mosaic_paste_job {
  const void* src;
  void* canvas;
  int32_t h0, w0, rh, rw, cw, x1a, y1a, x2a, y2a, x1b, y1b, blk0;
  int32_t fsrc, pad_;        /* fsrc: the loaded image is float32 in the reference (YOLOFRandomDistortion ran): cv2.resize takes
                                its FLOAT path (float32 coefficients, products and sums) and the assignment into the uint8
                                canvas truncates (dataset_mapper.py:531-567) */
} mi_mosaic_paste_job;
typedef struct mi_warp_job {
  const void* canvas;
  void* out;
  double minv[6];
  int32_t ch, cw, h, w, Hp, Wp, border, blk0;
} mi_warp_job;
int mi_mosaic_jobs_layout(mi_mosaic_paste_job* paste_host, int npaste, mi_warp_job* warp_host, int nwarp);
int mi_mosaic_paste(const mi_mosaic_paste_job* jobs_dev, int njobs, int total_blocks, mi_stream_t s);
int mi_warp_affine_u8(const mi_warp_job* jobs_dev, int njobs, int total_blocks, mi_stream_t s);
/* MyDatasetMapper2.mixup (data/dataset_mapper.py:686-768) in place on a warped sample: out[c][y][x] (y < th, x < tw) =
 * uint8(0.5 * out + 0.5 * partner), partner = the pool image src [h0][w0][3] resized to rw1 x rh1 (8-bit fixed point) into
 * the corner of a 114.0 canvas dh x dw, that canvas resized to ow x oh (float64 path), optionally mirrored, zero-padded to the
 * target, cropped at (x_off, y_off), truncated to uint8.  mi_mixup_jobs_layout fills blk0 and returns the block count. */
typedef struct mi_mixup_job {
  const void* src;
  void* out;
  int32_t h0, w0, rh1, rw1, dh, dw, oh, ow, flip, x_off, y_off, th, tw, Hp, Wp, blk0;
  int32_t fsrc, pad_;        /* fsrc: the pool image is float32 in the reference: the FIRST resize takes cv2's float path and is
                                not rounded (dataset_mapper.py:706-711) */
} mi_mixup_job;
int mi_mixup_jobs_layout(mi_mixup_job* jobs_host, int njobs);
int mi_mixup_blend(const mi_mixup_job* jobs_dev, int njobs, int total_blocks, mi_stream_t s);

/* ---- the detectron2 T.* front of the reference's input pipeline --------------------------------------------------
 * build_normal_augmentation (yolov7/data/detection_utils.py:37-86) as MyDatasetMapper2._load_image_with_annos applies it
 * to every image it loads (yolov7/data/dataset_mapper.py:642-683): T.ResizeShortestEdge = PIL.Image.resize(BILINEAR) of
 * the uint8 image (Pillow libImaging/Resample.c: fp64 coefficients -> 22-bit fixed point, horizontal pass rounded to 8
 * bits, then the vertical pass), T.RandomFlip horizontal / vertical, YOLOFRandomShift (data/transforms/transform.py:341-388:
 * zeros where the shifted image does not reach).  One job per image: src HWC uint8 [h0][w0][3] (rows src_ld bytes apart, so a
 * T.RandomCrop window is an offset pointer; optionally mirrored first, as DetrDatasetMapper's flip-then-resize order needs,
 * data/dataset_mapper.py:777-800) -> nh x nw, element
 * (c, y, x) at dst + c dsc + y dsy + x dsx bytes (HWC: 1, 3 nw, 3; a sample of a padded NCHW batch: Hp Wp, Wp, 1);
 * tmp = [h0][nw][3] scratch of the horizontal pass (unused when nw == w0).  RandomSaturation / RandomBrightness (detectron2
 * BlendTransform, numpy's fp64 / fp32 arithmetic) and YOLOFRandomDistortion (OpenCV's 8-bit RGB2HSV_b / HSV2RGB_b, restated:
 * no cv2 here to pin them) are applied per pixel between the flips and the shift.
 * mi_pil_resize_jobs_layout validates the (host) table, fills blk0h / blk0v and returns the block counts of the two flat
 * launches; the launches take the device copy of the table.  Down-scaling factors up to 8. */
typedef struct mi_pil_resize_job {
  const void* src;
  void* tmp;
  void* dst;
  int64_t dsc, dsy, dsx;
  int64_t src_ld;            /* bytes between source rows (3 w0 for a whole image; the parent's for a crop window) */
  double sat_src;            /* RandomSaturation: 1 - w (fp64, the grey image's weight) */
  int32_t h0, w0, nh, nw;
  int32_t hflip, vflip, shift_x, shift_y;
  int32_t src_hflip;         /* mirror the source BEFORE the resampling (DetrDatasetMapper: T.RandomFlip, then the resizes) */
  int32_t color;             /* bit 0 RandomSaturation, bit 1 RandomBrightness (d2 BlendTransform on the uint8 image), bit 2
                                YOLOFRandomDistortion (data/transforms/transform.py:250-308: cv2's 8-bit RGB <-> HSV around
                                three float32 scalings); in that order, after the flips */
  float sat_dst, bri_dst;    /* w as float32 */
  float dis_hue, dis_sat, dis_exp;   /* float32(dhue * 179 / 255.), float32(dsat), float32(dexp) */
  int32_t dis_pos;           /* dhue > 0 */
  int32_t blk0h, blk0v;
} mi_pil_resize_job;
int mi_pil_resize_jobs_layout(mi_pil_resize_job* jobs_host, int njobs, int32_t* blocks_h, int32_t* blocks_v);
int mi_pil_resize_h(const mi_pil_resize_job* jobs_dev, int njobs, int total_blocks, mi_stream_t s);
int mi_pil_resize_v(const mi_pil_resize_job* jobs_dev, int njobs, int total_blocks, mi_stream_t s);

/* ---- image decoding of the input pipeline: baseline JPEG ---------------------------------------------------------
 * What detectron2's utils.read_image(file, format="BGR") does for MyDatasetMapper2._load_image_with_annos
 * (yolov7/data/dataset_mapper.py:646-648; d2 un-vendored): PIL.Image.open -> EXIF orientation -> convert("RGB") -> BGR,
 * i.e. Pillow's libjpeg(-turbo) defaults - sequential Huffman decoding (jdhuff.c), JDCT_ISLOW (jidctint.c), fancy
 * up-sampling (jdsample.c), YCbCr -> RGB (jdcolor.c).  Served: SOF0 / SOF1 sequential and SOF2 progressive Huffman files
 * (jdphuff.c; any scan script, tables redefined between scans), 8 bit, grey or three components, sampling factors 1 or 2
 * (4:4:4, 4:2:2, 4:2:0, 4:4:0), restart intervals, Adobe transform 0, EXIF orientations 1-8.  Refused with MI_EINVAL:
 * lossless / hierarchical / arithmetic-coded / 12-bit / CMYK files.
 * HOST functions (no GPU needed): mi_jpeg_parse reads the markers up to the first scan; mi_jpeg_huffman decodes every scan's
 * entropy-coded data into int16 coefficient blocks (natural order, not de-quantised; info->coef_count values, component c's blocks_h[c] x
 * blocks_w[c] blocks of 64 from coef_off[c]) - the caller copies them to the device; mi_jpeg_job_fill builds one image's
 * device job (planes: sum over components of blocks * 64 bytes of scratch; out: HWC uint8 [h][w][3], h and w swapped for
 * orientations 5-8 when apply_orientation); mi_jpeg_jobs_layout lays a batch out.  DEVICE: mi_jpeg_idct (one thread per
 * 8x8 block), then mi_jpeg_color (one thread per output pixel), over the device copy of the job table. */
typedef struct mi_jpeg_info {
  int32_t width, height, ncomp, restart_interval, orientation, adobe_transform;   /* adobe_transform -1: no Adobe marker */
  int32_t progressive, pad0_;
  int32_t comp_id[3], hs[3], vs[3], tq[3];
  int32_t hmax, vmax, mcu_w, mcu_h;
  int32_t blocks_w[3], blocks_h[3];
  int64_t coef_off[3], coef_count, sos_pos;   /* sos_pos: offset of the first SOS segment's length field */
  uint16_t qt[4][64];                  /* natural (row-major) order */
  uint8_t dc_bits[4][17], dc_vals[4][256], ac_bits[4][17], ac_vals[4][256];     /* the tables defined before the first scan */
  uint8_t have_qt[4], have_dc[4], have_ac[4], pad_[4];
} mi_jpeg_info;
typedef struct mi_jpeg_job {
  const int16_t* coef;
  void* planes;
  void* out;
  int64_t coef_off[3], plane_off[3];
  int32_t width, height, ncomp, orientation, bgr, ycc;
  int32_t hs[3], vs[3], blocks_w[3], blocks_h[3];
  int32_t hmax, vmax;
  int32_t blk0_idct, blk0_pix;
  uint16_t qt[3][64];
} mi_jpeg_job;
int mi_jpeg_parse(const uint8_t* data, int64_t len, mi_jpeg_info* info);
int mi_jpeg_huffman(const uint8_t* data, int64_t len, const mi_jpeg_info* info, int16_t* coef_host);
/* n files on `threads` host threads of the library; rcs[k] = file k's return code, the call returns the first non-zero one */
int mi_jpeg_huffman_batch(const uint8_t* const* datas, const int64_t* lens, const mi_jpeg_info* infos, int16_t* const* coefs_host,
                          int n, int threads, int32_t* rcs);
int mi_jpeg_job_fill(const mi_jpeg_info* info, const void* coef_dev, void* planes_dev, void* out_dev, int bgr,
                     int apply_orientation, mi_jpeg_job* job);
int mi_jpeg_jobs_layout(mi_jpeg_job* jobs_host, int njobs, int32_t* blocks_idct, int32_t* blocks_pix);
int mi_jpeg_idct(const mi_jpeg_job* jobs_dev, int njobs, int total_blocks, mi_stream_t s);
int mi_jpeg_color(const mi_jpeg_job* jobs_dev, int njobs, int total_blocks, mi_stream_t s);

/* ---- COCO run-length encoding of masks (evaluation output format) ----------------------
 * what pycocotools.mask.encode does for instances_to_coco_json (evaluation/coco_evaluation.py:38-50; the algorithm is
 * cocoapi's maskApi.c rleEncode / rleToString, un-vendored): masks uint8 [n][H][W] (device, non-zero = foreground) ->
 * counts[n][max_runs] = lengths of the alternating runs of the COLUMN-major scan, starting with a (possibly empty) run of
 * zeros; nruns[n] = number of runs, or -(needed runs) when max_runs is too small (that mask's counts are undefined).
 * mi_rle_to_string is host code: counts -> the compact ASCII "counts" string; returns its length (NUL-terminated). */
int mi_rle_encode(const uint8_t* masks, int n, int H, int W, int max_runs, uint32_t* counts, int32_t* nruns, mi_stream_t s);
int mi_rle_to_string(const uint32_t* counts, int nruns, char* out, int out_cap);

/* ---- COCO AP / AR evaluation (csrc/coco_eval.hip): cocoapi's COCOeval evaluate -> accumulate and maskApi.c's bbIou / rleIou /
 * rleDecode / rleFrString, un-vendored and restated; fp64 and integers in the originals' operation order (parity unpinned
 * against pycocotools itself; tests/cocoeval_ref.py is the restatement the kernels equal element for element).
 * mi_coco_box_iou: dt [D][4], gt [G][4] XYWH doubles, gcrowd [G] (may be NULL) -> iou [D][G]: 0 unless w > 0 and h > 0 of the
 *   intersection, else i / (crowd ? da : da + ga - i).
 * mi_coco_mask_iou: dense masks uint8 [D][H][W], [G][H][W] (non-zero = foreground), any H, W >= 1 -> inter [D][G], darea [D],
 *   garea [G] (pixel counts) and iou [D][G] = i / u with u = 1 if i == 0, else crowd ? da : da + ga - i.  ws: the bit-packed
 *   masks, mi_coco_mask_iou_ws_bytes(D, G, H, W) bytes, 8-byte aligned.
 * mi_rle_decode: counts [n][max_runs], nruns [n] (device; run lengths of the COLUMN-major scan, first a run of zeros) ->
 *   out [n][H][W] row-major 0 / 1.  cum_ws: [n][max_runs] scratch.  err [n] (device) is set to 1 for a mask whose counts do
 *   not sum to H * W (or whose nruns is outside [0, max_runs]); that mask is written as zeros.  wait != 0: the call waits
 *   for the stream, reads err and returns MI_EINVAL for such a mask - the only waiting form; wait == 0 never synchronises.
 * mi_rle_from_string: host code, the inverse of mi_rle_to_string: NUL-terminated string -> counts; returns the number of
 *   runs, MI_EINVAL when max_runs is too small.
 * mi_coco_match: evaluateImg for every (cell = image * K + category, area range); lane = IoU threshold (T <= 64).
 *   Detections sorted by (cell, -score, stable): det_row [N] (offset of the detection's row in iou), det_area [N], det_start
 *   [ncell + 1]; the first max_det of a cell enter.  Ground truths sorted by (cell, annotation order): gt_start [ncell + 1],
 *   gt_col [Gt] (column in the row), gt_area [Gt], gt_crowd [Gt].  area_rng [A][2], bounds inclusive.  Writes dtm / dtig
 *   [A][T][N] (matched / ignored; zero for detections that did not enter), gtig [A][Gt], npig [ncell][A] (ground truths
 *   not ignored); gtm [A][T][Gt] is scratch.
 * mi_coco_accumulate: detections sorted by (category, -score, stable over ascending image, rank): dtm / dtig [A][T][N], score
 *   [N], rank [N] (place in the image's score order; rank < max_dets[m] enters), cat_start [K + 1], npig [K][A] -> precision
 *   and scores [T][R][K][A][M], recall [T][K][A][M]; -1 where npig == 0. */
int mi_coco_box_iou(const double* dt, int D, const double* gt, int G, const uint8_t* gcrowd, double* iou, mi_stream_t s);
int64_t mi_coco_mask_iou_ws_bytes(int D, int G, int H, int W);
int mi_coco_mask_iou(const uint8_t* dmasks, int D, const uint8_t* gmasks, int G, int H, int W, const uint8_t* gcrowd, void* ws,
                     int64_t ws_bytes, int64_t* inter, int64_t* darea, int64_t* garea, double* iou, mi_stream_t s);
int mi_rle_decode(const uint32_t* counts, const int32_t* nruns, int n, int max_runs, int H, int W, uint32_t* cum_ws, uint8_t* out,
                  int32_t* err, int wait, mi_stream_t s);
int mi_rle_from_string(const char* s, uint32_t* counts, int max_runs);
int mi_coco_match(const double* iou, const int64_t* det_row, const double* det_area, const int64_t* det_start,
                  const int64_t* gt_start, const int32_t* gt_col, const double* gt_area, const uint8_t* gt_crowd,
                  const double* iou_thrs, int T, const double* area_rng, int A, int max_det, int64_t ncell, int64_t N, int64_t Gt,
                  uint8_t* dtm, uint8_t* dtig, uint8_t* gtig, uint8_t* gtm, int32_t* npig, mi_stream_t s);
int mi_coco_accumulate(const uint8_t* dtm, const uint8_t* dtig, const double* score, const int32_t* rank, const int64_t* cat_start,
                       const int64_t* npig, const int32_t* max_dets, const double* rec_thrs, int T, int R, int K, int A, int M,
                       int64_t N, double* precision, double* recall, double* scores, mi_stream_t s);

/* ---- batched NMS -------------------------------------------------------------
 * replaces torchvision.ops.batched_nms as called by postprocess (utils/boxes.py:199).
 * boxes xyxy fp32 [n][4], scores [n], idxs (class id as float, as the reference passes) [n].
 * keep[n] receives the kept indices in descending score order, *n_keep their count.
 * workspaces: order int32[n], mask uint64[n*ceil(n/64)], sboxes float[5*n+1]. */
int mi_batched_nms(const float* boxes, const float* scores, const float* idxs, int n, float iou_thr,
                   int32_t* order, uint64_t* mask, float* sboxes, int64_t* keep, int32_t* n_keep,
                   mi_stream_t s);
/* the same with the IoU arithmetic chosen by the caller: -1 torchvision's choice by size, 0 class by class on the raw
 * coordinates, 1 the per-class coordinate offsets.  0 is also what batched_clusternms (meta_arch/utils.py:66-95) computes:
 * its fixed-point iteration over the IoU matrix converges to the greedy result. */
int mi_batched_nms_ex(const float* boxes, const float* scores, const float* idxs, int n, float iou_thr, int arithmetic,
                      int32_t* order, uint64_t* mask, float* sboxes, int64_t* keep, int32_t* n_keep, mi_stream_t s);
/* YOLOX eval postprocess (utils/boxes.py:171-210) for a whole batch in one fixed launch sequence, with no host sync, no
 * allocation and no memset (graph-capturable).  pred [B][A][ld] fp32 decoded (cx,cy,w,h,obj,cls[C],...), ld >= 5 + C: its
 * first four columns are rewritten IN PLACE to x1,y1,x2,y2 (the reference's side effect).  Per image: anchors with
 * obj * max(cls) >= conf_thr are the candidates (ascending anchor order), NMS as mi_batched_nms (its arithmetic chosen per
 * image by the image's candidate count), and the kept rows (x1,y1,x2,y2,obj,cls_conf,cls_idx) go to dets[b][0 .. counts[b])
 * of dets [B][A][7] in descending score order; rows past counts[b] are left as they were.  B <= 1024 per call,
 * 1 <= A <= 65536, C >= 1.  ws: >= mi_yolox_postprocess_ws_bytes(B, A, C) bytes, 8-byte aligned; the size is the worst
 * case, every anchor a candidate:
 *   B * (8 * A * ceil(A / 64) + 72 * A + 4 * ceil(A / 256) + 8)
 * where the first term is the suppression bitmask: ~142 MB at B = 16, A = 8400 and ~318 MB at B = 16, A = 12600.
 * _ws_bytes returns a negative MI_E* code for arguments outside those limits. */
int64_t mi_yolox_postprocess_ws_bytes(int B, int A, int C);
int mi_yolox_postprocess(float* pred, int B, int A, int C, int ld, float conf_thr, float nms_thr, float* dets,
                         int32_t* counts, void* ws, int64_t ws_bytes, mi_stream_t s);
/* class-aware Soft-NMS (batched_softnms, meta_arch/utils.py:33-63): scores are rescaled IN PLACE, keep[] receives the
 * indices with score > score_threshold in descending score order (ties: ascending index).  sigma is the reference's
 * iou_threshold argument; linear 0 = "gaussian" exp(-iou^2 / sigma), 1 = "linear".  n <= 16384. */
int mi_batched_softnms(const float* boxes, float* scores, const float* idxs, int n, float sigma, float score_threshold,
                       int linear, int64_t* keep, int32_t* n_keep, mi_stream_t s);
/* Matrix NMS (utils/solov2_utils.py:160-206) from the mask-intersection matrix inter[n][n] = masks @ masks^T
 * (candidates in descending score order), sum_masks[n], labels[n] (as float): out_scores[n] = scores * decay.
 * comp_ws: n floats of scratch. */
/* greedy mask NMS (utils/solov2_utils.py:209-236) on the same intersection matrix: keep[n] (1 = kept) */
int mi_mask_nms(const float* inter, const float* sum_masks, const float* labels, int n, float nms_thr, uint8_t* keep,
                mi_stream_t s);
int mi_matrix_nms(const float* inter, const float* sum_masks, const float* labels, const float* scores, int n, float sigma,
                  int linear, float* comp_ws, float* out_scores, mi_stream_t s);

/* ---- fused SGD(momentum, weight-decay) over a flat parameter arena -----------
 * replaces torch.optim.SGD.step as built by detectron2's build_optimizer
 * (train_det.py:73 -> DefaultTrainer). seg table: per segment (offset,count,wd,lr) */
typedef struct mi_sgd_seg {
  int64_t offset, count;
  float weight_decay, lr;
} mi_sgd_seg;
int mi_sgd_momentum_step(float* params, const float* grads, float* momentum_buf,
                         const mi_sgd_seg* segs_dev, int nseg, float momentum, float grad_scale,
                         int first_step, mi_stream_t s);

/* fp32 sigmoid of the DETR box head (meta_arch/detr.py:452): forward (x -> y; dy = dx = NULL) or backward
 * (dx = dy * y * (1 - y); x may be NULL) */
int mi_sigmoid_f32(const float* x, const float* dy, float* y, float* dx, int64_t n, mi_stream_t s);
/* fused AdamW (decoupled weight decay, bias-corrected moments) over the flat arena: replaces torch.optim.AdamW.step of
 * the DETR / SparseInst trainers (train_transformer.py, train_inseg.py -> optimizer/build.py); `step` is the 1-based
 * update count, seg table as for SGD */
int mi_adamw_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, const mi_sgd_seg* segs_dev,
                  int nseg, float beta1, float beta2, float eps, int64_t step, float grad_scale, mi_stream_t s);
/* the same update over SEPARATELY ALLOCATED tensors (an eager nn.Module tree: no flat arena) in one launch.  tensors_dev:
 * device table of (param, grad, exp_avg, exp_avg_sq, count, lr, weight_decay); chunks_dev: device table of (tensor index,
 * element offset, count <= 16384), one block each; step_dev: device int64 holding the 1-based update count of THIS step
 * (the caller advances it).  Everything the kernel dereferences is read at run time, so a captured hipGraph stays valid
 * when the tables are refilled (gradient addresses are only known once the capture has ended). */
typedef struct mi_adamw_tensor {
  float* p; const float* g; float* m; float* v;
  int64_t count;
  float lr, weight_decay;
} mi_adamw_tensor;
typedef struct mi_adamw_chunk {
  int32_t tensor, count;
  int64_t offset;
} mi_adamw_chunk;
int mi_adamw_step_multi(const mi_adamw_tensor* tensors_dev, const mi_adamw_chunk* chunks_dev, int nchunks, float beta1,
                        float beta2, float eps, const int64_t* step_dev, float grad_scale, mi_stream_t s);
/* FullModelGradientClippingOptimizer.step (yolov7/optimizer/build.py:206-223: clip_grad_norm_ over all parameters, then
 * the update) over the same tables without touching the host: mi_grad_norm_multi leaves coef_norm_out[0] = min(1, max_norm
 * / (||g||_2 + 1e-6)) and [1] = the norm on the device (partial_dev: nchunks doubles of scratch, summed in index order);
 * (of the gradients times grad_scale); mi_adamw_step_multi_clip multiplies every gradient by grad_scale * *grad_scale_dev
 * (NULL: grad_scale alone) */
int mi_grad_norm_multi(const mi_adamw_tensor* tensors_dev, const mi_adamw_chunk* chunks_dev, int nchunks,
                       double* partial_dev, float max_norm, float grad_scale, float* coef_norm_out, mi_stream_t s);
/* data-parallel form of the captured step (train_transformer.py:188-203 / train_inseg.py:63-77 -> d2 create_ddp_model): the
 * gradients of every tensor copied into ONE flat fp32 buffer (tensor k at element offset flat_off_dev[k]) in one launch -
 * the buffer is all-reduced in a few large messages and the update reads it (a table whose g fields point into it) with
 * grad_scale = 1 / world_size; mi_grad_norm_multi's grad_scale makes the clipped norm the AVERAGED gradient's */
int mi_grad_gather_multi(const mi_adamw_tensor* tensors_dev, const mi_adamw_chunk* chunks_dev, int nchunks,
                         const int64_t* flat_off_dev, float* flat, mi_stream_t s);
int mi_adamw_step_multi_clip(const mi_adamw_tensor* tensors_dev, const mi_adamw_chunk* chunks_dev, int nchunks, float beta1,
                             float beta2, float eps, const int64_t* step_dev, float grad_scale,
                             const float* grad_scale_dev, mi_stream_t s);
/* full-model gradient clipping (FullModelGradientClippingOptimizer, yolov7/optimizer/build.py:206-223 =
 * torch.nn.utils.clip_grad_norm_ over all parameters): grads *= min(1, max_norm / (||grads||_2 + 1e-6)) without a host
 * synchronisation; ws: 1024 doubles of scratch; norm_out (optional, device) receives the norm */
int mi_grad_clip_full_model(float* grads, int64_t n, float max_norm, double* ws, float* norm_out, mi_stream_t s);
/* PositionEmbeddingSine.forward (modeling/backbone/detr_backbone.py:309-375): mask [B][H][W] bytes (non-zero = padding)
 * -> pos fp32 [B][2*num_pos_feats][H][W] */
int mi_pos_embed_sine(const uint8_t* mask, int B, int H, int W, int num_pos_feats, float temperature, int normalize,
                      float scale, int centered, float* out, mi_stream_t s);

/* ---- SparseInst (config 5): bilinear resize (align_corners False) of bf16 NHWC maps and the mask losses of the matched
 * (prediction, target) pairs of SparseInstCriterion (loss/sparseinst_loss.py:123-187).  See csrc/sparseinst_ops.hip. */
int mi_bilinear_resize_bf16(const void* x, int ldx, int N, int H, int W, int C, void* y, int ldy, int Ho, int Wo,
                            mi_stream_t s);
/* (the backward gathers in a fixed order: no workspace; the float* argument is ignored and may be NULL) */
int mi_bilinear_resize_bwd_bf16(const void* dy, int lddy, int N, int H, int W, int C, void* dx, int lddx, int Ho, int Wo,
                                float* acc_ws_zeroed, mi_stream_t s);
/* PyramidPoolingModule's pooling stages (transcoders/encoder_sparseinst.py:18-62: F.avg_pool2d(x, kernel = (kh, kw), stride =
 * kernel, ceil_mode=False) per stage) of one bf16 NHWC map x [N][H][W][C] (ldx) in ONE launch: y[s] bf16 [N][H / kh[s]][W / kw[s]][C]
 * dense; and the backward: dx = sum over the stages of dy[s] spread over its windows / (kh kw) (dy[s] NULL: no gradient).
 * kh / kw / y / dy are HOST arrays of ns <= MI_PYR_MAX_STAGES entries. */
#define MI_PYR_MAX_STAGES 8
int mi_pyramid_pool_fwd(const void* x, int ldx, int N, int H, int W, int C, int ns, const int* kh, const int* kw, void* const* y,
                        mi_stream_t s);
int mi_pyramid_pool_bwd(void* const* dy, int N, int H, int W, int C, int ns, const int* kh, const int* kw, void* dx, int lddx,
                        mi_stream_t s);
/* masks bf16 logits [B][P][ldm] (instance = channel), targets fp32 [T][P], pairs int32 [K][3] = (b, n, t);
 * stats fp32 [K][8] = sum BCE, sum sig*t, sum sig^2, sum t^2, |sig>=.4 & t>.5|, |sig>=.4|, |t>.5|, 0 (rows with b < 0: zeros).
 * ws: mi_sparseinst_mask_stats_ws_floats(K, P) floats of block partials, summed in a fixed order (bit-reproducible; no
 * float atomics) */
int64_t mi_sparseinst_mask_stats_ws_floats(int K, int P);
int mi_sparseinst_mask_stats(const void* masks, int ldm, int P, const float* targets, const int32_t* pairs, int K,
                             float* stats, float* ws, mi_stream_t s);
int mi_sparseinst_mask_grad(const void* masks, int ldm, int P, const float* targets, const int32_t* pairs, int K,
                            const float* stats, float c_bce, float c_dice, void* dmasks_zeroed, mi_stream_t s);
/* the form a captured step uses: pair rows whose image index is < 0 are skipped by both kernels (a fixed-capacity pair table
 * filled by the device-side matching), and the two upstream gradients come from the device (coef_dev[0], coef_dev[1]) */
int mi_sparseinst_mask_grad_dev(const void* masks, int ldm, int P, const float* targets, const int32_t* pairs, int K,
                                const float* stats, const float* coef_dev, void* dmasks, mi_stream_t s);

/* SparseInstCriterion's scalar half and SparseInstMatcher's cost matrix (csrc/sparseinst_loss.hip; loss/sparseinst_loss.py:
 * 190-297, 300-354) - four launches for what the reference spells as ~150 small torch calls.
 * mi_sparseinst_match_cost: cost[b][n][t] = -(dice^alpha * prob^beta), dice = 2 num[b][n][t] / (s2[b][n] + t2[b][t] + 1e-4),
 *   prob = sigmoid(logits[b][n][labels[b][t]]); num fp32 [B][Np][cap], s2 [B][Np], t2 [B][cap], logits fp32 [B][N][C],
 *   labels int64 [B][cap] -> cost fp32 [B][N][cap].
 * The three criterion calls share one descriptor (all device pointers; fixed capacity `cap` pairs per image):
 *   _pairs:        match_q / match_t int64 [B][cap], nmatch int32 [B] (mi_lsap), labels -> pairs int32 [B*cap][3] = (b or -1, q,
 *                  b*cap+t), valid fp32 [B*cap], row_cls / row_pair int32 [B][N] (class / pair of the query's match or -1),
 *                  kdev[0] = max(sum nmatch, 1)
 *   _head_loss:    logits, scores fp32 [B][N] (objectness logits), stats fp32 [B*cap][8] (mi_sparseinst_mask_stats), inv_num[0]
 *                  -> losses[4] = weighted loss_ce, loss_mask, loss_dice, loss_objectness
 *   _head_loss_bwd: gup[4] upstream gradients -> dlogits [B][N][C], dscores [B][N], coef[2] (mi_sparseinst_mask_grad_dev's) */
typedef struct mi_sparseinst_loss_desc {
  const float* logits;
  const float* scores;
  const int64_t* labels;
  const int64_t* match_q;
  const int64_t* match_t;
  const int32_t* nmatch;
  const float* inv_num;
  const float* stats;
  const float* gup;
  int32_t* pairs;
  float* valid;
  int32_t* row_cls;
  int32_t* row_pair;
  float* kdev;
  float* losses;
  float* dlogits;
  float* dscores;
  float* coef;
  int B, N, C, cap, P, use_labels, use_masks, pad_;
  float alpha, gamma, w_ce, w_mask, w_dice, w_obj;
} mi_sparseinst_loss_desc;
int mi_sparseinst_match_cost(const float* num, const float* s2, const float* t2, const float* logits, const int64_t* labels,
                             int B, int N, int Np, int C, int cap, float alpha, float beta, float* cost, mi_stream_t s);
int mi_sparseinst_pairs(const mi_sparseinst_loss_desc* d, mi_stream_t s);
int mi_sparseinst_head_loss(const mi_sparseinst_loss_desc* d, mi_stream_t s);
int mi_sparseinst_head_loss_bwd(const mi_sparseinst_loss_desc* d, mi_stream_t s);

/* ---- box utilities of the DETR path (yolov7/utils/boxes.py:28-37,85-122) ------------------------------------------
 * mi_box_convert: n boxes [n][4] fp32; to_cxcywh 0 = box_cxcywh_to_xyxy, 1 = box_xyxy_to_cxcywh.
 * mi_box_iou_pairwise: box_iou (iou and union, [n][m]) and, when giou != NULL, generalized_box_iou of xyxy boxes in the
 * reference's operation order; *degenerate (may be NULL, caller zeroes it) gets bit 0 / 1 set when a box of the first /
 * second set has x1 < x0 or y1 < y0 - the condition generalized_box_iou asserts on. */
int mi_box_convert(const float* in, float* out, int64_t n, int to_cxcywh, mi_stream_t s);
int mi_box_iou_pairwise(const float* boxes1, int n, const float* boxes2, int m, float* iou, float* uni, float* giou,
                        int32_t* degenerate, mi_stream_t s);

/* sizeof() of the public structs as compiled into the library (binding self-check): 0 mi_conv_desc, 1 mi_wgrad_desc,
 * 2 mi_wgrad_group, 3 mi_pack_job, 4 mi_bias_job, 5 mi_yolox_loss_desc, 6 mi_detr_loss_desc, 7 mi_sgd_seg, 8 mi_cmd,
 * 9 mi_conv_group, 10 mi_bn_job, 11 mi_bn_group, 12 mi_pil_resize_job, 13 mi_jpeg_info, 14 mi_jpeg_job; -1 for an unknown id */
int mi_abi_sizeof(int which);

/* ---- command list executor -----------------------------------------------------
 * A step (forward / backward / update) is a flat list of mi_cmd records built once
 * by the host; mi_cmdlist_run() issues them back-to-back on one stream from C++
 * (no per-launch Python), and mi_graph_* capture/replay the same list as a hipGraph. */
typedef struct mi_cmd {
  int32_t op;          /* MI_OP_* */
  int32_t i[40];
  float f[8];
  void* p[16];
  int64_t l[4];
} mi_cmd;

enum {
  MI_OP_NOP = 0,
  MI_OP_CONV = 1,
  MI_OP_WGRAD = 2,
  MI_OP_PACK_W = 3,
  MI_OP_RESERVED4 = 4, /* was UNPACK_WG: wgrad now writes OIHW directly */
  MI_OP_RESERVED5 = 5, /* was BN_FINALIZE: folded into BN_ACT_FWD */
  MI_OP_BN_ACT_FWD = 6,
  MI_OP_BN_BWD_REDUCE = 7,
  MI_OP_RESERVED8 = 8, /* was BN_BWD_FINALIZE: folded into BN_BWD_APPLY */
  MI_OP_BN_BWD_APPLY = 9,
  MI_OP_FOCUS = 10,
  MI_OP_UPSAMPLE_FWD = 11,
  MI_OP_UPSAMPLE_BWD = 12,
  MI_OP_SPP_FWD = 13,
  MI_OP_SPP_BWD = 14,
  MI_OP_COPY = 15,
  MI_OP_COLSUM = 16,
  MI_OP_LOSS_FWD = 17,
  MI_OP_LOSS_BWD = 18,
  MI_OP_SPLIT_DPREDS = 19,
  MI_OP_MEMSET = 20,
  MI_OP_SGD = 21,
  MI_OP_BN_EVAL_AFFINE = 22,
  MI_OP_DECODE = 23,
  MI_OP_PACK_W_BATCH = 24,
  MI_OP_WGRAD_GROUP = 25,
  MI_OP_RESERVED26 = 26, /* was STREAM: every command runs on the caller's stream */
  MI_OP_RESERVED27 = 27, /* was FORK */
  MI_OP_RESERVED28 = 28, /* was JOIN */
  MI_OP_BIAS_GRADS = 29,
  MI_OP_CONV_GROUP = 30,   /* p0 = mi_conv_group* (host), p1 = device job table */
  MI_OP_BN_GROUP = 31,     /* p0 = mi_bn_group* (host),   p1 = device job table */
  MI_OP_SPLIT_DPREDS_BATCH = 32, /* p0 = mi_split_job* (host), p1 = dpreds, i = B, A, nch, njobs */
  MI_OP_BN_BWD_FUSED = 33, /* BN_BWD_APPLY's arguments + p[12] = barrier words */
  /* depthwise 3x3: i = ldx/lddy, ldy/lddx, N, H, W, C, stride, outH, outW, nslots/accumulate */
  MI_OP_DWCONV_FWD = 34,   /* p = x, w, y, stats_acc */
  MI_OP_DWCONV_DGRAD = 35, /* p = dy, w, dx */
  MI_OP_DWCONV_WGRAD = 36, /* p = x, dy, ws, dw; l0 = ws bytes */
  MI_OP_LOSS_BWD_FUSED = 37, /* p = loss desc, gw, dpreds, split jobs (host), bias jobs (host), ws; i = nsplit, nbias; l0 = ws floats */
  MI_OP_COUNT
};

int mi_cmdlist_run(const mi_cmd* cmds, int n, mi_stream_t s);
/* returns an opaque handle (>0) or <0 */
int64_t mi_graph_capture(const mi_cmd* cmds, int n, mi_stream_t s);
int mi_graph_launch(int64_t handle, mi_stream_t s);
int mi_graph_destroy(int64_t handle);

/* time one command list with HIP events on stream s: runs it `iters` times, returns avg ms in *ms;
 * if per_cmd_ms != NULL (n floats) each command is additionally timed alone (event pair per cmd). */
int mi_cmdlist_time(const mi_cmd* cmds, int n, int iters, float* ms, float* per_cmd_ms, mi_stream_t s);

/* ---- the batch-building half of the DETR / SparseInst steps (csrc/host_feed.hip): one launch per batch where the reference
 * runs a handful of torch calls per image.  The per-image records are passed BY VALUE inside the kernel arguments (`jobs` is
 * a HOST array; nothing is uploaded, nothing has to stay alive), MI_FEED_MAX_IMAGES images per launch.
 *
 * mi_normalize_pad_batch: yolov7/modeling/meta_arch/detr.py:273-278 and meta_arch/sparseinst.py:95-98 -
 *   dst[b][c][y][x] = (img_b[c][y][x] - mean[c]) / std[c] for y < h_b, x < w_b, else 0; dst fp32 [B][3][Hp][Wp] (16-byte
 *   stores when Wp % 4 == 0 and dst is 16-byte aligned), images CHW dense on the device, dtype 0 = fp32, 1 = uint8.
 * mi_mask_targets_batch: yolov7/utils/misc.py:148-170 (nested_masks_from_list) + yolov7/modeling/loss/sparseinst_loss.py:
 *   149-151, 326-328 (F.interpolate bilinear, align_corners=False) - image b's M_b masks [M_b][h_b][w_b] (fp32, or 1-byte
 *   bool / uint8 read as 0 / 1) zero-extended to (Hi, Wi), resized to (Ho, Wo), written as fp32 rows tgt[(b * cap + j)][Ho * Wo]
 *   (rows j >= M_b zero), as their bf16 transpose tgtT[b][Ho * Wo][cap] (NULL: skipped) and labels[b][cap] (int64, 0 beyond
 *   M_b; NULL: skipped; a job's `labels` may be NULL when M == 0).  cap % 8 == 0, 64 * cap * 2 bytes of LDS.
 *   t2 (NULL: skipped): fp32 [B][cap] = sum over the pixels of tgt^2 per row, summed in a fixed order through t2_ws
 *   (B * cap * ceil(Ho * Wo / 64) floats): wave sums of 64 pixels, then the chunks in sequence (a second small launch). */
#define MI_FEED_MAX_IMAGES 32
#define MI_FEED_MAX_LEVELS 8
typedef struct mi_image_job {
  const void* src;
  int h, w, dtype, pad_;
} mi_image_job;
typedef struct mi_mask_job {
  const void* masks;
  const int64_t* labels;
  int M, h, w, dtype;
} mi_mask_job;
int mi_normalize_pad_batch(const mi_image_job* jobs, int B, float* dst, int Hp, int Wp, const float* mean3, const float* std3,
                           mi_stream_t s);
/* mi_padding_masks: MaskedBackbone.mask_out_padding (yolov7/modeling/meta_arch/detr.py:385-403) for all feature levels in one
 *   launch, from the device copy of the image sizes (int64 [B][2] = (h, w)): out[l] uint8 / bool [B][H[l]][W[l]] = 0 where
 *   y < ceil(h / stride[l]) and x < ceil(w / stride[l]), else 1.  out / H / W / stride are HOST arrays of nlev entries. */
int mi_padding_masks(const int64_t* sizes_dev, int B, int nlev, void* const* out, const int* H, const int* W, const int* stride,
                     mi_stream_t s);
int mi_mask_targets_batch(const mi_mask_job* jobs, int B, int cap, int Hi, int Wi, int Ho, int Wo, float* tgt, void* tgtT_bf16,
                          int64_t* labels, float* t2, float* t2_ws, mi_stream_t s);

/* mi_polygon_masks: the polygon ground truth of a batch rasterised on the device (csrc/polygon_masks.hip) - per image the
 *   masks BitMasks.from_polygon_masks(polygons, h, w) gives (yolov7/modeling/meta_arch/sparseinst.py:111-115; pycocotools'
 *   rleFrPoly per ring, the union of an instance's rings), bit for bit: out uint8 [M][h][w] row-major, 0 / 1, written
 *   completely.  verts: the image's rings one after the other as fp64 x0, y0, x1, y1, ...; ring_off: int32 [rings + 1], the
 *   first VERTEX of every ring; inst_off: int32 [M + 1], the first RING of every instance - all three on the device, and the
 *   two offset tables once more in host memory (`*_host`: the argument checks read these; the caller keeps both copies
 *   equal).  Refused: a ring of fewer than 3 vertices, an instance without a ring, h > MI_POLY_MAX_H (a block keeps
 *   2 x 64 columns x (h + 1) bits in LDS), null pointers where M > 0.  One launch per MI_FEED_MAX_IMAGES images, no
 *   workspace, deterministic. */
#define MI_POLY_MAX_H 3807
typedef struct mi_poly_job {
  const double* verts;
  const int32_t* ring_off;
  const int32_t* inst_off;
  const int32_t* ring_off_host;
  const int32_t* inst_off_host;
  void* out;
  int M, h, w, pad_;
} mi_poly_job;
int mi_polygon_masks(const mi_poly_job* jobs, int B, mi_stream_t s);

/* ---- SparseInst inference postprocess for a whole batch (csrc/sparseinst_infer.hip): what SparseInst.inference
 * (yolov7/modeling/meta_arch/sparseinst.py:169-234 + rescoring_mask :24-27) computes in a per-image loop of torch ops, in three
 * launches and one host read-back (the counts).  No fp32 mask intermediate is written to memory.
 *
 * The mask logits are read IN PLACE: `masks` + element strides (sb, sq, sy, sx) for (image, query, row, column), all >= 1
 * (sb >= 0), mask_dtype 0 = fp32, 1 = bf16 - the decoder's NHWC bf16 tensor [B][h][w][Np] is (h * w * Np, 1, w * Np, Np), a dense
 * fp32 [B][N][h][w] is (N * h * w, h * w, w, 1).  Only queries 0 .. N - 1 are read.
 *
 * mi_sparseinst_infer_select: for every (b, q)
 *     score = max_c sqrt(sigmoid(logits[b][q][c]) * sigmoid(obj[b][q])), label = the FIRST maximum (torch.max), keep = score > cls_thr;
 *   the kept queries of an image are compacted in ascending q (the order of boolean-mask indexing), and each is rescored over
 *   the whole h x w prediction, padding included: m = sigmoid(float(mask)),
 *     score *= sum(m * (m > mask_thr)) / (sum(m > mask_thr) + 1e-6)            (fp32 sums in a fixed order: deterministic).
 *   logits fp32 [B][N][C], obj fp32 [B][N], both dense.  Outputs: counts int32 [B]; kept_query int32 [B][N], scores fp32 [B][N],
 *   labels int64 [B][N] - the first counts[b] entries of row b, the rest is left as it was.  ws: mi_sparseinst_infer_ws_bytes(B,
 *   N, h, w) = B * ceil(h * w / 256) * 2 * N * 4 bytes (the per-chunk partial sums), 4-byte aligned.  Two launches, no host sync.
 * mi_sparseinst_infer_masks: for image b and its j-th kept query q = kept_query[b][j], j < descs[b].n, every pixel (oy, ox) of
 *   out[descs[b].out_off + (j * Hout + oy) * Wout + ox] = value > mask_thr ? 1 : 0   (one byte), value being the composition
 *     bilinear (h, w) -> (Hpad, Wpad), crop to (h_img, w_img), bilinear -> (Hout, Wout)   of sigmoid(mask), in fp32,
 *   with ATen's align_corners=False arithmetic on both levels: scale = float(in) / float(out), src = max(0, scale * (dst + 0.5)
 *   - 0.5), i0 = min(int(src), in - 1), i1 = min(i0 + 1, in - 1), l = src - int(src), value = (1 - ly) * ((1 - lx) * a + lx * b) +
 *   ly * ((1 - lx) * c + lx * d).  The outer level's `in` is the cropped size (h_img, w_img), so its indices never leave the
 *   crop; each of its 2 x 2 samples is the inner level's 2 x 2 interpolation (in = (h, w), out = (Hpad, Wpad)), a complete fp32
 *   value before the outer level uses it.  `descs` is a HOST array of B records, passed on by value (MI_FEED_MAX_IMAGES images
 *   per launch); an image with n == 0 writes nothing.  sigmoid is evaluated once per source pixel of a block's tile and kept
 *   in LDS; an image whose total down-scale makes a tile's source rectangle exceed that stage reads its taps from memory.
 * Refused before any launch (-1, mi_last_error): null pointers; B < 0; N, C, h or w < 1; Hpad or Wpad < 1; a mask dtype other
 *   than 0 / 1 or a stride < 1; a descriptor with n outside 0 .. N, or - where n > 0 - Hout or Wout < 1, h_img or w_img < 1 or
 *   beyond (Hpad, Wpad), or n * Hout * Wout bytes at out_off not inside out_bytes; a workspace smaller than the size query.
 *   B == 0 returns 0 without a launch. */
typedef struct mi_sparseinst_infer_desc {
  int64_t out_off;                    /* byte offset of the image's [n][Hout][Wout] block in `out` */
  int32_t n, h_img, w_img, Hout, Wout, pad_;
} mi_sparseinst_infer_desc;
int64_t mi_sparseinst_infer_ws_bytes(int B, int N, int h, int w);          /* -1: B < 0 or N, h, w < 1 */
int mi_sparseinst_infer_select(const float* logits, const float* obj, const void* masks, int mask_dtype, int64_t sb, int64_t sq,
                               int64_t sy, int64_t sx, int B, int N, int C, int h, int w, float cls_thr, float mask_thr,
                               int* counts, int* kept_query, float* scores, int64_t* labels, void* ws, int64_t ws_bytes,
                               mi_stream_t s);
int mi_sparseinst_infer_masks(const void* masks, int mask_dtype, int64_t sb, int64_t sq, int64_t sy, int64_t sx, int B, int N,
                              int h, int w, int Hpad, int Wpad, const int* kept_query, const mi_sparseinst_infer_desc* descs,
                              float mask_thr, void* out, int64_t out_bytes, mi_stream_t s);

/* ---- hardware probes used by tests (lane layouts of MFMA / LDS transpose read) */
int mi_probe_mfma32(const void* a_bf16_32x16, const void* b_bf16_16x32, float* d_32x32, mi_stream_t s);
int mi_probe_mfma16(const void* a_bf16_16x32, const void* b_bf16_32x16, float* d_16x16, mi_stream_t s);

#ifdef __cplusplus
}
#endif
#endif /* MI355_DET_H */
