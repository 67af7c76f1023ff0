"""Row-column decoupled attention of Anchor DETR on the MI355X kernels - drop-in for the reference's `MultiheadRCDA`
(yolov7/modeling/backbone/layers/row_column_decoupled_attention.py): same constructor, parameters, state_dict keys,
initialisation and forward signature.

    Qr = lin0(query_row)  Qc = lin1(query_col)                                  [B, L, E]
    Kr = lin2(mean over H of key_row)   Kc = lin3(mean over W of key_col)       [B, W, E] / [B, H, E]
    V  = lin4(value)                                                            [B, H, W, E]
    O  = rcda_core(Qr, Qc, Kr, Kc, V, mask[:, 0, :], mask[:, :, 0])             [B, L, E]   (csrc/rcda.hip, scale = hd^-0.5 inside)
    out = out_proj(O) as (L, B, E)

Two things differ from the reference's arithmetic, both stated in DESIGN.md 3.14: the key means are taken BEFORE the
projections (a mean commutes with an affine map: only the order of roundings changes, and H (W) times fewer rows are
projected), and a query whose row or column keys are all padded gives 0 and no gradient instead of NaN.
The five projections and out_proj run on the token-row GEMM path of modeling/transformer.py; in_proj_weight / in_proj_bias
receive their gradients as whole tensors (one autograd node over all five row blocks).
"""
import ctypes as C

import torch
from torch import nn

from .. import _lib as L
from .transformer import _LinearFn, _can_defer, _linear_bwd, _linear_fwd

HEAD_DIM = 32
MAX_SIDE = 96


def _desc(q_row, q_col, k_row, k_col, v, mask_row, mask_col, num_heads):
    B, Lq, E = q_row.shape
    H, W = v.shape[1], v.shape[2]
    d = L.mi_rcda_desc()
    d.q_row, d.q_col, d.k_row, d.k_col, d.v = (t.data_ptr() for t in (q_row, q_col, k_row, k_col, v))
    d.mask_row, d.mask_col = L.ptr(mask_row), L.ptr(mask_col)
    d.B, d.heads, d.L, d.H, d.W, d.E = B, num_heads, Lq, H, W, E
    d.ldq = d.ldk = d.ldv = d.ldo = E
    d.scale = float(E // num_heads) ** -0.5
    return d


class _RcdaCore(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q_row, q_col, k_row, k_col, v, mask_row, mask_col, num_heads):
        ts = (q_row, q_col, k_row, k_col, v)
        if not all(t.is_cuda for t in ts):
            raise L.MI355Error("rcda_core: the MI355X path needs device tensors (no CPU fallback)")
        B, Lq, E = q_row.shape
        H, W = v.shape[1], v.shape[2]
        if q_col.shape != q_row.shape or k_row.shape != (B, W, E) or k_col.shape != (B, H, E) or v.shape != (B, H, W, E):
            raise ValueError(f"rcda_core: shapes q_row {tuple(q_row.shape)} q_col {tuple(q_col.shape)} k_row {tuple(k_row.shape)} "
                             f"k_col {tuple(k_col.shape)} v {tuple(v.shape)}")
        q_row, q_col, k_row, k_col, v = (t.to(torch.bfloat16).contiguous() for t in ts)
        mr = None if mask_row is None else mask_row.to(torch.uint8).contiguous()
        mc = None if mask_col is None else mask_col.to(torch.uint8).contiguous()
        o = torch.empty_like(q_row)
        lse = torch.empty(2, B, num_heads, Lq, dtype=torch.float32, device=o.device)
        d = _desc(q_row, q_col, k_row, k_col, v, mr, mc, num_heads)
        d.o, d.lse_row, d.lse_col = o.data_ptr(), lse[0].data_ptr(), lse[1].data_ptr()
        L.check(L.lib().mi_rcda_fwd(C.byref(d), L.stream_ptr()), "mi_rcda_fwd")
        if any(ctx.needs_input_grad[:5]):
            ctx.save_for_backward(q_row, q_col, k_row, k_col, v, mr, mc, lse)
            ctx.num_heads = num_heads
        return o

    @staticmethod
    def backward(ctx, do):
        q_row, q_col, k_row, k_col, v, mr, mc, lse = ctx.saved_tensors
        do = do.to(torch.bfloat16).contiguous()
        d = _desc(q_row, q_col, k_row, k_col, v, mr, mc, ctx.num_heads)
        grads = [torch.empty_like(t) for t in (q_row, q_col, k_row, k_col, v)]
        d.lse_row, d.lse_col, d.dout = lse[0].data_ptr(), lse[1].data_ptr(), do.data_ptr()
        d.dq_row, d.dq_col, d.dk_row, d.dk_col, d.dv = (g.data_ptr() for g in grads)
        need = L.check(L.lib().mi_rcda_bwd_ws_bytes(C.byref(d)), "mi_rcda_bwd_ws_bytes")
        ws = torch.empty(max(int(need), 16), dtype=torch.uint8, device=do.device)
        d.ws, d.ws_bytes = ws.data_ptr(), ws.numel()
        L.check(L.lib().mi_rcda_bwd(C.byref(d), L.stream_ptr()), "mi_rcda_bwd")
        return (*grads, None, None, None)


def rcda_core(q_row, q_col, k_row, k_col, v, mask_row=None, mask_col=None, num_heads=8):
    """q_row, q_col bf16 [B, L, E]; k_row [B, W, E]; k_col [B, H, E]; v [B, H, W, E]; mask_row bool / uint8 [B, W], mask_col
    [B, H] (True = padded) or None; E = num_heads * 32.  Returns bf16 [B, L, E] (before the out-projection)."""
    return _RcdaCore.apply(q_row, q_col, k_row, k_col, v, mask_row, mask_col, num_heads)


class _KeyMeanFn(torch.autograd.Function):
    """(mean over H of key_row [B, W, E], mean over W of key_col [B, H, E]) in one launch (mi_rcda_key_mean).  The backward is
    a broadcast over H (W) divided by H (W): the divided gradient is handed to autograd as an expanded (stride 0) view - no
    kernel writes the H (W) copies; whatever consumes the map's gradient reads the one row."""

    @staticmethod
    def forward(ctx, key_row, key_col):
        B, H, W, E = key_row.shape
        key_row, key_col = key_row.to(torch.bfloat16).contiguous(), key_col.to(torch.bfloat16).contiguous()
        mr = torch.empty(B, W, E, dtype=torch.bfloat16, device=key_row.device)
        mc = torch.empty(B, H, E, dtype=torch.bfloat16, device=key_row.device)
        L.check(L.lib().mi_rcda_key_mean(key_row.data_ptr(), key_col.data_ptr(), mr.data_ptr(), mc.data_ptr(), B, H, W, E,
                                         L.stream_ptr()), "mi_rcda_key_mean")
        ctx.hw = (H, W)
        return mr, mc

    @staticmethod
    def backward(ctx, gr, gc):
        H, W = ctx.hw
        B, _, E = gr.shape
        return (gr * (1.0 / H)).unsqueeze(1).expand(B, H, W, E), (gc * (1.0 / W)).unsqueeze(2).expand(B, H, W, E)


class _InProj5Fn(torch.autograd.Function):
    """the five in-projections y_i = x_i W[iE:(i+1)E]^T + b[iE:(i+1)E] as ONE autograd node over the whole in_proj_weight
    [5E, E] / in_proj_bias [5E] (transformer._InProjFn for five row blocks): the weight-gradient launches write their row
    blocks of one gradient tensor, nothing is sliced through autograd"""

    @staticmethod
    def forward(ctx, x0, x1, x2, x3, x4, w, b):
        E = w.shape[1]
        w32 = w.detach().float().contiguous()
        b32 = None if b is None else b.detach().float().contiguous()
        outs, wds = [], []
        for i, x in enumerate((x0, x1, x2, x3, x4)):
            y, wd = _linear_fwd(x, w32[i * E:(i + 1) * E], None if b32 is None else b32[i * E:(i + 1) * E])
            outs.append(y)
            wds.append(wd)
        ctx.save_for_backward(x0, x1, x2, x3, x4, *wds)
        ctx.E = E
        ctx.params = (w, b)
        return tuple(outs)

    @staticmethod
    def backward(ctx, *dys):
        xs, wds = ctx.saved_tensors[:5], ctx.saved_tensors[5:]
        E = ctx.E
        dev = xs[0].device
        gw = torch.empty(5 * E, E, dtype=torch.float32, device=dev)
        gb = torch.empty(5 * E, dtype=torch.float32, device=dev) if ctx.params[1] is not None else None
        ok = _can_defer(*ctx.params)
        dxs = []
        for i, (x, wd, dy) in enumerate(zip(xs, wds, dys)):
            dxs.append(_linear_bwd(x, wd, dy, E, ctx.needs_input_grad[i], gw[i * E:(i + 1) * E],
                                   None if gb is None else gb[i * E:(i + 1) * E], defer_ok=ok, owner=ctx.params[0]))
        return (*dxs, gw, gb)


class MultiheadRCDA(nn.Module):
    """the reference's MultiheadRCDA.  Served: head_dim 32, maps up to 96 x 96, bf16 activations on the device, dropout 0 in
    training mode (any dropout in eval mode).  Everything else is refused by name before any launch."""

    def __init__(self, embed_dim, num_heads, dropout=0., bias=True, add_bias_kv=False, add_zero_attn=False, kdim=None, vdim=None):
        super().__init__()
        if add_bias_kv:
            raise NotImplementedError("MultiheadRCDA: add_bias_kv is not served (the reference's function never uses bias_k / bias_v)")
        if add_zero_attn:
            raise NotImplementedError("MultiheadRCDA: add_zero_attn is not served (the reference's function ignores it)")
        if (kdim is not None and kdim != embed_dim) or (vdim is not None and vdim != embed_dim):
            raise NotImplementedError("MultiheadRCDA: kdim / vdim other than embed_dim are not served")
        if embed_dim != num_heads * HEAD_DIM:
            raise NotImplementedError(f"MultiheadRCDA: head_dim must be {HEAD_DIM} (embed_dim {embed_dim}, num_heads {num_heads})")
        self.embed_dim, self.kdim, self.vdim = embed_dim, embed_dim, embed_dim
        self._qkv_same_embed_dim = True
        self.num_heads, self.dropout, self.head_dim = num_heads, dropout, embed_dim // num_heads
        self.in_proj_weight = nn.Parameter(torch.empty(5 * embed_dim, embed_dim))
        for n in ("q_row_proj_weight", "q_col_proj_weight", "k_row_proj_weight", "k_col_proj_weight", "v_proj_weight"):
            self.register_parameter(n, None)
        if bias:
            self.in_proj_bias = nn.Parameter(torch.empty(5 * embed_dim))
        else:
            self.register_parameter("in_proj_bias", None)
        self.out_proj = nn.Linear(embed_dim, embed_dim, bias=bias)
        self.bias_k_row = self.bias_k_col = self.bias_v = None
        self.add_zero_attn = False
        self._reset_parameters()

    def _reset_parameters(self):
        nn.init.xavier_uniform_(self.in_proj_weight)
        if self.in_proj_bias is not None:
            nn.init.constant_(self.in_proj_bias, 0.)
            nn.init.constant_(self.out_proj.bias, 0.)

    def forward(self, query_row, query_col, key_row, key_col, value, key_padding_mask=None, need_weights=False, attn_mask=None):
        if need_weights:
            raise NotImplementedError("MultiheadRCDA: need_weights=True is not served (the [L, B, H, W] weights are never formed)")
        if attn_mask is not None:
            raise NotImplementedError("MultiheadRCDA: attn_mask is not served (the reference does not implement it either)")
        if self.training and self.dropout > 0:
            raise NotImplementedError("MultiheadRCDA: dropout > 0 in training mode is not served (the reference's config sets 0.0)")
        ts = (query_row, query_col, key_row, key_col, value)
        if not all(t.is_cuda for t in ts):
            raise L.MI355Error("MultiheadRCDA: the MI355X path needs device tensors (no CPU fallback)")
        B, Lq, E = query_row.shape
        _, H, W, _ = value.shape
        if E != self.embed_dim:
            raise ValueError(f"MultiheadRCDA: embed_dim {E} != {self.embed_dim}")
        if H > MAX_SIDE or W > MAX_SIDE:
            raise L.MI355Error(f"MultiheadRCDA: map {H} x {W} above the served size {MAX_SIDE} x {MAX_SIDE}")
        bf = lambda t: t.to(torch.bfloat16).contiguous()
        mean_row, mean_col = _KeyMeanFn.apply(key_row, key_col)
        qr, qc, kr, kc, v = _InProj5Fn.apply(bf(query_row).view(B * Lq, E), bf(query_col).view(B * Lq, E), mean_row.view(B * W, E),
                                             mean_col.view(B * H, E), bf(value).view(B * H * W, E), self.in_proj_weight,
                                             self.in_proj_bias)
        mr = mc = None
        if key_padding_mask is not None:
            mr, mc = key_padding_mask[:, 0, :], key_padding_mask[:, :, 0]
        o = rcda_core(qr.view(B, Lq, E), qc.view(B, Lq, E), kr.view(B, W, E), kc.view(B, H, E), v.view(B, H, W, E), mr, mc,
                      self.num_heads)
        out = _LinearFn.apply(o.view(B * Lq, E), self.out_proj.weight, self.out_proj.bias)
        return out.view(B, Lq, E).transpose(0, 1), None
