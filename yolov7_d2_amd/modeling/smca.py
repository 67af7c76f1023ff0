"""SMCA (spatially modulated co-attention) on the MI355X attention kernels - the transformer of SMCA-DETR
(yolov7/modeling/backbone/smcadetr_backbone.py:27-152, 215-324 and layers/smca_attention.py): `GaussianMultiheadAttention`,
the decoder layer with its point / scale heads, the decoder and the `Transformer`, with the reference's module paths and
state_dict keys.

The reference adds a dense Gaussian-like prior [Lq, Lk, B*heads] to the attention scores.  Here the prior is the closed form

    G[q][key] = -| a dx^2 + b dy^2 + c dx^2 dy^2 | / smooth,    dx = px - key % W,  dy = py - key // W

of five numbers per (query, batch, head), evaluated inside the fused kernels (csrc/mha.hip, PRIOR instantiations: mi_smca_fwd /
mi_smca_bwd); the four `dynamic_scale` types map onto (a, b, c):

    type1 (1, 1, 0)    type2 (s^2, s^2, 0)    type3 (sx^2, sy^2, 0)    type4 (sx^2, sy^2, sxy^2)

Which nodes run where (device path): norm4, the residual LayerNorms, the self-attention, the FFN, the in / out projections and
the two hidden 256 -> 256 ReLU layers of point1 are the token-row kernels of modeling/transformer.py; the last layer of point1
and point2 / point3 (2, 2*heads, heads..3*heads outputs) are plain fp32 torch linears: their outputs are grid coordinates and
squared scales, which the bf16 output of the token-row GEMM would round to a quarter of a cell at x = 40.
Host tensors (any dtype) and the reference's `gaussian=[dense]` call form take a plain torch composition.
"""
import ctypes as C
import math

import torch
import torch.nn.functional as F
from torch import nn

from .. import _lib as L
from .attention import _O32
from .detr import MLP
from .transformer import (MultiheadAttention, TransformerEncoder, TransformerEncoderLayer, _AddFn, _InProjFn, _LayerNormFn,
                          _LinearFn, _next_seed, _tok, wgrad_flush_point)

HEAD_DIM = 32
TYPES = ("type1", "type2", "type3", "type4")


# ------------------------------------------------------------------ the operator
def _desc(q, k, v, m, point, coef, map_hw, smooth, num_heads, drop_p, seed):
    Lq, B, E = q.shape
    d = L.mi_smca_desc()
    d.q, d.k, d.v, d.mask, d.point, d.coef = q.data_ptr(), k.data_ptr(), v.data_ptr(), L.ptr(m), point.data_ptr(), coef.data_ptr()
    d.B, d.H, d.Lq, d.Lk, d.E, d.ldq, d.ldk = B, num_heads, Lq, k.shape[0], E, E, E
    d.map_h, d.map_w = int(map_hw[0]), int(map_hw[1])
    d.scale, d.inv_smooth, d.drop_p, d.seed = 1.0 / math.sqrt(E // num_heads), 1.0 / float(smooth), float(drop_p), int(seed)
    return d


class _SmcaCore(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, point, coef, mask, map_hw, smooth, num_heads, drop_p, seed):
        if not all(t.is_cuda for t in (q, k, v, point, coef)):
            raise L.MI355Error("smca_core: the MI355X path needs device tensors (no CPU fallback)")
        Lq, B, E = q.shape
        Lk = k.shape[0]
        if tuple(point.shape) != (Lq, B, num_heads, 2) or tuple(coef.shape) != (Lq, B, num_heads, 3):
            raise ValueError(f"smca_core: point {tuple(point.shape)} / coef {tuple(coef.shape)} for q {tuple(q.shape)}, {num_heads} heads")
        if int(map_hw[0]) * int(map_hw[1]) != Lk:
            raise ValueError(f"smca_core: {Lk} keys are not a {map_hw[0]} x {map_hw[1]} map")
        q, k, v = (t.to(torch.bfloat16).contiguous() for t in (q, k, v))
        point, coef = point.float().contiguous(), coef.float().contiguous()
        m = None if mask is None else mask.to(torch.uint8).contiguous()
        o = torch.empty_like(q)
        need32 = _O32() and any(ctx.needs_input_grad[:5])
        o32 = torch.empty(Lq, B, E, dtype=torch.float32, device=q.device) if need32 else None
        lse = torch.empty(B, num_heads, Lq, dtype=torch.float32, device=q.device)
        d = _desc(q, k, v, m, point, coef, map_hw, smooth, num_heads, drop_p, seed)
        d.o, d.o_f32, d.lse = o.data_ptr(), L.ptr(o32), lse.data_ptr()
        L.check(L.lib().mi_smca_fwd(C.byref(d), L.stream_ptr()), "mi_smca_fwd")
        ctx.save_for_backward(q, k, v, point, coef, m, o, lse, o32)
        ctx.args = (tuple(int(x) for x in map_hw), float(smooth), num_heads, float(drop_p), int(seed))
        return o

    @staticmethod
    def backward(ctx, do):
        q, k, v, point, coef, m, o, lse, o32 = ctx.saved_tensors
        do = do.to(torch.bfloat16).contiguous()
        dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        dpoint, dcoef = torch.empty_like(point), torch.empty_like(coef)
        delta = torch.empty_like(lse)
        d = _desc(q, k, v, m, point, coef, *ctx.args)
        d.o, d.o_f32, d.lse, d.dout, d.delta = o.data_ptr(), L.ptr(o32), lse.data_ptr(), do.data_ptr(), delta.data_ptr()
        d.dq, d.dk, d.dv, d.dpoint, d.dcoef = dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), dpoint.data_ptr(), dcoef.data_ptr()
        L.check(L.lib().mi_smca_bwd(C.byref(d), L.stream_ptr()), "mi_smca_bwd")
        return dq, dk, dv, dpoint, dcoef, None, None, None, None, None, None


def smca_core(q, k, v, point, coef, map_hw, smooth, key_padding_mask=None, num_heads=8, dropout_p=0.0, seed=0):
    """q bf16 [Lq, B, E], k / v [Lk, B, E] (after the in-projection, E = num_heads * 32, Lk = map_hw[0] * map_hw[1]);
    point fp32 [Lq, B, heads, 2] = (px, py) in grid cells; coef fp32 [Lq, B, heads, 3] = (a, b, c); key_padding_mask bool / uint8
    [B, Lk] (True = padded).  Returns bf16 [Lq, B, E] (before the out-projection); gradients for q, k, v, point and coef."""
    return _SmcaCore.apply(q, k, v, point, coef, key_padding_mask, map_hw, smooth, num_heads, dropout_p, seed)


def dense_gaussian(point, coef, map_hw, smooth):
    """the reference's dense prior [Lq, Lk, B*heads] (smcadetr_backbone.py:285-310) from point [Lq, B, heads, 2] and coef
    [Lq, B, heads, 3], in their dtype: what `gaussian=[...]` takes"""
    Lq = point.shape[0]
    h, w = int(map_hw[0]), int(map_hw[1])
    gy, gx = torch.meshgrid(torch.arange(h, device=point.device), torch.arange(w, device=point.device), indexing="ij")
    grid = torch.stack((gx, gy), 2).to(point.dtype).reshape(-1, 1, 2)                    # [Lk, 1, (x, y)]
    d2 = (point.reshape(Lq, 1, -1, 2) - grid.unsqueeze(0)).pow(2)                       # [Lq, Lk, B*heads, 2]
    c = coef.reshape(Lq, 1, -1, 3)
    dist = c[..., 0] * d2[..., 0] + c[..., 1] * d2[..., 1] + c[..., 2] * (d2[..., 0] * d2[..., 1])
    return -dist.abs() / smooth


def attention_torch(q, k, v, gaussian, key_padding_mask, num_heads, dropout_p=0.0):
    """smca_attention.py:179-287 after the in-projection, as plain torch in the operands' dtype: scores = (q * hd^-0.5) k^T,
    -inf on padded keys, + gaussian.permute(2, 0, 1), softmax, dropout, x v.  q [Lq, B, E], k / v [Lk, B, E] -> [Lq, B, E]"""
    Lq, B, E = q.shape
    Lk = k.shape[0]
    hd = E // num_heads
    qh = (q * float(hd) ** -0.5).contiguous().view(Lq, B * num_heads, hd).transpose(0, 1)
    kh = k.contiguous().view(Lk, B * num_heads, hd).transpose(0, 1)
    vh = v.contiguous().view(Lk, B * num_heads, hd).transpose(0, 1)
    w = torch.bmm(qh, kh.transpose(1, 2))
    if key_padding_mask is not None:
        w = w.view(B, num_heads, Lq, Lk).masked_fill(key_padding_mask.to(torch.bool).unsqueeze(1).unsqueeze(2), float("-inf"))
        w = w.view(B * num_heads, Lq, Lk)
    if gaussian is not None:
        w = w + gaussian.permute(2, 0, 1).to(w.dtype)
    w = F.softmax(w, dim=-1)
    if dropout_p > 0:
        w = F.dropout(w, p=dropout_p, training=True)
    return torch.bmm(w, vh).transpose(0, 1).contiguous().view(Lq, B, E)


def _mha_torch(mod, query, key, value, key_padding_mask, gaussian=None):
    """nn.MultiheadAttention's arithmetic on a module holding in_proj_weight / in_proj_bias / out_proj, in the inputs' dtype"""
    E = mod.embed_dim
    dt = query.dtype
    w, b = mod.in_proj_weight.to(dt), mod.in_proj_bias.to(dt)
    q, k, v = F.linear(query, w[:E], b[:E]), F.linear(key, w[E:2 * E], b[E:2 * E]), F.linear(value, w[2 * E:], b[2 * E:])
    o = attention_torch(q, k, v, gaussian, key_padding_mask, mod.num_heads, mod.dropout if mod.training else 0.0)
    return F.linear(o, mod.out_proj.weight.to(dt), mod.out_proj.bias.to(dt))


class GaussianMultiheadAttention(MultiheadAttention):
    """the reference's GaussianMultiheadAttention (parameters and state_dict keys of nn.MultiheadAttention).
    prior=(point, coef, map_hw, smooth): the fused path on device tensors (the dense prior is never formed); on host tensors the
    dense prior is built from it and the torch composition runs.  gaussian=[dense [Lq, Lk, B*heads]]: the reference's call form,
    always the torch composition."""

    def __init__(self, embed_dim, num_heads, dropout=0.0):
        super().__init__(embed_dim, num_heads, dropout)
        self.gaussian = True

    def forward(self, query, key, value, key_padding_mask=None, need_weights=False, attn_mask=None, gaussian=None, prior=None):
        if attn_mask is not None:
            raise NotImplementedError("GaussianMultiheadAttention: attn_mask is not served (the reference always passes None)")
        if need_weights:
            raise NotImplementedError("GaussianMultiheadAttention: need_weights=True is not served (the weights are never formed)")
        if (gaussian is None) == (prior is None):
            raise ValueError("GaussianMultiheadAttention: pass exactly one of prior=(point, coef, map_hw, smooth) and gaussian=[dense]")
        if gaussian is not None:
            return _mha_torch(self, query, key, value, key_padding_mask, gaussian[0]), None
        point, coef, map_hw, smooth = prior
        if not query.is_cuda:
            return _mha_torch(self, query, key, value, key_padding_mask, dense_gaussian(point, coef, map_hw, smooth)), None
        E = self.embed_dim
        Lq, B, _ = query.shape
        Lk = key.shape[0]
        q, k, v = _InProjFn.apply(_tok(query).view(Lq * B, E), _tok(key).view(Lk * B, E), _tok(value).view(Lk * B, E),
                                  self.in_proj_weight, self.in_proj_bias)
        drop = self.dropout if self.training else 0.0
        o = smca_core(q.view(Lq, B, E), k.view(Lk, B, E), v.view(Lk, B, E), point, coef, map_hw, smooth, key_padding_mask,
                      self.num_heads, drop, _next_seed() if drop > 0 else 0)
        out = _LinearFn.apply(o.reshape(Lq * B, E), self.out_proj.weight, self.out_proj.bias).view(Lq, B, E)
        return out, None


# ------------------------------------------------------------------ decoder layer, decoder, transformer
def _ln(norm, x):
    if not x.is_cuda:
        return F.layer_norm(x, norm.normalized_shape, norm.weight.to(x.dtype), norm.bias.to(x.dtype), norm.eps)
    Lx, B, E = x.shape
    return _LayerNormFn.apply(x.reshape(Lx * B, E), norm.weight, norm.bias, norm.eps).view(Lx, B, E)


def _add(a, b):
    return a + b if not a.is_cuda else _AddFn.apply(_tok(a), _tok(b))


def _lin(lin, x, relu=False):
    """a hidden linear: the token-row GEMM on the device (bf16 out), F.linear on the host"""
    if not x.is_cuda:
        y = F.linear(x, lin.weight.to(x.dtype), lin.bias.to(x.dtype))
        return F.relu(y) if relu else y
    shp = x.shape
    return _LinearFn.apply(_tok(x).reshape(-1, shp[-1]), lin.weight, lin.bias, relu).view(*shp[:-1], lin.out_features)


def _head(lin, x):
    """a point / scale head: fp32 on the device (coordinates must not be rounded to bf16), the input's dtype on the host"""
    dt = torch.float32 if x.is_cuda else x.dtype
    return F.linear(x.to(dt), lin.weight.to(dt), lin.bias.to(dt))


def _self_attn(mod, q, v, mask):
    if not q.is_cuda:
        return _mha_torch(mod, q, q, v, mask)
    return mod(q, q, value=v, key_padding_mask=mask)[0]


def _res_norm(layer, norm, res, x):
    """norm(res + dropout(x))"""
    if not x.is_cuda:
        return _ln(norm, res + F.dropout(x, layer.dropout_p, layer.training))
    return layer._ln_res(norm, res, x)


def _ffn(layer, x):
    if not x.is_cuda:
        return _lin(layer.linear2, F.dropout(_lin(layer.linear1, x, True), layer.dropout_p, layer.training))
    return layer._ffn(x)


class SMCATransformerDecoderLayer(nn.Module):
    """smcadetr_backbone.py:215-324 (forward_post; forward_pre there has another signature and cannot run: refused)"""

    def __init__(self, dynamic_scale, smooth, layer_index, d_model, nhead, dim_feedforward=2048, dropout=0.1, activation="relu",
                 normalize_before=False):
        super().__init__()
        if activation != "relu":
            raise NotImplementedError(activation)
        if normalize_before:
            raise NotImplementedError("SMCATransformerDecoderLayer: normalize_before=True is not served (the reference's forward_pre "
                                      "takes no grid / h_w and cannot be called by its decoder)")
        if dynamic_scale not in TYPES:
            raise ValueError(f"SMCATransformerDecoderLayer: dynamic_scale {dynamic_scale!r} is not one of {TYPES}")
        assert d_model == HEAD_DIM * nhead, "the MFMA attention kernel is built for head_dim 32 (d_model == 32 * nhead)"
        self.self_attn = MultiheadAttention(d_model, nhead, dropout=dropout)
        self.multihead_attn = GaussianMultiheadAttention(d_model, nhead, dropout=dropout)
        self.linear1 = nn.Linear(d_model, dim_feedforward)
        self.linear2 = nn.Linear(dim_feedforward, d_model)
        self.smooth, self.dynamic_scale, self.nhead = smooth, dynamic_scale, nhead
        self.norm1 = nn.LayerNorm(d_model)
        self.norm2 = nn.LayerNorm(d_model)
        self.norm3 = nn.LayerNorm(d_model)
        self.norm4 = nn.LayerNorm(d_model)
        self.dropout_p = dropout
        if layer_index == 0:
            self.point1 = MLP(d_model, d_model, 2, 3)
        self.point2 = nn.Linear(d_model, 2 * nhead)
        self.layer_index = layer_index
        if dynamic_scale != "type1":
            self.point3 = nn.Linear(d_model, {"type2": 1, "type3": 2, "type4": 3}[dynamic_scale] * nhead)
        self.normalize_before = normalize_before

    _ln_res = TransformerEncoderLayer._ln_res
    _ffn = TransformerEncoderLayer._ffn

    def prior(self, out, h_w, point_ref_previous):
        """the point / scale heads on out = norm4(tgt + query_pos): (point [Lq, B, heads, 2], coef [Lq, B, heads, 3],
        point_sigmoid_ref_inter or None, point_sigmoid_ref [Lq, B, 2 * heads])"""
        Lq, B, _ = out.shape
        H = self.nhead
        offset = _head(self.point2, out)
        inter = None
        if self.layer_index == 0:
            x = out
            for lin in self.point1.layers[:-1]:
                x = _lin(lin, x, True)
            inter = _head(self.point1.layers[-1], x)
            ref = ((h_w.to(inter.dtype) - 0) * inter.sigmoid() / 32).repeat(1, 1, H)
        else:
            ref = point_ref_previous
        point = (ref + offset).view(Lq, B, H, 2)
        if self.dynamic_scale == "type1":
            coef = torch.cat([torch.ones_like(point), torch.zeros_like(point[..., :1])], -1)
        else:
            s = _head(self.point3, out)
            s = s * s
            if self.dynamic_scale == "type2":
                s = s.view(Lq, B, H, 1)
                coef = torch.cat([s, s, torch.zeros_like(s)], -1)
            elif self.dynamic_scale == "type3":
                s = s.view(Lq, B, H, 2)
                coef = torch.cat([s, torch.zeros_like(s[..., :1])], -1)
            else:
                coef = s.view(Lq, B, H, 3)
        return point, coef, inter, ref

    def forward(self, map_hw, h_w, tgt, memory, tgt_mask=None, memory_mask=None, tgt_key_padding_mask=None,
                memory_key_padding_mask=None, pos=None, query_pos=None, point_ref_previous=None, mem_k=None):
        """map_hw = (h, w) of the feature map stands where the reference passes its dense `grid`"""
        if tgt_mask is not None or memory_mask is not None:
            raise NotImplementedError("SMCATransformerDecoderLayer: attn masks are not served (the reference always passes None)")
        if tgt.is_cuda:
            tgt, memory = wgrad_flush_point(_tok(tgt)), _tok(memory)
        if mem_k is None:
            mem_k = _add(memory, pos)
        # the reference takes norm4 and the offset head before the self-attention, from the layer's input
        q = _add(tgt, query_pos)
        out = _ln(self.norm4, q)
        point, coef, inter, ref = self.prior(out, h_w, point_ref_previous)
        tgt = _res_norm(self, self.norm1, tgt, _self_attn(self.self_attn, q, tgt, tgt_key_padding_mask))
        tgt2 = self.multihead_attn(_add(tgt, query_pos), mem_k, memory, key_padding_mask=memory_key_padding_mask,
                                   prior=(point, coef, map_hw, self.smooth))[0]
        tgt = _res_norm(self, self.norm2, tgt, tgt2)
        tgt = _res_norm(self, self.norm3, tgt, _ffn(self, tgt))
        return tgt, inter, ref


class SMCATransformerDecoder(nn.Module):
    """smcadetr_backbone.py:110-152: a list of (different) layers; point_sigmoid_ref is handed from layer to layer"""

    def __init__(self, decoder_layer, num_layers, norm=None, return_intermediate=False):
        super().__init__()
        self.layers = nn.ModuleList(decoder_layer)
        self.num_layers = num_layers
        self.norm = norm
        self.return_intermediate = return_intermediate

    def forward(self, map_hw, h_w, tgt, memory, tgt_mask=None, memory_mask=None, tgt_key_padding_mask=None,
                memory_key_padding_mask=None, pos=None, query_pos=None):
        output = tgt
        if tgt.is_cuda:
            output, memory, pos, query_pos = _tok(tgt), _tok(memory), _tok(pos), _tok(query_pos)
        mem_k = _add(memory, pos)       # the same sum in every layer: formed once
        intermediate, points, ref = [], [], None
        for layer in self.layers:
            output, point, ref = layer(map_hw, h_w, output, memory, tgt_mask=tgt_mask, memory_mask=memory_mask,
                                       tgt_key_padding_mask=tgt_key_padding_mask, memory_key_padding_mask=memory_key_padding_mask,
                                       pos=pos, query_pos=query_pos, point_ref_previous=ref, mem_k=mem_k)
            points.append(point)
            if self.return_intermediate:
                intermediate.append(_ln(self.norm, output))
        if self.norm is not None:
            output = intermediate[-1] if self.return_intermediate else _ln(self.norm, output)
        if self.return_intermediate:
            return torch.stack(intermediate), points[0]
        return output.unsqueeze(0)


def _encoder_torch(enc, src, mask, pos):
    """the existing TransformerEncoder's modules as plain torch, for host tensors (post-norm, as the decoder requires)"""
    x = src
    for layer in enc.layers:
        q = x + pos
        x = _res_norm(layer, layer.norm1, x, _mha_torch(layer.self_attn, q, q, x, mask))
        x = _res_norm(layer, layer.norm2, x, _ffn(layer, x))
    return x if enc.norm is None else _ln(enc.norm, x)


class SMCATransformer(nn.Module):
    """smcadetr_backbone.py:27-83: src [B, C, H, W], mask [B, H, W] (True = padding), query_embed [Q, C], pos_embed [B, C, H, W],
    h_w [1, B, 2] = (image width, image height)  ->  (hs [layers, B, Q, C], points [B, Q, 2]: layer 0's reference points before
    the sigmoid)"""

    def __init__(self, d_model=512, nhead=8, num_encoder_layers=6, num_decoder_layers=6, dim_feedforward=2048, dropout=0.1,
                 activation="relu", normalize_before=False, return_intermediate_dec=False, smooth=8, dynamic_scale="type3"):
        super().__init__()
        if normalize_before:
            raise NotImplementedError("SMCATransformer: normalize_before=True is not served (the reference's decoder cannot run it)")
        enc = TransformerEncoderLayer(d_model, nhead, dim_feedforward, dropout, activation, normalize_before)
        self.encoder = TransformerEncoder(enc, num_encoder_layers, None)
        layers = [SMCATransformerDecoderLayer(dynamic_scale, smooth, i, d_model, nhead, dim_feedforward, dropout, activation,
                                              normalize_before) for i in range(num_decoder_layers)]
        self.decoder = SMCATransformerDecoder(layers, num_decoder_layers, nn.LayerNorm(d_model), return_intermediate=return_intermediate_dec)
        self._reset_parameters()
        if dynamic_scale != "type1":
            for layer in self.decoder.layers:
                nn.init.zeros_(layer.point3.weight)
                nn.init.ones_(layer.point3.bias)
        self.d_model, self.nhead = d_model, nhead

    def _reset_parameters(self):
        for p in self.parameters():
            if p.dim() > 1:
                nn.init.xavier_uniform_(p)

    def forward(self, src, mask, query_embed, pos_embed, h_w):
        bs, c, h, w = src.shape
        src = src.flatten(2).permute(2, 0, 1)
        pos_embed = pos_embed.flatten(2).permute(2, 0, 1)
        query_embed = query_embed.unsqueeze(1).repeat(1, bs, 1)
        mask = mask.flatten(1)
        if src.is_cuda:
            if not pos_embed.requires_grad:
                pos_embed = _tok(pos_embed)
            mask = mask.to(torch.uint8).contiguous()
            tgt = torch.zeros_like(query_embed, dtype=torch.bfloat16)
            memory = self.encoder(src, src_key_padding_mask=mask, pos=pos_embed)
        else:
            tgt = torch.zeros_like(query_embed)
            memory = _encoder_torch(self.encoder, src, mask, pos_embed)
        out = self.decoder((h, w), h_w, tgt, memory, memory_key_padding_mask=mask, pos=pos_embed, query_pos=query_embed)
        if not self.decoder.return_intermediate:
            return out.transpose(1, 2)
        hs, points = out
        return hs.transpose(1, 2), points.transpose(0, 1)
