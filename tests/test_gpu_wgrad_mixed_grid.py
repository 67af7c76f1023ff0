"""GPU (-m gpu): the mixed grid of the grouped weight gradient (MI_WG_MULTI; csrc/conv_wgrad.hip wgrad2_multi_kernel: the 1x1
layers of a plan in ONE grid whatever their tile widths) against one grid per tile configuration, through the C-ABI
(mi_conv2d_wgrad_group_plan / _run): conv wgrad of BaseConv (layers/wrappers.py:60-83) for the layer shapes of the YOLOX-s
step, both forms against torch."""
import ctypes as C

import pytest
import torch

from yolov7_d2_amd import _lib as L

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _rup(a, b):
    return (a + b - 1) // b * b


def _layer(k, stride, Cin, Cout, N, H, W, seed, accumulate=0, scaled=False):
    g = torch.Generator().manual_seed(seed)
    CinPad = _rup(Cin, 16) if k > 1 else _rup(Cin, 32)
    CoutPad = _rup(Cout, 32)
    pad = k // 2
    oH, oW = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    x = torch.zeros(N, H, W, CinPad, dtype=torch.bfloat16)
    x[..., :Cin] = torch.randn(N, H, W, Cin, generator=g).to(torch.bfloat16)
    dy = torch.zeros(N, oH, oW, CoutPad, dtype=torch.bfloat16)
    dy[..., :Cout] = (torch.randn(N, oH, oW, Cout, generator=g) * 0.1).to(torch.bfloat16)
    g0 = torch.randn(Cout, Cin, k, k, generator=g)
    rs = (0.5 + torch.rand(Cout, generator=g)) if scaled else None
    return dict(k=k, stride=stride, Cin=Cin, Cout=Cout, CinPad=CinPad, CoutPad=CoutPad, N=N, H=H, W=W, oH=oH, oW=oW,
                x=x.to(DEV), dy=dy.to(DEV), g0=g0, accumulate=accumulate, rs=None if rs is None else rs.to(DEV))


def _descs(layers, gws):
    descs = (L.mi_wgrad_desc * len(layers))()
    for d, l, gw in zip(descs, layers, gws):
        d.x, d.dy, d.gw = l["x"].data_ptr(), l["dy"].data_ptr(), gw.data_ptr()
        d.ldx, d.ldy = l["CinPad"], l["CoutPad"]
        d.N, d.H, d.W, d.outH, d.outW, d.stride = l["N"], l["H"], l["W"], l["oH"], l["oW"], l["stride"]
        d.Cin, d.Cout, d.CinPad, d.CoutPad = l["Cin"], l["Cout"], l["CinPad"], l["CoutPad"]
        k, pad = l["k"], l["k"] // 2
        d.ntaps = k * k
        for t, (r, s) in enumerate((r, s) for r in range(k) for s in range(k)):
            d.tap_dy[t], d.tap_dx[t] = r - pad, s - pad
        d.accumulate = l["accumulate"]
        d.row_scale = l["rs"].data_ptr() if l["rs"] is not None else None
    return descs


def _run_group(layers, monkeypatch, multi, runs=1):
    """plan + upload + run the grouped launch `runs` times; returns the gradients after every run and the launch meta"""
    lib = L.lib()
    monkeypatch.setenv("MI_WG_MULTI", multi)
    gws = [l["g0"].clone().to(DEV) for l in layers]
    descs = _descs(layers, gws)
    meta = L.mi_wgrad_group()
    L.check(lib.mi_conv2d_wgrad_group_plan(descs, len(layers), None, None, 0, C.byref(meta)), "plan (sizes)")
    ws = torch.empty(int(meta.ws_bytes) + 256, dtype=torch.uint8, device=DEV)
    ws.fill_(0xFF)                                                   # stale partials must never be read as sums
    host = (C.c_char * int(meta.table_bytes))()
    L.check(lib.mi_conv2d_wgrad_group_plan(descs, len(layers), ws.data_ptr(), host, meta.table_bytes, C.byref(meta)), "plan")
    table = torch.frombuffer(bytearray(bytes(host)[:int(meta.table_bytes)]), dtype=torch.uint8).to(DEV)
    outs = []
    st = torch.cuda.current_stream().cuda_stream
    for _ in range(runs):
        L.check(lib.mi_conv2d_wgrad_group_run(C.byref(meta), table.data_ptr(), st), "run")
        torch.cuda.synchronize()
        outs.append([g.cpu().clone() for g in gws])
    return outs, meta


YOLOX_LAYERS = [
    # k, stride, Cin, Cout, N, H, W                (CSPDarknet / PAFPN / head shapes of the 640 x 640 step, batch 4)
    (3, 1, 64, 64, 4, 80, 80),       # dark3 bottleneck conv2: the 64 x 64 x 9 tile configuration
    (3, 1, 32, 32, 4, 160, 160),     # dark2 bottleneck conv2
    (3, 2, 32, 64, 4, 160, 160),     # dark2.0 (stride 2)
    (3, 2, 128, 256, 4, 40, 40),     # dark4.0
    (3, 1, 16, 32, 4, 96, 96),       # stem (Focus output: 12 -> 16 channels)
    (1, 1, 128, 128, 4, 80, 80),     # CSP conv1
    (1, 1, 512, 256, 4, 20, 20),     # lateral conv
    (1, 1, 256, 512, 4, 20, 20),
    (1, 1, 64, 32, 4, 160, 160),
    (3, 1, 128, 128, 4, 40, 40),     # head tower
    (1, 1, 128, 85, 4, 40, 40),      # prediction convs (Cout 85 -> pad 96; reads a map with padded channels)
]


def test_mixed_grid_equals_one_grid_per_configuration(monkeypatch):
    """MI_WG_MULTI (round 6: the 1x1 layers of a plan in ONE grid whatever their tile widths, wgrad2_multi_kernel) against one
    grid per tile configuration: fewer groups, the same gradients up to the split-K summation order (the pooled slot count
    changes the splits), and both equal to the fp64 reference"""
    layers = [_layer(*s, seed=300 + i) for i, s in enumerate(YOLOX_LAYERS)]
    ref, meta0 = _run_group(layers, monkeypatch, "0")
    got, meta1 = _run_group(layers, monkeypatch, "3")   # (3: forced for this 11-layer plan; the default needs >= 16 1x1 layers)
    assert meta1.ngroups < meta0.ngroups
    assert any(meta1.g[i].cfg[0] == 1 and meta1.g[i].cfg[1] == 0 for i in range(meta1.ngroups))
    for l, s, a, b in zip(layers, YOLOX_LAYERS, ref[0], got[0]):
        xr = l["x"][..., :l["Cin"]].float().permute(0, 3, 1, 2).cpu()
        dyr = l["dy"][..., :l["Cout"]].float().permute(0, 3, 1, 2).cpu()
        w = torch.zeros(l["Cout"], l["Cin"], l["k"], l["k"], requires_grad=True)
        torch.nn.functional.conv2d(xr, w, stride=l["stride"], padding=l["k"] // 2).backward(dyr)
        assert float((b - w.grad).norm() / w.grad.norm()) < 2e-3, s
        assert float((a - b).abs().max()) <= 1e-5 * float(w.grad.abs().max()) + 1e-7, s   # (fp32 sums in another order)
