"""GPU (-m gpu): the block-statistics tail of the persistent convolution kernels (csrc/conv_bn.h cbn_block_stats: counted
wait, halving exchange over the lanes, LDS stage over the waves, fp64 slot atomics) - c1s_kernel MODE 1 and its XF form
(csrc/conv1x1_stream.h), w3_kernel MODE 1 (csrc/conv3x3_ws.h) - checked with EQUALITY, the method of tests/test_gpu_bn_exact.py:

  x holds integers in [-2, 2], a weight row holds at most 8 nonzero entries, all of them +-1.  Then |y| <= 16: every output is
  an integer that bf16 stores exactly, and a block's fp32 partial sums - at most 16 * P and 256 * P over the P pixels the block
  owns - stay below 2^24, so they are exact in any order, and so are the fp64 totals.  The bounds are asserted on the host
  operands before anything is launched (check_premise).

Every case asserts (1) the slot accumulators, summed over the slots, equal the fp64 sums of the kernel's OWN stored y, (2) y is
bit-equal to the tile kernel's (MI_CONV_STREAM=0 / MI_CONV_WS=0), (3) slots beyond stats_slots stay untouched.

Shapes: the smallest at which the tail can go wrong - every (K, waves over cout, pixel tile) instantiation c1s_fill can
choose; maps with exactly one tile per block, with fewer tiles than the chip has blocks, and with a tile count that is no
multiple of the block count (some blocks run one tile fewer and their last LDS-DMAs come from the zero page: the case the
counted wait must survive); two convolutions of one input; channel-slice views; 1 and 8 slots; for w3 K = 32 / 64 / 128,
the stride-2 K -> 2 K form and three jobs of different maps in one launch, one of them with partial tiles."""
import ctypes as C

import pytest
import torch

from yolov7_d2_amd import _lib as L

pytestmark = pytest.mark.gpu
DEV = "cuda"
XMAX, NNZ = 2, 8
ALL_SLOTS = L.MI_BN_SLOTS


def sp():
    return L.stream_ptr()


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def ints(shape, seed, hi=XMAX):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-hi, hi + 1, shape, generator=g).float()


def sparse_w(cout, cin, k, seed):
    """OIHW fp32: NNZ entries of +-1 per output channel, the rest 0"""
    g = torch.Generator().manual_seed(seed)
    w = torch.zeros(cout, cin * k * k)
    for co in range(cout):
        pos = torch.randperm(cin * k * k, generator=g)[:NNZ]
        w[co, pos] = (torch.randint(0, 2, (NNZ,), generator=g) * 2 - 1).float()
    return w.view(cout, cin, k, k).contiguous()


def check_premise(x, ws, block_pixels):
    """on the host operands: |x| <= XMAX integers, <= NNZ entries of +-1 per weight row -> |y| <= 16; the pixels one block sums"""
    assert float(x.abs().max()) <= XMAX and bool((x == x.round()).all())
    for w in ws:
        assert int((w != 0).flatten(1).sum(1).max()) <= NNZ and float(w.abs().max()) <= 1
    ymax = NNZ * XMAX
    assert ymax <= 256 and ymax * ymax * block_pixels < 2 ** 24, (ymax, block_pixels)


def stats_buf(c):
    st = torch.full((ALL_SLOTS, c, 2), -1536.0, dtype=torch.float64, device=DEV)
    return st


def check_stats(st, nslots, y, what):
    """st [ALL_SLOTS][C][2] after the launch; y [..., C] the kernel's own output (bf16)"""
    c = y.shape[-1]
    v = y.reshape(-1, c).double()
    got = st[:nslots].sum(0)
    assert bool((st[nslots:] == -1536.0).all()), (what, "slots beyond stats_slots were written")
    assert torch.equal(got[:, 0], v.sum(0)), (what, "sum", (got[:, 0] - v.sum(0)).abs().max().item())
    assert torch.equal(got[:, 1], (v * v).sum(0)), (what, "sum of squares", (got[:, 1] - (v * v).sum(0)).abs().max().item())
    assert float(v.abs().max()) <= NNZ * XMAX and bool((v != 0).any())


# ------------------------------------------------------------------------------------------------------ streaming 1x1
def pack1(w):
    cout, k = w.shape[:2]
    wf = torch.empty(k * cout, dtype=torch.bfloat16, device=DEV)
    wd = w.to(DEV)
    L.check(L.lib().mi_pack_conv_weight(wd.data_ptr(), cout, k, 1, 1, wf.data_ptr(), k, cout, None, 0, 0, sp()), "pack")
    torch.cuda.synchronize()
    return wf


def desc1(x, ldx, xoff, npix_hw, K, wf, y, ldy, yoff, cout, st, nslots):
    H, W = npix_hw
    d = L.mi_conv_desc()
    d.x, d.w, d.y = x.data_ptr() + xoff * 2, wf.data_ptr(), y.data_ptr() + yoff * 2
    d.ldx, d.ldy = ldx, ldy
    d.N, d.H, d.W, d.outH, d.outW, d.gridH, d.gridW = 1, H, W, H, W, H, W
    d.in_stride = d.out_stride = 1
    d.K8, d.Cout, d.CoutPad, d.ntaps = K // 8, cout, cout, 1
    if st is not None:
        d.stats_acc, d.stats_slots = st.data_ptr(), nslots
    return d


def c1_form(K, couts, ntiles_for):
    """c1s_fill, mirrored: waves over cout, pixel tile, cout tiles and blocks per cout tile for n slices of 32 channels.
    ntiles_for(tpix, nb) -> the tile count the case wants"""
    ns = sum(couts) // 32
    wm = 4 if ns % 4 == 0 else (2 if ns % 2 == 0 else 1)
    nco = ns // wm
    nb = max(cus() // nco, 1)
    if nco > 1 and nb >= 8:
        nb &= ~7
    valid = lambda tp: (tp * K * 2) % 8192 == 0 and tp * K * 2 * (2 if tp * K * 2 >= 65536 else (3 if tp * K * 2 >= 32768 else 4)) <= 160 * 1024
    tpix = 256 if wm == 1 else 128
    if wm == 4:
        nt = ntiles_for(128, nb)
        small = nt * nco < 2 * cus()
        if not valid(128) or (small and valid(64)):
            tpix = 64
    assert valid(tpix), (K, wm, tpix)
    return wm, tpix, nco, nb


# how many tiles a map gets, given the blocks per cout tile
MAPS = {
    "one_tile_per_block": lambda nb: nb,
    "fewer_tiles_than_blocks": lambda nb: 5,
    "uneven": lambda nb: nb + 3,                     # three blocks run two tiles, the others one and two zero-page rounds
    "uneven_many": lambda nb: 2 * nb + nb // 2 + 1,
}
C1_CASES = (
    # K, couts, map, x channel offset, y channel offset (ldy = offset + Cout), the form the case is there for
    [(K, (512,), "big", 0, 0, (4, 128)) for K in (32, 64, 128, 256)] +
    [(K, (128,), "uneven", 0, 0, (4, 64)) for K in (64, 128, 256, 512)] +
    [(K, (64,), "uneven", 0, 0, (2, 128)) for K in (32, 64, 128, 256)] +
    [(K, (32,), "uneven", 0, 0, (1, 256)) for K in (32, 64, 128)] +
    [(128, (128,), "one_tile_per_block", 0, 0, (4, 64)), (64, (64,), "one_tile_per_block", 0, 0, (2, 128)),
     (128, (128,), "fewer_tiles_than_blocks", 0, 0, (4, 64)), (32, (32,), "fewer_tiles_than_blocks", 0, 0, (1, 256)),
     (512, (128,), "uneven_many", 0, 0, (4, 64)), (64, (64,), "uneven_many", 0, 0, (2, 128)),
     (128, (64, 64), "uneven", 0, 0, (4, 64)),            # CSP conv1 + conv2: two convolutions in the slice table of one launch
     (256, (128, 128), "uneven", 0, 0, (4, 64)),          # ... over two cout tiles
     (128, (128,), "uneven", 128, 64, (4, 64)),           # x and y are channel slices of wider tensors
     (64, (64,), "uneven", 64, 32, (2, 128))])


def c1_geometry(K, couts, mapname):
    if mapname == "big":      # WM 4 on 128-pixel tiles needs a map that is not "small": 2 tiles per CU over the cout tiles, + 8: uneven
        f = lambda tpix, nb: -(-2 * cus() // (sum(couts) // 128)) + 8
    else:
        f = lambda tpix, nb: MAPS[mapname](nb)
    wm, tpix, nco, nb = c1_form(K, couts, f)
    return wm, tpix, nco, nb, f(tpix, nb)


def run_c1(K, couts, ntiles, tpix, xoff, yoff, nslots, stream, monkeypatch, xbuf, wfs):
    npix = ntiles * tpix
    ys, sts = [], []
    descs = (L.mi_conv_desc * len(couts))()
    for j, c in enumerate(couts):
        y = torch.full((npix, yoff + c), 7.0, dtype=torch.bfloat16, device=DEV)
        st = stats_buf(c)
        st[:nslots] = 0
        d = desc1(xbuf, xbuf.shape[1], xoff, (ntiles, tpix), K, wfs[j], y, yoff + c, yoff, c, st, nslots)
        C.memmove(C.byref(descs[j]), C.byref(d), C.sizeof(d))
        ys.append(y)
        sts.append(st)
    if stream:
        L.check(L.lib().mi_conv1x1_stream(descs, len(couts), sp()), "conv1x1_stream")
    else:
        monkeypatch.setenv("MI_CONV_STREAM", "0")
        for j in range(len(couts)):
            L.check(L.lib().mi_conv2d(C.byref(descs[j]), sp()), "conv2d")
        monkeypatch.delenv("MI_CONV_STREAM")
    torch.cuda.synchronize()
    return ys, sts


@pytest.mark.parametrize("case", C1_CASES, ids=["K%d_Co%s_%s_x%d_y%d" % (c[0], "+".join(map(str, c[1])), c[2], c[3], c[4]) for c in C1_CASES])
def test_c1s_statistics_exact(case, monkeypatch):
    K, couts, mapname, xoff, yoff, form = case
    wm, tpix, nco, nb, ntiles = c1_geometry(K, couts, mapname)
    assert (wm, tpix) == form, ("the case does not reach the form it is there for", wm, tpix)
    npix = ntiles * tpix
    x = ints((npix, K), 11 * K + ntiles)
    ws = [sparse_w(c, K, 1, 100 * K + c + j) for j, c in enumerate(couts)]
    check_premise(x, ws, -(-ntiles // min(nb, ntiles)) * tpix)
    xbuf = torch.full((npix, xoff + K), float("nan"), dtype=torch.bfloat16)
    xbuf[:, xoff:] = x.to(torch.bfloat16)
    xbuf = xbuf.to(DEV)
    wfs = [pack1(w) for w in ws]
    tile_y, _ = run_c1(K, couts, ntiles, tpix, xoff, yoff, 8, False, monkeypatch, xbuf, wfs)
    for nslots in (1, 8):
        ys, sts = run_c1(K, couts, ntiles, tpix, xoff, yoff, nslots, True, monkeypatch, xbuf, wfs)
        for j, c in enumerate(couts):
            what = (case, "conv", j, "slots", nslots)
            assert torch.equal(ys[j], tile_y[j]), (what, "y differs from the tile kernel's")
            assert bool((ys[j][:, :yoff] == 7.0).all()), (what, "channels below the output view were written")
            check_stats(sts[j], nslots, ys[j][:, yoff:], what)


# ---- XF: BatchNorm + activation of the input inside the launch, against mi_bn_act_fwd followed by the plain launch.  The
# producer's accumulators are made up so that the transform is exact: slot 0 holds (0, count) for every channel - mean 0,
# variance 1 - and eps = 0, so invstd = 1, scale = gamma in {-1, 1}, shift = beta in {-1, 0, 1}; act 0; x in [-1, 1]: |a| <= 2
@pytest.mark.parametrize("writer", [1, 0], ids=["writer", "reader"])
@pytest.mark.parametrize("K,cout,form", [(128, 128, (4, 64)), (64, 64, (2, 128))])
def test_c1s_xf_statistics_exact(K, cout, form, writer, monkeypatch):
    wm, tpix, nco, nb, ntiles = c1_geometry(K, (cout,), "uneven")
    assert (wm, tpix) == form
    npix, count, nslots = ntiles * tpix, 4096, 4
    xraw = ints((npix, K), 5 + K, hi=1)
    gamma = (ints((K,), 6, hi=1).abs() * 2 - 1) * 1.0        # +-1
    beta = ints((K,), 7, hi=1)
    a_exp = xraw * gamma + beta
    w = sparse_w(cout, K, 1, 900 + K)
    check_premise(a_exp, [w], -(-ntiles // min(nb, ntiles)) * tpix)
    wf = pack1(w)
    xr = xraw.to(DEV, torch.bfloat16)
    acc = torch.zeros(nslots, K, 2, dtype=torch.float64, device=DEV)
    acc[0, :, 1] = count
    gd, bd = gamma.to(DEV), beta.to(DEV)

    def record_buffers():
        return [torch.zeros(K, device=DEV) for _ in range(4)]        # scale, shift, mean, invstd

    # two launches: mi_bn_act_fwd, then the statistics launch on the activated tensor
    a2 = torch.full((npix, K), float("nan"), dtype=torch.bfloat16, device=DEV)
    r2 = record_buffers()
    L.check(L.lib().mi_bn_act_fwd(xr.data_ptr(), K, acc.data_ptr(), nslots, count, gd.data_ptr(), bd.data_ptr(), 0.0, 0.03, None, None,
                                  None, r2[0].data_ptr(), r2[1].data_ptr(), r2[2].data_ptr(), r2[3].data_ptr(), None, 0, a2.data_ptr(), K,
                                  npix, K, 0, sp()), "mi_bn_act_fwd")
    torch.cuda.synchronize()
    assert torch.equal(a2.float().cpu(), a_exp), "the made-up BatchNorm is not exact"
    y2, st2 = run_c1(K, (cout,), ntiles, tpix, 0, 0, 8, True, monkeypatch, a2, [wf])
    # one launch
    a1 = torch.full((npix, K), float("nan"), dtype=torch.bfloat16, device=DEV)
    r1 = record_buffers()
    rec = L.mi_bnx()
    rec.a, rec.gamma, rec.beta, rec.lda, rec.act = a1.data_ptr(), gd.data_ptr(), bd.data_ptr(), K, 0
    rec.scale, rec.shift, rec.mean, rec.invstd = [t.data_ptr() for t in r1]
    rec.inv_count, rec.unbias, rec.eps, rec.momentum = 1.0 / count, count / (count - 1.0), 0.0, 0.03
    rec.acc, rec.sld, rec.nslots, rec.C = acc.data_ptr(), 2 * K, nslots, K
    recd = torch.frombuffer(bytearray(bytes(rec)), dtype=torch.uint8).to(DEV)
    y1 = torch.full((npix, cout), 7.0, dtype=torch.bfloat16, device=DEV)
    st1 = stats_buf(cout)
    st1[:8] = 0
    d = desc1(xr, K, 0, (ntiles, tpix), K, wf, y1, cout, 0, cout, st1, 8)
    d.xf, d.xf_write, d.xf_C = recd.data_ptr(), writer, K
    L.check(L.lib().mi_conv1x1_stream(C.byref(d), 1, sp()), "conv1x1_stream (xf)")
    torch.cuda.synchronize()
    assert torch.equal(y1, y2[0]), "y differs from the two-launch form"
    check_stats(st1, 8, y1, ("xf", K, writer))
    assert torch.equal(st1[:8].sum(0), st2[0][:8].sum(0))
    if writer:
        assert torch.equal(a1, a2), "the activated tensor the writer stored differs from mi_bn_act_fwd's"
        for p, q in zip(r1, r2):
            assert torch.equal(p, q)
    else:
        assert bool(a1.isnan().all()), "a launch without xf_write stored the activated tensor"


# -------------------------------------------------------------------------------------------- weight-stationary 3x3
def desc3(x, N, H, W, K, wimg, y, cout, stride, st, nslots):
    d = L.mi_conv_desc()
    d.x, d.w, d.y = x.data_ptr(), wimg.data_ptr(), y.data_ptr()
    d.ldx, d.ldy = K, cout
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    d.N, d.H, d.W, d.outH, d.outW, d.gridH, d.gridW = N, H, W, Ho, Wo, Ho, Wo
    d.in_stride, d.out_stride = stride, 1
    d.K8, d.Cout, d.CoutPad, d.ntaps = K // 8, cout, cout, 9
    t = 0
    for r in range(3):
        for s_ in range(3):
            d.tap_dy[t], d.tap_dx[t], d.tap_w[t] = r - 1, s_ - 1, r * 3 + s_
            t += 1
    d.stats_acc, d.stats_slots = st.data_ptr(), nslots
    return d


W3_CASES = [
    # K, Cout, stride, [(N, H, W) per job of ONE launch]
    (32, 32, 1, [(2, 24, 24)]),
    (64, 64, 1, [(2, 24, 24)]),
    (128, 128, 1, [(2, 24, 24)]),
    (32, 32, 1, [(1, 8, 16)]),                            # one tile, one block
    (128, 128, 1, [(1, 13, 17)]),                         # partial tiles in both directions
    (32, 64, 2, [(2, 24, 24)]),                           # stride 2, K -> 2 K
    (64, 128, 2, [(2, 23, 21)]),
    (128, 256, 2, [(1, 24, 24)]),                         # two 128-channel jobs over one input
    (32, 32, 1, [(2, 24, 24), (1, 16, 16), (2, 13, 17)]),   # three jobs of different maps, the last with tiles partly outside
    (64, 64, 1, [(1, 24, 16), (2, 8, 16), (1, 9, 20)]),
    (128, 128, 1, [(1, 16, 16), (2, 8, 16), (1, 5, 7)]),
]


@pytest.mark.parametrize("case", W3_CASES, ids=["K%d_Co%d_s%d_%s" % (c[0], c[1], c[2], "+".join("%dx%dx%d" % j for j in c[3])) for c in W3_CASES])
def test_w3_statistics_exact(case, monkeypatch):
    K, cout, stride, jobs = case
    xs = [ints((N, H, W, K), 31 * K + H + j) for j, (N, H, W) in enumerate(jobs)]
    ws = [sparse_w(cout, K, 3, 7 * K + cout + j) for j in range(len(jobs))]
    for x, w, (N, H, W) in zip(xs, ws, jobs):
        check_premise(x, [w], N * H * W)                  # (whatever the split into blocks)
    xd = [x.to(DEV, torch.bfloat16) for x in xs]
    imgs = []
    for w in ws:
        img = torch.empty(9 * K * cout, dtype=torch.bfloat16, device=DEV)
        wd = w.to(DEV)
        L.check(L.lib().mi_pack_conv_weight(wd.data_ptr(), cout, K, 3, 3, img.data_ptr(), K, cout, None, 0, 0, sp()), "pack")
        torch.cuda.synchronize()
        imgs.append(img)

    def run(ws_on, nslots):
        ys, sts = [], []
        descs = (L.mi_conv_desc * len(jobs))()
        for j, (N, H, W) in enumerate(jobs):
            Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
            y = torch.full((N, Ho, Wo, cout), 7.0, dtype=torch.bfloat16, device=DEV)
            st = stats_buf(cout)
            st[:nslots] = 0
            d = desc3(xd[j], N, H, W, K, imgs[j], y, cout, stride, st, nslots)
            C.memmove(C.byref(descs[j]), C.byref(d), C.sizeof(d))
            ys.append(y)
            sts.append(st)
        if ws_on:
            L.check(L.lib().mi_conv3x3_ws(descs, len(jobs), sp()), "conv3x3_ws")
        else:
            monkeypatch.setenv("MI_CONV_WS", "0")
            for j in range(len(jobs)):
                L.check(L.lib().mi_conv2d(C.byref(descs[j]), sp()), "conv2d")
            monkeypatch.delenv("MI_CONV_WS")
        torch.cuda.synchronize()
        return ys, sts

    tile_y, _ = run(False, 8)
    for nslots in (1, 8):
        ys, sts = run(True, nslots)
        for j in range(len(jobs)):
            what = (case, "job", j, "slots", nslots)
            assert torch.equal(ys[j], tile_y[j]), (what, "y differs from the tile kernel's")
            check_stats(sts[j], nslots, ys[j], what)
