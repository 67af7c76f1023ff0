"""The YOLOX loss call through the C ABI and the three SimOTA inputs whose outputs tests/golden/simota_round5_record.npz
holds: shared by tests/test_gpu_step.py and tools/record_simota_outputs.py, so that both build identical tensors."""
import ctypes as C
import hashlib

import numpy as np
import torch

import yolox_oracle as O
from yolov7_d2_amd import _lib as L

DEV = "cuda"
RECORD = "simota_round5_record.npz"
RECORD_WORDS = ("ngt", "fg", "matched_gt", "matched_iou", "out")      # kept in full (fg bit-packed)
RECORD_DIGESTS = ("cost", "iou", "dpreds")                            # tens of MB each: kept as SHA-256 of their bytes


def loss_call(raw, labels, anchors, gw=(1, 1, 1, 1), gmax=None, use_l1=False):
    B, A, nch = raw.shape
    ML = labels.shape[1]
    gmax = ML if gmax is None else gmax
    t = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=DEV)
    ws = dict(cost=t(B, gmax, A), iou=t(B, gmax, A), match=t(B, gmax, A, dt=torch.uint8), ngt=t(B, dt=torch.int32),
              fg=t(B, A, dt=torch.uint8), matched_gt=t(B, A, dt=torch.int32), matched_iou=t(B, A),
              partial=t(B * ((A + 255) // 256), 4), out=t(8), dpreds=t(B, A, nch),
              partial_l1=t(B * ((A + 255) // 256)), gw=torch.tensor(gw, dtype=torch.float32, device=DEV))
    rd, ld, ad = raw.to(DEV).contiguous(), labels.to(DEV).contiguous(), anchors.to(DEV).contiguous()
    d = L.mi_yolox_loss_desc()
    d.preds, d.labels, d.anchors = rd.data_ptr(), ld.data_ptr(), ad.data_ptr()
    d.B, d.A, d.ncls, d.max_labels, d.gmax = B, A, nch - 5, ML, gmax
    for k in ("cost", "iou", "match", "ngt", "fg", "matched_gt", "matched_iou", "partial", "out"):
        setattr(d, k, ws[k].data_ptr())
    if use_l1:
        d.use_l1, d.partial_l1 = 1, ws["partial_l1"].data_ptr()
    L.check(L.lib().mi_yolox_loss_fwd(C.byref(d), L.stream_ptr()), "loss_fwd")
    L.check(L.lib().mi_yolox_loss_bwd(C.byref(d), ws["gw"].data_ptr(), ws["dpreds"].data_ptr(), L.stream_ptr()), "loss_bwd")
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in ws.items()}


def record_cases():
    """[(name, raw, labels, anchors, loss_call keywords)]: the bench-size batch; exact ties everywhere with lists that overflow
    the LDS capacity (the block-wide rounds take over); <= 9 candidates on 2 100 anchors (NV = 9) with use_l1"""
    B, H, W = 16, 640, 640
    _, labels = O.synth_batch(B, H, W, seed=1234, max_gt=20)
    hw = [(H // s, W // s) for s in (8, 16, 32)]
    raw, anchors = O.synth_raw(B, hw, 35, labels=labels)
    cases = [("bench", raw, labels, anchors, {})]
    # exact ties everywhere: constant predictions (equal IoU along rows / columns of the grid, equal class terms), one huge
    # box per image so that thousands of anchors are candidates of equal cost: the lists overflow -> fallback path
    raw0 = torch.zeros(2, anchors.shape[0], 85)
    lab0 = torch.zeros(2, 100, 5)
    lab0[0, 0] = torch.tensor([3.0, 320, 320, 600, 600])
    lab0[0, 1] = torch.tensor([7.0, 100, 100, 64, 64])
    lab0[1, 0] = torch.tensor([1.0, 320, 320, 16, 16])
    cases.append(("ties", raw0, lab0, anchors, {}))
    # few candidates (a 4-pixel box: only its centre-radius anchors) and the small-map instantiation (NV = 9)
    hw2 = [(40, 40), (20, 20), (10, 10)]
    anchors2 = O.make_anchors(hw2)
    _, lab2 = O.synth_batch(3, 320, 320, seed=5, max_gt=8)
    lab2[2] = 0.0
    lab2[2, 0] = torch.tensor([2.0, 7, 9, 4, 4])
    raw2, _ = O.synth_raw(3, hw2, 36, labels=lab2)
    cases.append(("small", raw2, lab2, anchors2, dict(use_l1=True, gw=(1, 1, 1, 1, 1))))
    return cases


def record_of(ws):
    """what the record keeps of one loss_call result: {key: numpy array}"""
    rec = {k: ws[k].numpy() for k in RECORD_WORDS}
    rec["fg"] = np.packbits(rec["fg"].reshape(-1))
    for k in RECORD_DIGESTS:
        rec["sha256_" + k] = np.frombuffer(hashlib.sha256(ws[k].contiguous().numpy().tobytes()).digest(), dtype=np.uint8)
    return rec
