"""Data-parallel gradient exchange for the YOLOX step: bucketed all-reduce(mean) of the flat gradient
arena over RCCL (torch.distributed backend "nccl" on ROCm = RCCL over xGMI), overlapped with backward.

Replaces detectron2's create_ddp_model / torch DistributedDataParallel as reached from
train_det.py:73 (DefaultTrainer.__init__) — d2 upstream, un-vendored.  The path is pure data parallel
(SURVEY.md §8e): every rank runs the whole model on its own images; the only exchange is the
gradient all-reduce (8.97 M fp32 = 35.9 MB for YOLOX-s) plus one parameter broadcast at start.

MI355X design: gradients already live in ONE contiguous fp32 arena (params.ParamArena) in parameter
order, so a bucket is a plain slice — no flatten/unflatten copies and no per-parameter hooks.  The
backward command list is cut where a bucket's last gradient has been written; each cut launches that
bucket's all-reduce while the remaining backward keeps the compute stream busy.  On the 8-GPU xGMI
mesh the message is bandwidth-trivial (35.9 MB ~ 0.1-0.4 ms): what matters is starting early and using
few, large messages, hence 2-4 buckets rather than PyTorch's 25 MiB default policy tuned for NVSwitch.
"""
import ctypes as C

import torch
import torch.distributed as dist

from . import _lib as L


def grad_write_ranges(plan, grad_tensor):
    """for every backward command: list of (byte_lo, byte_hi) it writes inside the flat gradient arena"""
    base = grad_tensor.data_ptr()
    end = base + grad_tensor.numel() * 4
    arr, n = plan.bwd_cmds
    out = []
    for k in range(n):
        c = arr[k]
        ptrs = []
        if c.op == L.OP["WGRAD"]:
            d = C.cast(c.p[0], C.POINTER(L.mi_wgrad_desc)).contents
            ptrs.append((d.gw, d.ntaps * d.Cout * d.Cin * 4))
        elif c.op == L.OP["WGRAD_GROUP"]:
            for d in plan.cmd_descs["bwd"][k]:
                ptrs.append((d.gw, d.ntaps * d.Cout * d.Cin * 4))
        elif c.op in (L.OP["BN_BWD_APPLY"], L.OP["BN_BWD_FUSED"]):
            ptrs += [(c.p[8], c.i[5] * 4), (c.p[9], c.i[5] * 4)]
        elif c.op == L.OP["BN_GROUP"] and c.i[0] in (2, 3):
            for j in plan.cmd_descs["bwd"][k]:
                ptrs += [(j.dgamma, j.C * 4), (j.dbeta, j.C * 4)]
        elif c.op == L.OP["DWCONV_WGRAD"]:
            ptrs.append((c.p[3], c.i[5] * 9 * 4))
        elif c.op == L.OP["COLSUM"]:
            ptrs.append((c.p[1], c.i[1] * 4))
        elif c.op == L.OP["BIAS_GRADS"]:
            jobs = C.cast(c.p[0], C.POINTER(L.mi_bias_job))
            for j in range(c.i[3]):
                ptrs.append((jobs[j].out, jobs[j].nc * 4))
        elif c.op == L.OP["LOSS_BWD_FUSED"]:
            jobs = C.cast(c.p[4], C.POINTER(L.mi_bias_job))
            for j in range(c.i[1]):
                ptrs.append((jobs[j].out, jobs[j].nc * 4))
        elif c.op == L.OP["MEMSET"]:
            ptrs.append((c.p[0], c.l[0]))
        rs = []
        for p, nb in ptrs:
            if p is not None and base <= p < end:
                rs.append((p - base, p - base + nb))
        out.append(rs)
    return out


def plan_buckets(total_elems, writes, n_buckets, bounds=None):
    """split [0,total) into n contiguous buckets (element ranges; equal parts, or the given interior `bounds`) and
    return, per bucket, the index of the LAST backward command that writes into it: [(lo, hi, last_cmd)], ordered by
    completion time."""
    if bounds:
        bounds = [0] + sorted(int(b) // 4 * 4 for b in bounds if 0 < b < total_elems) + [total_elems]
        n_buckets = len(bounds) - 1
    else:
        n_buckets = max(1, min(n_buckets, total_elems))
        bounds = [total_elems * i // n_buckets for i in range(n_buckets + 1)]
        bounds = [b // 4 * 4 for b in bounds[:-1]] + [total_elems]
    res = []
    for i in range(n_buckets):
        lo, hi = bounds[i], bounds[i + 1]
        last = -1
        for k, rs in enumerate(writes):
            for (b0, b1) in rs:
                if b0 < hi * 4 and lo * 4 < b1:
                    last = k
        res.append((lo, hi, last))
    res.sort(key=lambda t: t[2])
    return res


class GradReducer:
    """all-reduce(sum) of flat-gradient buckets, launched as soon as each bucket is complete; the 1/world
    scaling is folded into the optimizer update (grad_scale)."""

    def __init__(self, grad, buckets, group=None):
        self.grad, self.buckets, self.group = grad, buckets, group
        self.world = dist.get_world_size(group) if dist.is_initialized() else 1
        self.pending = []
        self.enabled = True      # False: skip the collectives (bench.py measures the exposed communication time that way)

    def segments(self, n_cmds):
        """[(cmd_lo, cmd_hi, bucket or None)]: run cmds [lo,hi) then reduce the bucket"""
        segs, prev = [], 0
        for (lo, hi, last) in self.buckets:
            cut = max(prev, last + 1)
            segs.append((prev, cut, (lo, hi)))
            prev = cut
        if prev < n_cmds:
            segs.append((prev, n_cmds, None))
        return segs

    def reduce_bucket(self, bucket):
        if self.world == 1 or bucket is None or not self.enabled:
            return
        lo, hi = bucket
        self.pending.append(dist.all_reduce(self.grad[lo:hi], op=dist.ReduceOp.SUM, group=self.group, async_op=True))

    def wait(self):
        for w in self.pending:
            w.wait()
        self.pending = []


def broadcast_params(flat_params, src=0, group=None):
    """rank-0 parameter broadcast at construction (DDP semantics); BN buffers are NOT synchronised
    (create_ddp_model(broadcast_buffers=False))."""
    if dist.is_initialized() and dist.get_world_size(group) > 1:
        dist.broadcast(flat_params, src=src, group=group)
