"""GPU (-m gpu): the chain between the two phases of the one-launch BatchNorm backward (csrc/bn_act.hip bn_bwd_fused_body,
csrc/bn_barrier.h) - rotated block sums, the arrival tree, the last block's 16-byte fold and hand-back, one release lane
per group, phase 2's constants kept across the barrier - on the exact families of tests/bn_ref.py, with NO tolerance, and
under the hygiene of tests/test_gpu_bn_exact.py, whose job classes this file drives (imported, not edited).

Grids, pinned through mi_bn_fused_set_capacity: 1, 2, one below / at / one above both fan-in boundaries of the two-level
arrival tree (16 blocks: the groups get a second member; 32: every group has two), and the device's capacity.  Channels:
C = 8 (one channel group, 256 pixel lanes), 24 (255 working threads), 64, 2048 (one pixel lane, eight trips of every
c += 256 loop; the rotation wraps).  Items per thread 0, 1, 14, 15, 19 among others (the retained / streamed boundary at 14,
the four-wide and two-wide streaming tails).  dres absent / written / accumulated, dgamma and dbeta NULL.  Eight launches
on one barrier record that is never re-zeroed; the same launch captured in a hipGraph and replayed three times; three
jobs in one grouped launch under a third of the capacity they ask for.  After EVERY launch: dy, dres, dgamma, dbeta exactly,
the folded totals in slot 0 with the NaN pattern of the unused slots and pad channels intact, and the barrier record."""
import types

import pytest
import torch

import bn_ref as R
import test_gpu_bn_exact as E
from yolov7_d2_amd import _lib as L

pytestmark = pytest.mark.gpu
B = R.BwdCase


def chain_cases():
    """name C npix nslots k act dres lds nblk cap nodg seed; npix = nb * PL * m + r gives the threads m or m + 1 items"""
    return [
        B("k-c64-n5-nb1", 64, 5, 3, 4, 0, 1, (64, 72, 80, 88), 1, 1, False, 51),                          # items 0, 1
        B("k-c8-nb2", 8, 2 * 256 * 14 + 100, 16, 8, "sat", 2, (16, 24, 8, 32), 1, 2, False, 52),          # 14, 15
        B("k-c24-nb15", 24, 15 * 85 * 18 + 700, 5, 8, 0, 0, (40, 24, 32, 0), 1, 15, True, 53),            # 18, 19
        B("k-c64-nb16", 64, 16 * 32 * 14 + 40, 16, 8, "sat", 1, (72, 64, 80, 96), 1, 16, False, 54),      # 14, 15
        B("k-c2048-nb17", 2048, 17 * 14 + 5, 1, 8, 0, 2, (2056, 2064, 2048, 2072), 1, 17, False, 55),     # 14, 15
        B("k-c64-nb31", 64, 31 * 32 * 5 + 17, 3, 8, 0, 2, (64, 80, 72, 88), 1, 31, False, 56),
        B("k-c24-nb32", 24, 32 * 85 * 4 + 33, 16, 8, "sat", 0, (24, 32, 48, 0), 1, 32, False, 57),
        B("k-c8-nb33", 8, 33 * 256 * 4 + 77, 2, 8, 0, 1, (8, 16, 24, 32), 1, 33, True, 58),
        B("k-c2048-nb33", 2048, 33 * 19 + 3, 16, 8, "sat", 2, (2048, 2056, 2064, 2072), 1, 33, False, 59),  # 19, 20
    ]


def capacity_cases(hw):
    """the whole device: every block of the launch resident, every group of the tree full"""
    return [B("k-c2048-cap", 2048, hw * 4 + 3, 16, 8, 0, 1, (2048, 2056, 2064, 2072), 1, 0, False, 61),
            B("k-c64-cap", 64, hw * 32 * 4 + 19, 16, 4, "sat", 2, (64, 72, 80, 88), 1, 0, False, 62)]


def test_cases_reach_the_grids_and_item_counts():
    """the grids the cases pin and the item counts their threads hold (no launch)"""
    stats = dict(nb=set(), items=set())
    try:
        for c in chain_cases():
            assert E.effective_capacity(c.cap) == c.cap
            nb = R.fused_blocks(c.npix, c.C, c.cap)
            stats["nb"].add(nb)
            stats["items"] |= R.nmine_set(c.npix, c.C, nb)
        hw = E.effective_capacity(0)
        for c in capacity_cases(hw):
            assert R.fused_blocks(c.npix, c.C, hw) == hw
    finally:
        L.lib().mi_bn_fused_set_capacity(0)
    assert stats["nb"] == {1, 2, 15, 16, 17, 31, 32, 33} and stats["items"] >= {0, 1, 14, 15, 19}, stats


@pytest.mark.parametrize("c", chain_cases(), ids=lambda c: c.name)
def test_chain_exact_on_pinned_grids(c):
    """three launches on one record, everything refilled and checked every time"""
    bad = E.run_fused_case(c)
    assert bad == [], bad[:10]


def test_chain_exact_at_device_capacity():
    hw = E.effective_capacity(0)
    for c in capacity_cases(hw):
        bad = E.run_fused_case(c)
        assert bad == [], bad[:10]


def test_eight_launches_on_one_record():
    """the record is zeroed once: after launch i the generation words hold i, every counter is back at zero"""
    c = B("k-c64-nb33-x8", 64, 33 * 32 * 6 + 21, 16, 8, 0, 2, (64, 80, 72, 88), 1, 33, False, 63)
    job = E.make_bwd_job(c)
    bad = []
    try:
        cap = E.effective_capacity(c.cap)
        nb = R.fused_blocks(c.npix, c.C, cap)
        assert nb == 33
        for i in range(8):
            job.refill()
            job.fused()
            bad += job.check("launch %d" % (i + 1)) + job.check_sums("fused", folded=True) + job.check_barrier([nb] * (i + 1))
    finally:
        L.lib().mi_bn_fused_set_capacity(0)
    assert bad == [], bad[:10]


def test_captured_launch_replayed():
    """the launch captured in a hipGraph (as the step plan runs it) and replayed three times on the record the eager warm-up
    launch left: outputs, totals and record after each replay"""
    c = B("k-c24-nb17-graph", 24, 17 * 85 * 15 + 60, 16, 8, "sat", 1, (40, 24, 32, 48), 1, 17, False, 64)
    job = E.make_bwd_job(c)
    bad = []
    try:
        cap = E.effective_capacity(c.cap)
        nb = R.fused_blocks(c.npix, c.C, cap)
        assert nb == 17

        def launch():
            L.check(L.lib().mi_bn_act_bwd_fused(*job.head(), job.gamma.ptr, job.dacc.ptr, c.nslots, job.o.count, *job.tail(),
                                                job.bar.ptr, E.sp()), "fused")
        job.refill()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            launch()                                   # warm-up on the capture stream
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        bad += job.check("eager") + job.check_barrier([nb])
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            launch()
        for i in range(3):
            job.refill()
            torch.cuda.synchronize()
            graph.replay()
            torch.cuda.synchronize()
            E.SEEN[R.kernel_name("bn_bwd_fused", c.act)] += 1
            bad += job.check("replay %d" % (i + 1)) + job.check_sums("fused", folded=True) + job.check_barrier([nb] * (i + 2))
    finally:
        L.lib().mi_bn_fused_set_capacity(0)
    assert bad == [], bad[:10]


@pytest.mark.parametrize("act", [0, "sat"], ids=["act0", "sat"])
def test_grouped_launch_shares_a_third_of_the_capacity(act):
    """three jobs (C = 8, 64, 2048) in one launch under a third of the blocks they ask for: two launches, every job exact, its
    own record"""
    jobs = [B("k-g0-%s" % act, 8, 9000, 16, 8, act, 2, (16, 24, 8, 32), 1, 0, False, 71),
            B("k-g1-%s" % act, 64, 3000, 3, 8, act, 0, (64, 72, 80, 0), 1, 0, True, 72),
            B("k-g2-%s" % act, 2048, 150, 16, 8, act, 1, (2048, 2056, 2064, 2072), 1, 0, False, 73)]
    bad = E.run_group_case(types.SimpleNamespace(kind=3, n=3, act=act, jobs=jobs))
    assert bad == [], bad[:10]
