"""The word protocol of the one-launch BatchNorm backward's grid barrier (yolov7_d2_amd/csrc/bn_barrier.h) on the CPU, before
any GPU sees it: tests/native/bn_barrier_host.cpp instantiates the header the kernel uses with std::atomic_ref and one
std::thread per block - 1, 2, 15, 16, 17, 33, 257 and 512 blocks, 64 launches on one record each - and checks the last-arriver
detection, that nobody is released early, that every thread sees every release exactly once, and the end state against the
rule of tests/bn_ref.py::barrier_expected.  Built plainly and once more with -fsanitize=thread (a stand-alone program: nothing
is preloaded)."""
import os
import shutil
import subprocess

import pytest

import bn_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "bn_barrier_host.cpp")
COUNTS = (1, 2, 15, 16, 17, 33, 257, 512)


def test_the_header_states_the_layout_of_the_reference():
    """BNB_G / BNB_WORDS / the flag word of bn_barrier.h are the constants of tests/bn_ref.py (which mirror include/mi355_det.h;
    conv_bn.h asserts the same against that header at compile time)"""
    text = open(os.path.join(ROOT, "yolov7_d2_amd", "csrc", "bn_barrier.h")).read()
    assert "#define BNB_G %d\n" % R.BAR_G in text
    assert "#define BNB_WORDS (64 * (1 + 2 * BNB_G))" in text and R.BAR_WORDS == 64 * (1 + 2 * R.BAR_G)
    assert "#define BNB_FLAG 2\n" in text


@pytest.mark.parametrize("flags", [(), ("-fsanitize=thread", "-g")], ids=["plain", "tsan"])
def test_barrier_protocol_on_host_threads(flags, tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "bn_barrier_host")
    subprocess.run(["g++", "-std=c++20", "-O2", "-pthread", *flags, "-o", exe, SRC], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "WARNING: ThreadSanitizer" not in r.stderr, (r.stdout[-2000:], r.stderr[-2000:])
    for nb in COUNTS:
        assert "nb %3d: ok" % nb in r.stdout
