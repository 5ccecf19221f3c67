"""The planning arithmetic of dictionary training -- the argument checks, the epochs, the round bound, the kernels' words and the scratch
carve (rcx_plan_train and the constexpr functions beside it in rust_compress_amd/csrc/rcx_plan.h, which the kernels call too) -- driven by
the stand-alone tests/host_plan/test_plan_train.cpp, built with AddressSanitizer and UndefinedBehaviorSanitizer.  Host code: no GPU
needed, and no kernel runs."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("host_plan_train") / "test_plan_train")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall",
                           "-I", os.path.join(ROOT, "rust_compress_amd", "csrc"),
                           os.path.join(ROOT, "tests", "host_plan", "test_plan_train.cpp"), "-o", out])
    return out


def _run(exe, section):
    p = subprocess.run([exe, section], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "HOST_PLAN_OK " + section in p.stdout, p.stdout[-3000:] + p.stderr[-3000:]


def test_epoch_arithmetic_and_the_kernels_words(exe):
    """n = 0, n < k, n = k, epochs of n / E with a remainder, the 10 k branch, the largest corpus; dead jobs; the round bound; the
    headers and sample ends of a three-job plan with an empty sample and a job without samples; a call without jobs."""
    _run(exe, "epochs")


def test_refusals_name_the_job(exe):
    """d = 7, k < d, k = 4097, f = 9 and 23, each null array, sample lengths that fall short, overshoot or would wrap, a corpus or a
    capacity of 2^32 (arithmetic only); the largest corpus there is still plans."""
    _run(exe, "refuse")


def test_scratch_carve(exe):
    """For 200 random batches (1 .. 300 jobs, dead ones among them, k 6 .. 4096, f 10 .. 22) at four alignments of the caller's
    pointer: the head and every array of every live job lie inside plan.scratch_bytes, regions follow each other without overlap, and
    rcx_dict_train_scratch_bytes with every job at the largest sizes is no smaller."""
    _run(exe, "carve")
