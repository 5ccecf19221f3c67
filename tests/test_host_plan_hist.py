"""The planning arithmetic of the DEFLATE calls with history -- the argument checks and aux words (rcx_plan_hist of
rust_compress_amd/csrc/rcx_plan.h) and the scratch carve with its history slots (dh_hist_scratch_bytes / dh_hist_carve of
k_deflate_hc_hist.hip) -- driven by the stand-alone tests/host_plan/test_plan_hist.cpp, built with AddressSanitizer and
UndefinedBehaviorSanitizer.  Host code: no GPU needed, and no kernel runs."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("host_plan_hist") / "test_plan_hist")
    ws = os.path.join(ROOT, "tests", "wavesim")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-x", "c++",
                           "-include", os.path.join(ws, "wavesim.h"), "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas",
                           "-Wno-unused-variable", "-Wno-attributes", "-I", os.path.join(ROOT, "rust_compress_amd", "csrc"),
                           os.path.join(ROOT, "tests", "host_plan", "test_plan_hist.cpp"), os.path.join(ws, "wavesim.cpp"), "-o", out])
    return out


def _run(exe, section):
    p = subprocess.run([exe, section], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "HOST_PLAN_OK " + section in p.stdout, p.stdout[-3000:] + p.stderr[-3000:]


def test_history_arguments(exe):
    """hist_len beyond 32768, beyond the offset in front of the block, beyond 32 bits: refused by the block's number, with the
    caller's prefix; the aux words are the lengths, then the DICTIDs; nhist counts the blocks with a history."""
    _run(exe, "args")


def test_history_slots(exe):
    """For 1 .. 8212 blocks of 0 .. 3 segments with no, one or every block with a history, at four alignments of the scratch: the
    carve's arrays lie inside dh_hist_scratch_bytes, in ascending order without overlap, the link array last and longer by one
    segment per history; a scratch below the fixed part holds no segment."""
    _run(exe, "slots")
