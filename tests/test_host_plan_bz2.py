"""The chain plan of the bzip2 decoder -- rcx_plan_bz2_chain in rust_compress_amd/csrc/rcx_plan.h, which strings the scan's candidates
and the speculative block decodes into validated streams -- driven by the stand-alone tests/host_plan/test_plan_bz2.cpp, built with
AddressSanitizer and UndefinedBehaviorSanitizer.  Host code: no GPU needed, and no kernel runs."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("host_plan_bz2") / "test_plan_bz2")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall",
                           "-I", os.path.join(ROOT, "rust_compress_amd", "csrc"),
                           os.path.join(ROOT, "tests", "host_plan", "test_plan_bz2.cpp"), "-o", out])
    return out


def _run(exe, section):
    p = subprocess.run([exe, section], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "HOST_PLAN_OK " + section in p.stdout, p.stdout[-3000:] + p.stderr[-3000:]


def test_chains_against_expected_results(exe):
    """a candidate off the chain (failed and decoded), a gap, an overlap, a block over its stream's level and one exactly at it, two
    streams with different levels, trailing bytes, a header with nothing behind it, a missing stream end, an end mark cut off, a wrong
    combined CRC, zero blocks, the magic, short files, a block's own failure in stream order, a block that makes no progress"""
    _run(exe, "chain")


def test_records_that_arrive_in_rounds(exe):
    """the same walks with the blocks' records made available one, two and three candidates at a time (the others poisoned): the same
    status, in_used and live blocks"""
    _run(exe, "rounds")
