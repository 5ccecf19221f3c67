"""The plan of the Zstandard decoder -- rcx_plan_zstd and rcx_plan_zstd_retry in rust_compress_amd/csrc/rcx_plan.h: the persistent
waves, the scratch, the dictionary words, the size query's retry list -- driven by the stand-alone tests/host_plan/test_plan_zstd.cpp,
built with AddressSanitizer and UndefinedBehaviorSanitizer.  Host code: no GPU needed, and no kernel runs."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("host_plan_zstd") / "test_plan_zstd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall",
                           "-I", os.path.join(ROOT, "rust_compress_amd", "csrc"),
                           os.path.join(ROOT, "tests", "host_plan", "test_plan_zstd.cpp"), "-o", out])
    return out


def _run(exe, section):
    p = subprocess.run([exe, section], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "HOST_PLAN_OK " + section in p.stdout, p.stdout[-3000:] + p.stderr[-3000:]


def test_waves_literal_buffers_and_dictionary_words(exe):
    """no dictionaries, more files than waves, one range shared, a file with none, a range beyond 4 GiB kept whole; one array without the
    other, too many files, a dictionary of 4 GiB and a range that wraps are refused by name"""
    _run(exe, "plan")


def test_the_size_querys_retry_list(exe):
    """the files that reported a size, with the size, in batch order; none for an empty call"""
    _run(exe, "retry")
