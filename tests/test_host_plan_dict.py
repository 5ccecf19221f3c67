"""The planning arithmetic of the encoders behind shared dictionaries -- the argument checks, the clamp, the deduplication and the
kernels' words (rcx_plan_dict of rust_compress_amd/csrc/rcx_plan.h) and the scratch carve with the dictionaries' tables in front
(hc_dict_scratch_bytes / dh_dict_scratch_bytes, lzd_carve of lz_dict.h) -- driven by the stand-alone tests/host_plan/test_plan_dict.cpp,
built with AddressSanitizer and UndefinedBehaviorSanitizer.  Host code: no GPU needed, and no kernel runs."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("host_plan_dict") / "test_plan_dict")
    ws = os.path.join(ROOT, "tests", "wavesim")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-x", "c++",
                           "-include", os.path.join(ws, "wavesim.h"), "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas",
                           "-Wno-unused-variable", "-Wno-attributes", "-I", os.path.join(ROOT, "rust_compress_amd", "csrc"),
                           os.path.join(ROOT, "tests", "host_plan", "test_plan_dict.cpp"), os.path.join(ws, "wavesim.cpp"), "-o", out])
    return out


def _run(exe, section):
    p = subprocess.run([exe, section], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "HOST_PLAN_OK " + section in p.stdout, p.stdout[-3000:] + p.stderr[-3000:]


def test_dictionary_arguments(exe):
    """Lengths beyond the format's largest and ranges that wrap are refused by the block's number, behind the caller's prefix; a
    dictionary is clamped to the bytes within reach BEFORE ranges are compared; equal ranges are one dictionary, ranges that overlap
    but differ are two; an offset without a length is ignored; n = 0 reads nothing; the words are laid out as csrc/lz_dict.h reads
    them."""
    _run(exe, "plan")


def test_scratch_carve_and_what_dictionaries_cost(exe):
    """For 1 .. 8212 blocks of 0 .. 2 segments with 0 .. 64 distinct dictionaries, at four alignments of the scratch, for both families:
    every array of the carve lies inside *_dict_scratch_bytes; and the scratch beyond the encoder without history is at most 256 KiB
    per distinct dictionary + 32 bytes per block + 4 KiB (the history calls add 128 KiB per block)."""
    _run(exe, "carve")
