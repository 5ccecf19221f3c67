"""The host plan of the bzip2 encoder -- rcx_plan_bz2e_chunks, _step, _less, _cut, _rounds, _layout and _block_bound in
rust_compress_amd/csrc/rcx_plan.h: the cut of a file into blocks, the blocks' bit offsets, the combined CRC, the sizes against the
capacities -- driven by the stand-alone tests/host_plan/test_plan_bz2_enc.cpp, built with AddressSanitizer and
UndefinedBehaviorSanitizer.  Host code: no GPU needed, and no kernel runs."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("host_plan_bz2_enc") / "test_plan_bz2_enc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall",
                           "-I", os.path.join(ROOT, "rust_compress_amd", "csrc"),
                           os.path.join(ROOT, "tests", "host_plan", "test_plan_bz2_enc.cpp"), "-o", out])
    return out


def _run(exe, section):
    p = subprocess.run([exe, section], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "HOST_PLAN_OK " + section in p.stdout, p.stdout[-3000:] + p.stderr[-3000:]


def test_pieces_chunk_lengths_and_cuts_at_the_boundaries(exe):
    """len = C, C + 1 and 2C, empty files between others, a form of C + 1, a last chunk of one byte, the real block size, a file of
    4 GiB"""
    _run(exe, "chunks")


def test_bit_offsets_padding_combined_crc_and_capacities(exe):
    _run(exe, "layout")


def test_rounds_of_one_two_and_three_blocks_give_the_same_plan(exe):
    _run(exe, "rounds")
