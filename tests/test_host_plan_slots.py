"""The planning arithmetic of the decoders behind shared dictionaries -- what travels back to a host-memory batch (rcx_plan_slot_copies
of rust_compress_amd/csrc/rcx_plan.h) and the words of rcx_plan_dict that the decoders read -- driven by the stand-alone
tests/host_plan/test_plan_slots.cpp, built with AddressSanitizer and UndefinedBehaviorSanitizer.  Host code: no GPU needed, and no
kernel runs."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("host_plan_slots") / "test_plan_slots")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall",
                           "-I", os.path.join(ROOT, "rust_compress_amd", "csrc"),
                           os.path.join(ROOT, "tests", "host_plan", "test_plan_slots.cpp"), "-o", out])
    return out


def _run(exe, section):
    p = subprocess.run([exe, section], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "HOST_PLAN_OK " + section in p.stdout, p.stdout[-3000:] + p.stderr[-3000:]


def test_only_what_the_blocks_produced_travels_back(exe):
    """Contiguous full slots are one copy; a gap, a failed block or a short block ends a range; no byte between the slots or beyond a
    slot's capacity is covered, every produced byte is, once (random layouts against a map of the buffer)."""
    _run(exe, "copies")


def test_the_words_the_decoders_read(exe):
    """The clamped length (LZ4: 65536 counts as 65535 and the offset moves with it), the offset's two words, the DICTIDs, the span that
    travels in; one byte over the limit is refused by the block's number behind the caller's prefix."""
    _run(exe, "words")


def test_which_layouts_take_the_single_span_copy(exe):
    """rcx_plan_out_dense: fixed slots that tile the buffer are dense in any order; a byte in front of the first slot, padding between
    slots or a one-byte gap is not; 2000 random layouts (gaps, overlaps, empty slots, shuffled) against a byte map of the buffer."""
    _run(exe, "dense")
