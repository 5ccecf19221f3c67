"""The planning arithmetic of the host-descriptor batch path (rust_compress_amd/csrc/rcx_plan.h, what run_batch in rcx_api.hip
plans with): span limits, the input ranges of a gated launch, the chains of a linked LZ4 batch, what travels back.  Pure integer
code, driven by tests/host_plan/test_plan.cpp.  Host code: no GPU needed."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("host_plan") / "test_plan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "rust_compress_amd", "csrc"),
                           os.path.join(ROOT, "tests", "host_plan", "test_plan.cpp"), "-o", out])
    return out


def _run(exe, section):
    p = subprocess.run([exe, section], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "HOST_PLAN_OK " + section in p.stdout, p.stdout[-3000:] + p.stderr[-3000:]


def test_span_check(exe):
    """A block of 2^32 - 1 bytes passes and one of 2^32 does not; an off + len that wraps is refused by its block's number; the
    spans and the longest block are what the descriptors say."""
    _run(exe, "spans")


def test_range_plan(exe):
    """The boundaries of 255 / 256 / 700 / 4096 blocks under the default knobs, the knobs' caps, and over 300 seeded batches (up to
    5000 blocks, empty ones among them, ragged offsets, blocks in order, reversed and dealt out of order): every block in one range,
    every non-empty block inside its range's bytes, the bytes cut at 256-byte lines or the end of the span, and one range
    exactly when more than in_span + in_span / 4 bytes would move or the ranges' spans do not ascend."""
    _run(exe, "ranges")


def test_reversed_block_order_takes_one_range(exe):
    """Blocks listed in reverse input order fall back to one range: consecutive blocks of such a batch still lie side by side in
    the input, so the ranges' byte spans do not overlap and move hardly more than in_span -- it is the spans starting ever lower,
    range after range, that sends the batch back to one copy in front of the launch.  20 seeded batches of 817 .. 4421 blocks;
    the driver prints every batch's figures."""
    _run(exe, "reversed")


def test_chain_plan(exe):
    """head / depth of hand-written link patterns and 200 random ones; order a permutation by depth, by index within a depth;
    rounds_off its partition; block 0 cannot continue a chain; a dictionary reaches no lower than out_base and counts 65536 bytes
    at the most."""
    _run(exe, "chains")


def test_copy_back_ranges(exe):
    """The used span of the plain path; the linked decoder's copies: ascending, disjoint, touching chains as one, a chain's sum
    capped at its head's slot, empty chains skipped -- the union is every chain's bytes, counted one by one."""
    _run(exe, "copies")
