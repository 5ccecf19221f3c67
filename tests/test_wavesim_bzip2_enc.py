"""The bzip2 ENCODER on the wave simulator: the unmodified kernels and launch loop of k_bzip2_enc.hip, with the suffix sorter beneath
them, give the serial reference's bytes (tests/bz2_enc_ref.py) -- and its T, L, origPtr, symbols, tables and selectors, so that a failure
names its stage."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bz2_cases as BC                                                       # noqa: E402
import bz2_enc_cases as EC                                                   # noqa: E402
import sim_bzip2_enc_run as S                                                # noqa: E402

NAMES = [c[0] for c in EC.cases()]
OK, E_TOO_SMALL = 0, 2
RC_BAD_ARG = -1


def _check_stages(got, want):
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert a["t"] == b["t"] and a["tt"] == b["t"] + b["t"], "the run-length step"
        assert a["crc"] == b["crc"], "the block CRC"
        assert a["used"] == b["used"], "the used-byte map"
        assert (a["l"], a["orig"]) == (b["l"], b["orig"]), "the rotation order"
        assert a["symbols"] == b["symbols"], "MTF and RUNA / RUNB"
        assert a["selectors"] == b["selectors"], "the fit: selectors"
        assert a["tables"] == b["tables"], "the fit: lengths"


@pytest.mark.parametrize("name", NAMES)
def test_case_equals_the_reference(name):
    _, data, level, c = EC.by_name(name)
    stream, blocks = EC.ref(name)
    r = S.run([data], [len(stream) + 9], level, c)
    assert r["rc"] == 0, r["err"]
    _check_stages(r["blocks"], blocks)
    assert r["status"][0] == OK and int(r["out_len"][0]) == len(stream) and int(r["in_used"][0]) == len(data)
    assert r["data"][0] == stream
    assert S.untouched_outside(r["out"], r["out_off"], r["out_cap"])
    assert (r["out"][int(r["out_off"][0]) + len(stream):int(r["out_off"][0]) + len(stream) + 9] == 0xEE).all()


def _small_files():
    rnd = np.random.default_rng(9)
    out = []
    for i in range(300):
        kind = i % 4
        n = int(rnd.integers(0, 60)) if i % 7 else 0
        if kind == 0:
            out.append(rnd.integers(0, 256, n, dtype=np.uint8).tobytes())
        elif kind == 1:
            out.append(bytes([65 + i % 20]) * n)
        elif kind == 2:
            out.append((b"ab" * 40)[:n])
        else:
            out.append(rnd.integers(97, 101, n, dtype=np.uint8).tobytes())
    return out


def test_many_small_files_in_one_round_and_in_rounds_of_64():
    files = _small_files()
    import bz2_enc_ref as R
    want = [R.encode(d, 4)[0] for d in files]
    one = S.run(files, [len(w) for w in want], 4, stages=False)
    assert one["rc"] == 0, one["err"]
    assert one["rounds"] == 1
    assert (one["status"] == OK).all() and one["data"] == want
    assert [int(x) for x in one["in_used"]] == [len(d) for d in files]
    assert S.untouched_outside(one["out"], one["out_off"], one["out_cap"])
    many = S.run(files, [len(w) for w in want], 4, round=64, stages=False)
    nblocks = sum(1 for d in files if d)
    assert many["rc"] == 0 and many["rounds"] == -(-nblocks // 64)
    assert many["data"] == want and (many["out"] == one["out"]).all()
    for d, w in zip(files[:40], want[:40]):
        assert BC.strict(w) == (d, len(w))


def test_rounds_inside_a_file():
    name = "many_blocks"
    _, data, level, c = EC.by_name(name)
    stream, blocks = EC.ref(name)
    for rnd in (1, 3):
        r = S.run([data, b"", data[:1000]], [len(stream), 14, 2000], level, c, round=rnd)
        assert r["rc"] == 0, r["err"]
        assert r["rounds"] == -(-(len(blocks) + 2) // rnd)
        assert r["data"][0] == stream and len(r["data"][1]) == 14
        assert BC.strict(r["data"][2]) == (data[:1000], len(r["data"][2]))
        _check_stages(r["blocks"][:len(blocks)], blocks)


def test_capacity_exact_one_less_and_zero():
    names = ("text300", "many_blocks", "run260", "empty")
    datas = [EC.by_name(x)[1] for x in names]
    import bz2_enc_ref as R
    want = [R.encode(d, 2, 700)[0] for d in datas]
    caps = [len(want[0]), len(want[1]) - 1, 0, 13]
    r = S.run(datas, caps, 2, 700, stages=False)
    assert r["rc"] == 0, r["err"]
    assert list(r["status"]) == [OK, E_TOO_SMALL, E_TOO_SMALL, E_TOO_SMALL]
    assert [int(x) for x in r["out_len"]] == [len(w) for w in want]          # the exact size, fitting or not
    assert [int(x) for x in r["in_used"]] == [len(datas[0]), 0, 0, 0]
    assert r["data"][0] == want[0]
    # nothing of a slot that is too small is written, and nothing outside any slot
    assert (r["out"][int(r["out_off"][1]):int(r["out_off"][1]) + caps[1]] == 0xEE).all()
    assert (r["out"][int(r["out_off"][3]):int(r["out_off"][3]) + caps[3]] == 0xEE).all()
    assert S.untouched_outside(r["out"], r["out_off"], r["out_cap"])
    again = S.run(datas, [len(w) for w in want], 2, 700, stages=False)
    assert (again["status"] == OK).all() and again["data"] == want


def test_refusals():
    for level in (0, 10, -1):
        r = S.run([b"abc"], [100], level, chunk=1000)
        assert r["rc"] == RC_BAD_ARG and "level" in r["err"]
        assert (r["out"] == 0xEE).all() and r["status"][0] == -1
    r = S.run([b"abc"], [100], 1, chunk=100000)                              # more than the level's blocks hold
    assert r["rc"] == RC_BAD_ARG and "chunk" in r["err"]
    r = S.run([b"abc"], [100], 1, round=5000)
    assert r["rc"] == RC_BAD_ARG and "round" in r["err"]


def test_a_call_twice_gives_identical_bytes():
    _, data, level, c = EC.by_name("words3000")
    a = S.run([data, data[:77]], [3000, 200], level, c, stages=False)
    b = S.run([data, data[:77]], [3000, 200], level, c, stages=False)
    assert a["rc"] == 0 and a["data"] == b["data"] and (a["out"] == b["out"]).all()
