"""The Zstandard decoder (rust_compress_amd/csrc/k_zstd.hip with k_xxh64.hip, UNMODIFIED) and the host's rcx_plan_zstd on the wave64
simulator, against tests/zstd_ref.py: every named and crafted input in one call with slots of exactly the decoded size, the statuses by
name, the size query and the exact retry, the dictionary cases, the 200 single-bit flips, guard bytes around every slot; the edge cases (zstd_cases.edge_cases(), golden_more())
in both executors and on two waves, persistent waves over files that would show what the file before left, the capacity sweep, the 600
mutations.  Every malformed input runs to completion.  CPU only."""
import numpy as np
import pytest

import sim_zstd_run as S
import zstd_cases as Z
import zstd_ref as R


def _cases():
    return [dict(name=g["name"], blob=g["blob"], dict=g["dict"]) for g in Z.golden()] + \
           [dict(name=c["name"], blob=c["blob"], dict=c["dict"]) for c in Z.crafted()]


def check(cases, r, caps=None):
    """every file's status, out_len, in_used and bytes are the reference's for the capacity it had"""
    assert r["rc"] == 0, r["err"]
    for i, c in enumerate(cases):
        cap = None if caps is None else caps[i]
        st, data, out_len, used = R.outcome(c["blob"], c["dict"] or b"", cap) if cap is not None else Z.expected(c["blob"], c["dict"])
        got = (int(r["status"][i]), int(r["out_len"][i]), int(r["in_used"][i]))
        assert got == (R.STATUS[st], out_len, used), (c["name"], got, st, out_len, used)
        if st == "OK":
            assert r["data"][i] == data, c["name"]
    assert S.untouched_outside(r["out"], r["out_off"], r["out_cap"])


@pytest.fixture(scope="module")
def everything():
    cases = _cases()
    caps = [Z.expected(c["blob"], c["dict"])[2] if Z.expected(c["blob"], c["dict"])[0] == "OK" else 64 for c in cases]   # (a failing file: any slot)
    return cases, caps, S.run([c["blob"] for c in cases], caps, [c["dict"] for c in cases])


def test_every_named_and_crafted_input_in_exact_slots(everything):
    cases, caps, r = everything
    assert r["waves"] == len(cases) and r["scratch"] == len(cases) * (131072 + 64)
    check(cases, r, caps)
    assert sum(1 for c in cases if Z.expected(c["blob"], c["dict"])[0] == "OK") >= 30


def test_statuses_by_name(everything):
    cases, caps, r = everything
    by_name = {c["name"]: int(r["status"][i]) for i, c in enumerate(cases)}
    want = {c["name"]: R.STATUS[c["status"]] for c in Z.crafted()}
    assert {k: by_name[k] for k in want} == want
    for st in ("E_EOF", "E_ZSTD_MAGIC", "E_ZSTD_HEADER", "E_ZSTD_DATA", "E_ZSTD_CHECKSUM", "E_ZSTD_DICT"):
        assert R.STATUS[st] in want.values(), st


def test_persistent_waves_take_several_files_each(everything):
    cases, caps, r = everything
    few = S.run([c["blob"] for c in cases], caps, [c["dict"] for c in cases], waves=3)
    assert few["waves"] == 3
    check(cases, few, caps)
    assert few["data"] == r["data"]


def test_the_executor_built_first_gives_the_same_results(everything):
    """the A/B variant of DESIGN.md 3.22: a sequence at a time, where the shipped executor takes a lane per output byte of a batch"""
    cases, caps, r = everything
    plain = S.run([c["blob"] for c in cases], caps, [c["dict"] for c in cases], variant=2)
    check(cases, plain, caps)
    assert plain["data"] == r["data"]
    short = [c - 1 if c else 0 for c in caps]
    check(cases, S.run([c["blob"] for c in cases], short, [c["dict"] for c in cases], variant=2), short)


def test_size_query_then_exact_retry():
    cases = [c for c in _cases() if c["name"] not in ("text_300000_l3_sum", "text_300000_l19_sum")]
    zero = [0] * len(cases)
    q = S.run([c["blob"] for c in cases], zero, [c["dict"] for c in cases])
    check(cases, q, zero)
    sized = [i for i in range(len(cases)) if int(q["status"][i]) == R.STATUS["E_OUTPUT_TOO_SMALL"]]
    assert any(cases[i]["name"] == "stream_no_size" for i in sized)                 # a frame without Frame_Content_Size is sized too
    assert not any(cases[i]["name"] == "wrong_checksum" and int(q["status"][i]) == R.STATUS["E_ZSTD_CHECKSUM"] for i in range(len(cases)))
    again = [cases[i] for i in sized]
    caps = [int(q["out_len"][i]) for i in sized]
    r = S.run([c["blob"] for c in again], caps, [c["dict"] for c in again])
    check(again, r, caps)
    assert {c["name"]: int(r["status"][k]) for k, c in enumerate(again)}["wrong_checksum"] == R.STATUS["E_ZSTD_CHECKSUM"]   # the retry checks it


def test_one_byte_short_of_the_size():
    cases = [c for c in _cases() if Z.expected(c["blob"], c["dict"])[0] == "OK" and 0 < Z.expected(c["blob"], c["dict"])[2] < 50000]
    caps = [Z.expected(c["blob"], c["dict"])[2] - 1 for c in cases]
    r = S.run([c["blob"] for c in cases], caps, [c["dict"] for c in cases])
    check(cases, r, caps)
    assert all(int(s) == R.STATUS["E_OUTPUT_TOO_SMALL"] for s in r["status"])


def test_dictionaries():
    g = [g for g in Z.golden() if g["dict"]][0]
    far = [c for c in Z.crafted() if c["name"].startswith("offset_")]
    cases = [dict(name="with", blob=g["blob"], dict=g["dict"]), dict(name="without", blob=g["blob"], dict=None),
             dict(name="wrong", blob=g["blob"], dict=g["dict"][:-1])] + far + [dict(name="again", blob=g["blob"], dict=g["dict"])]
    caps = [len(g["raw"])] * 3 + [7] * len(far) + [len(g["raw"])]
    r = S.run([c["blob"] for c in cases], caps, [c["dict"] for c in cases])
    check(cases, r, caps)
    assert r["data"][0] == g["raw"] == r["data"][-1] and int(r["status"][1]) == R.STATUS["E_ZSTD_DATA"]
    assert r["span"] > 32768


def test_single_bit_flips():
    fl = Z.flips()
    assert len(fl) >= 196
    caps = [max(Z.expected(f["blob"])[2], 16) for f in fl]
    r = S.run([f["blob"] for f in fl], caps)
    check([dict(name=f["name"], blob=f["blob"], dict=None) for f in fl], r, caps)


def test_xxh64_lengths_seeds_and_offsets():
    rng = np.random.default_rng(64)
    blobs = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in (0, 1, 3, 4, 7, 8, 31, 32, 33, 63, 64, 65, 1000, 4099)]
    for seed in (0, 0x9E3779B97F4A7C15):
        assert S.xxh64(blobs, seed) == [R.xxh64(b, seed) for b in blobs]


def test_the_plan_refuses_what_the_header_says():
    r = S.run([b"x"] * 3, [1] * 3)
    assert r["rc"] == 0 and all(int(s) == R.STATUS["E_EOF"] for s in r["status"])
    lib = S.lib()
    import ctypes as C
    err = C.create_string_buffer(256)
    z = np.zeros(4, np.uint64)
    p = lambda a: C.c_void_p(a.ctypes.data)
    st = np.zeros(4, np.int32)
    rc = lib.sim_zstd_decode(p(z), p(z), p(z), p(z), None, p(z), p(z), p(z), p(z), p(z), p(st), 1, 0, p(z), err, 256)
    assert rc == -1 and b"together" in err.value


# ---- the edge cases, the capacity sweep, the mutations ----------------------------------------------------------------------------------
def _edge():
    return [dict(name=c["name"], blob=c["blob"], dict=c["dict"]) for c in Z.golden_more() + Z.edge_cases()]


def _exact(cases):
    return [Z.expected(c["blob"], c["dict"])[2] if Z.expected(c["blob"], c["dict"])[0] == "OK" else 64 for c in cases]


@pytest.fixture(scope="module")
def edges():
    cases = _edge()
    caps = _exact(cases)
    return cases, caps, S.run([c["blob"] for c in cases], caps, [c["dict"] for c in cases])


def test_edge_cases_in_exact_slots(edges):
    cases, caps, r = edges
    assert r["waves"] == len(cases)
    check(cases, r, caps)
    by_name = {c["name"]: int(r["status"][i]) for i, c in enumerate(cases)}
    assert {c["name"]: by_name[c["name"]] for c in Z.edge_cases()} == {c["name"]: R.STATUS[c["status"]] for c in Z.edge_cases()}
    assert {c["name"]: int(r["out_len"][i]) for i, c in enumerate(cases) if by_name[c["name"]] == 0} == \
           dict([(c["name"], c["size"]) for c in Z.edge_cases() if c["status"] == "OK"] + [(g["name"], len(g["raw"])) for g in Z.golden_more()])


def test_edge_cases_in_the_executor_built_first_and_on_two_waves(edges):
    cases, caps, r = edges
    blobs, dicts = [c["blob"] for c in cases], [c["dict"] for c in cases]
    plain = S.run(blobs, caps, dicts, variant=2)
    check(cases, plain, caps)
    assert plain["data"] == r["data"]
    two = S.run(blobs, caps, dicts, waves=2)
    assert two["waves"] == 2
    check(cases, two, caps)
    assert two["data"] == r["data"]


def test_persistent_waves_keep_nothing_of_the_file_before():
    """tests/test_gpu_zstd.py's files on 12 waves: each takes two of a triple, six take all three"""
    cases = Z.persistent_files(n=30, waves=12)
    caps = _exact(cases)
    for variant in (0, 2):
        r = S.run([c["blob"] for c in cases], caps, [c["dict"] for c in cases], waves=12, variant=variant)
        assert r["waves"] == 12
        check(cases, r, caps)
    refused = {c["name"]: int(r["status"][i]) for i, c in enumerate(cases) if i >= 12 and int(r["status"][i])}
    assert refused == {name: R.STATUS["E_ZSTD_DATA"] for name in (
        "treeless_without_table", "repeat_mode_without_table", "offset_beyond_history", "treeless_with_the_table_of_the_file_before",
        "repeat_mode_with_the_tables_of_the_file_before", "treeless_in_second_frame_alone")}
    assert cases[4]["name"] == "bits3_4000_l1" and cases[16]["name"] == "treeless_with_the_table_of_the_file_before"   # one wave's, in turn
    assert cases[15]["name"] == cases[5]["name"] == "rle_tables" and cases[27]["name"] == cases[17]["name"] == "repeat_mode_with_the_tables_of_the_file_before"


@pytest.mark.parametrize("variant", [0, 2])
def test_capacity_sweep(variant):
    """nothing at or beyond a capacity that ends inside a literal run, a match, a batch or between frames; the size is still exact"""
    cases = Z.capacity_sweep()
    assert len(set(c["blob"] for c in cases)) >= 40 and len(cases) >= 200
    caps = [c["cap"] for c in cases]
    r = S.run([c["blob"] for c in cases], caps, [c["dict"] for c in cases], variant=variant)
    assert r["rc"] == 0, r["err"]
    small = 0
    for i, c in enumerate(cases):
        st, data, out_len, used = R.outcome(c["blob"], c["dict"] or b"", c["cap"])
        got = (int(r["status"][i]), int(r["out_len"][i]), int(r["in_used"][i]))
        assert got == (R.STATUS[st], out_len, used), (c["name"], got, st, out_len, used)
        small += st == "E_OUTPUT_TOO_SMALL"
    assert S.untouched_outside(r["out"], r["out_off"], r["out_cap"])
    by_name = {c["name"]: int(r["status"][i]) for i, c in enumerate(cases)}
    assert by_name["bad_sum_then_overflow@22"] == R.STATUS["E_ZSTD_CHECKSUM"] and by_name["bad_sum_then_overflow@21"] == R.STATUS["E_OUTPUT_TOO_SMALL"]
    assert small >= len(cases) - 8                                   # (all but the files that decode to 0 or 1 bytes, and the checksum)


def test_mutations():
    mu = Z.mutations()
    assert len(mu) >= 596
    caps = [max(Z.expected(m["blob"])[2], 16) for m in mu]
    r = S.run([m["blob"] for m in mu], caps)
    check([dict(name=m["name"], blob=m["blob"], dict=None) for m in mu], r, caps)
