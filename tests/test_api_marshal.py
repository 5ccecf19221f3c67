"""What the Python host layer hands to librcx.so, and what it makes of the answers, against tests/golden/api_marshal.json -- on the CPU, with
a stand-in for the library (tests/gen_api_marshal_golden.py has the stand-in, the cases and the generator).  Everything is compared for
equality: the rcx_batch of every call (null pointers, offsets, lengths, capacities, the input bytes, the output buffer as handed over), every
extra argument, the order of the calls, the results and every exception's type and message."""
import json

import pytest

import gen_api_marshal_golden as G


with open(G.GOLDEN) as _f:
    RECORDED = json.load(_f)


@pytest.fixture(scope="module")
def recorded():
    return RECORDED


@pytest.fixture(scope="module")
def replayed():
    """every case once, under the stand-in (module scope: pytest's monkeypatch fixture is per test, so its class is used directly)"""
    import rust_compress_amd._native as N
    stand_in = G.StandIn()
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(N, "lib", lambda: stand_in)
        return json.loads(G.dumps(G.record(stand_in)))                 # (through JSON, as the recording went: tuples are lists there)


def test_every_case_is_recorded(recorded, replayed):
    assert list(replayed) == list(recorded)


def test_every_batch_entry_point_is_reached(replayed):
    """each rcx_*_batch function that the layer binds for host memory is handed a batch by some case"""
    import rust_compress_amd._native as N
    bound = {e for e in N.EXPORTS if e.endswith("_batch") and e != "rcx_multi_batch"}
    assert bound == set(G.EXTRA)
    assert {c["fn"] for case in replayed.values() for c in case["calls"]} == bound


@pytest.mark.parametrize("name", list(RECORDED))
def test_case(name, recorded, replayed):
    got, want = replayed[name], recorded[name]
    assert [c["fn"] for c in got["calls"]] == [c["fn"] for c in want["calls"]]
    for g, w in zip(got["calls"], want["calls"]):
        assert g == w
    assert got == want
