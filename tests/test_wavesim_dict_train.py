"""CPU suite: dictionary training (rcx_dict_train_batch) -- the UNMODIFIED kernels and launch loop of k_dict_train.hip with the host's
rcx_plan_train on the wave64 simulator, against the serial reference tests/dict_train_ref (written from the specification of DESIGN.md
3.19 by definition): bytes, out_len, in_used and status of every job.  The cases are the smallest at which each rule can go wrong."""
import os
import sys
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dict_train_cases as K          # noqa: E402
import sim_dict_train_run as S        # noqa: E402
from rust_compress_amd import synth   # noqa: E402


def check(jobs, k, d, f):
    """jobs: [(name, samples, C)] in ONE call -> the call's result, every job held to the reference"""
    r = S.run([(s, c) for _, s, c in jobs], k=k, d=d, f=f)
    assert r["rc"] == 0, r["err"]
    for i, (name, s, c) in enumerate(jobs):
        ref = K.ref_train(s, c, k, d, f)
        assert r["status"][i] == 0 and int(r["in_used"][i]) == sum(len(x) for x in s), name
        assert int(r["out_len"][i]) == len(ref), (name, int(r["out_len"][i]), len(ref))
        assert r["dicts"][i] == ref, name
    assert S.untouched_outside(r)
    return r


def rand(n, seed):
    return synth.gen("rand", n, seed).tobytes()


@pytest.mark.parametrize("d", [6, 8])
def test_corpus_and_capacity_edges(d):
    """n = 0, n < d, n = d with k > n, n = k (one start), n = k + 1; C = 0, d - 1, d, k - 1, k, 1000, 4096, 32768"""
    jobs = K.size_jobs(16, d)
    r = check([(n, s, c) for n, s, c, _, _, _ in jobs], 16, d, 20)
    by = {j[0]: int(l) for j, l in zip(jobs, r["out_len"])}
    assert by["n=0"] == 0 and by["n<d"] == 0 and by["n=d, k>n"] == 0 and by["C=0"] == 0 and by["C=%d" % (d - 1)] == 0
    assert by["n=k"] == 16 and by["C=%d" % d] == d and 1000 - d < by["C=1000"] <= 1000      # (a tail below d ends the job)


@pytest.mark.parametrize("d,k", [(d, k) for d in (6, 8) for k in (0, 16, 64, 256, 4096)])
def test_parameters(d, k):
    """d = 6 and 8, k = d, 16, 64, 256, 4096, f = 10, 20, 22"""
    k = k or d
    for name, s, c, kk, dd, f in K.param_jobs():
        if (kk, dd) == (k, d):
            check([(name, s, c)], kk, dd, f)


def test_small_table_of_colliding_hashes():
    """f = 10 over 64 KiB of text: 1024 frequencies for 65 000 substrings, so colliding hashes inside one segment are the rule"""
    t = K.text(65536, 21)
    check([("f=10", K.split(t, [2048] * 31), 4096)], 256, 8, 10)


def test_samples_of_length_0_and_shorter_than_d_between_long_ones():
    t = K.text(6000, 22)
    for d in (6, 8):
        sizes = [1500, 0] + list(range(1, d)) + [0, 0, 2000, d - 1, d, d + 1, 1]
        check([("short samples", K.split(t, sizes), 1024), ("short samples first", K.split(t, [0, 1, d - 1, 3000]), 512)], 32, d, 20)


def test_substrings_that_span_two_samples_do_not_count():
    """W's eight-byte substrings are frequent, each in a sample of its own.  The end of one sample and the start of the next spell W: if
    the substrings across that boundary counted, the start there would score 9 x 21 and win.  They do not, so the winner is V, six
    whole copies: 9 x 6 = 54 against 28 for a sample of one frequent substring and junk.  C = k: the dictionary is the winner."""
    W, V = b"0123456789abcdef", b"VWXYZvwxyz[]{}()"
    junk = rand(4096, 23)
    samples, at = [], 0
    for rep in range(20):
        for j in range(1, 8):
            samples.append(W[j:j + 8] + junk[at:at + 8])
            at += 8
    samples += [junk[at:at + 40] + W[:8], W[8:] + junk[at + 40:at + 80]]
    samples += [V] * 6
    r = check([("spanning", samples, 16)], 16, 8, 20)
    assert r["dicts"][0] == V


def test_a_periodic_stretch_loses_to_distinct_frequent_substrings():
    """An 8-byte pattern repeated 64 times: a segment of it sums 57 x 57 counting every position, but holds 8 DISTINCT substrings, 8 x 57.
    Q, 64 bytes without a repeat, in twenty samples: 57 x 20.  Q wins although the periodic stretch comes first and sums higher.  (A
    segment may lie across samples: 64 bytes that occur once keep the two stretches out of one segment.)"""
    Q = rand(64, 24)
    samples = [b"abcdefgh" * 64, rand(64, 34)] + [Q] * 20
    r = check([("periodic", samples, 64)], 64, 8, 20)
    assert r["dicts"][0] == Q


def test_ties_go_to_the_lowest_start():
    t = K.text(2048, 25)
    r = check([("two halves", [t, t], 256)], 64, 8, 20)
    assert r["dicts"][0] == K.ref_train([t, t], 256, 64, 8, 20)
    x = rand(1500, 26)
    # 1500 random substrings in a table of 2^22 all have frequency 1: every score of an epoch is equal and its first start is taken
    # (E = 2, size = 750); the third round is back in the first epoch, where the first segment whose nine substrings are all left starts at 9
    r = check([("rand", [x], 160)], 16, 8, 22)
    assert r["dicts"][0][-16:] == x[:16] and r["dicts"][0][-32:-16] == x[750:766] and r["dicts"][0][-48:-32] == x[9:25]


def test_epochs():
    """Positions at or beyond E x size are never starts: n = 420, k = 16, C = 1024 gives epochs of 10 k = 160 and E = 2; the hundred
    bytes left over hold five copies of V and nothing else does, so only a start among them could bring V into the dictionary.  The
    same job exercises the size < 10 k branch, and its second epoch is clipped at n - k + 1 by nothing (the rest lies behind it); the
    random corpus of 5000 has its last epoch clipped."""
    V = b"VWXYZvwxyz[]{}()"
    x = rand(340, 27)                                                # (no segment of a start below 320 reaches V at 340)
    r = check([("remainder", [x + V * 5], 1024)], 16, 8, 20)
    assert V[:8] not in r["dicts"][0] and len(r["dicts"][0]) > 0
    check([("clipped", [rand(5000, 28)], 2048)], 64, 8, 20)


def test_more_rounds_than_epochs():
    """C = 32768, k = 64, a 64 KiB corpus: 102 epochs, 606 rounds"""
    t = K.text(65536, 29)
    samples = K.split(t, [2048] * 31)
    r = check([("rounds", samples, 32768)], 64, 8, 20)
    assert int(r["rounds"][0]) == K.ref_train(samples, 32768, 64, 8, 20, with_rounds=True)[1] > 400


def test_running_dry():
    """one 512-byte record eight times, C = 32768: ten rounds without a start end the job; the dictionary holds the record once"""
    rec = K.text(512, 30)
    r = check([("dry", [rec] * 8, 32768)], 256, 8, 20)
    dct = r["dicts"][0]
    assert 512 <= len(dct) < 1024
    assert {rec[i:i + 8] for i in range(505)} <= {dct[i:i + 8] for i in range(len(dct) - 7)}


def test_last_segment():
    """tail smaller than the segment: its first bytes alone (C = 1000, segments of 256); tail smaller than d: the job stops"""
    x = rand(3000, 31)
    r = check([("clipped", [x], 1000), ("stops", [x], 16 + 5), ("stops at once", [x], 7)], 16, 8, 20)
    assert [int(v) for v in r["out_len"]] == [1000, 16, 0]
    r = check([("clipped", [K.text(20000, 32)], 1000)], 256, 8, 20)
    assert int(r["out_len"][0]) == 1000


def test_batch_of_twelve_and_its_permutation():
    jobs = K.batch_jobs()
    r = check(jobs, 64, 8, 20)
    assert len(set(int(v) for v in r["rounds"])) > 6                 # (different round counts in one call)
    order = [7, 2, 0, 11, 5, 9, 1, 3, 10, 4, 8, 6]
    p = check([jobs[i] for i in order], 64, 8, 20)
    assert [p["dicts"][order.index(i)] for i in range(12)] == r["dicts"]


def test_a_job_larger_than_a_launch():
    """200 KiB in ONE epoch (C = 1000): more positions than the hash, distance and range launches' grids times their tiles (128 Ki) and
    more difference words than the scan's; and C = 32768 against the last launch's 16 Ki"""
    t = K.text(200 * 1024, 33)
    check([("one epoch", K.split(t, [70000, 65536]), 1000), ("large C", K.split(t[:150000], [4096] * 30), 32768)], 256, 8, 20)


def test_refusals():
    ok = dict(in_len=[100], out_cap=[64], nsamples=[2], sample_len=[60, 40])
    assert S.plan_only(**ok)[0] == 0
    for kw in (dict(d=7), dict(k=7, d=8), dict(k=5, d=6), dict(k=4097), dict(f=9), dict(f=23)):
        rc, err = S.plan_only(**ok, **kw)
        assert rc == S.RC_BAD_ARG and "dict train" in err, kw
    rc, err = S.plan_only([100, 100], [64, 64], [1, 2], [100, 60, 41])
    assert rc == S.RC_BAD_ARG and "job 1" in err
    rc, err = S.plan_only([100, 1 << 32], [64, 64], [1, 1], [100, 1 << 32])
    assert rc == S.RC_BAD_ARG and "job 1" in err
    for name in ("in_len", "out_cap", "nsamples", "sample_len"):
        assert S.plan_only(**ok, null=name)[0] == S.RC_BAD_ARG, name
    assert S.plan_only([], [], [], [])[0] == 0
    # ... and through the whole call: lengths that do not add up
    r = S.run([([b"x" * 100], 64)], k=16, lens_override={0: [99]})
    assert r["rc"] == S.RC_BAD_ARG and "job 0" in r["err"]


def _deflate_total(records, zdict):
    total = 0
    for rec in records:
        c = zlib.compressobj(6, zlib.DEFLATED, -15, zdict=zdict) if zdict else zlib.compressobj(6, zlib.DEFLATED, -15)
        total += len(c.compress(rec) + c.flush())
    return total


@pytest.mark.parametrize("kind", ["text", "words", "dna4", "runs"])
def test_usefulness(kind):
    """256 training records of 2 KiB, 64 held-out ones, raw DEFLATE at level 6 through libz: behind the trained dictionary (C = 32768,
    k = 256, d = 8, f = 20) the held-out records take less than without one; for text and words also less than behind the first C
    bytes of the corpus, which in turn beats none.  The totals are DESIGN.md 3.19's."""
    train = K.records(kind, 256, 2048, 1000)
    held = K.records(kind, 64, 2048, 5000)
    r = check([(kind, train, 32768)], 256, 8, 20)
    none, head, trained = _deflate_total(held, None), _deflate_total(held, b"".join(train)[:32768]), _deflate_total(held, r["dicts"][0])
    print("usefulness %s: none %d head %d trained %d rounds %d" % (kind, none, head, trained, int(r["rounds"][0])))
    assert trained < none
    if kind in ("text", "words"):
        assert trained < head < none
