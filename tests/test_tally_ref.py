"""The TALLY reference of tests/_tally_ref.py checked on the CPU: on A/C/G/T reads it agrees with a brute-force count
and with the numpy reference, a world with U windows gives a non-empty log, and a log with a wrong entry fails."""
import collections
import random

import numpy as np
import pytest

import _synth
import _tally_ref as tr

COMP = bytes.maketrans(b"ACGT", b"TGCA")


def _brute(keys, informative, recs):
    """per record (all, informative) and the log {(record, offset, row)} by looking every window up"""
    row_of = {k: i for i, k in enumerate(keys)}
    tally, log, off = [], [], 0
    for r, rec in enumerate(recs):
        u = rec.upper()
        h = n = 0
        for j in range(len(u) - 30):
            w = u[j:j + 31]
            if set(w) - set(b"ACGT"):
                continue
            row = row_of.get(max(w, w.translate(COMP)[::-1]))
            if row is not None:
                h += 1
                if informative[row]:
                    n += 1
                    log.append((r, off + j + 30, row))
        tally.append((h, n))
        off += len(rec) + 1
    return np.array(tally, dtype=np.int64).reshape(-1, 2), log


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_reference_agrees_with_brute_force(seed):
    rng = random.Random(seed)
    strain = _synth.tally_strains(rng, seed, 1, sizes=(3000,))[0]
    recs, _ = _synth.tally_reads(rng, [strain], 150, junk=False)
    stream = b"\n".join(recs) + b"\n"
    starts = tr.starts_of(recs)
    o = tr.OracleStrain(strain + b"\n")
    informative = np.zeros(o.nrows, dtype=bool)
    informative[rng.sample(range(o.nrows), o.nrows // 4)] = True
    bt, blog = _brute(o.keys, informative, recs)
    assert int(bt[:, 1].sum()) > 20                                   # (not vacuous)
    ot, olog = o.tally(stream, starts, informative)
    assert np.array_equal(ot, bt)
    assert olog == collections.Counter((r, row) for r, _, row in blog)
    packed = np.array([int(k.translate(bytes.maketrans(b"ACGT", b"0123")), 4) for k in o.keys], dtype=np.uint64)
    ct, clog = tr.canonical_tally(packed, informative, stream, starts)
    assert np.array_equal(ct, bt)
    assert np.array_equal(clog, np.array(sorted((p, row) for _, p, row in blog), dtype=np.int64).reshape(-1, 2))
    tr.check_single(o, stream, starts, (ot, olog), ot, clog, "brute")
    bad = clog.copy()                                                 # one entry moved by a base: the window check must see it
    bad[len(bad) // 2, 0] += 1
    with pytest.raises(AssertionError):
        tr.check_log(o, stream, starts, bad, olog)
    bad = clog.copy()                                                 # one entry with another row
    bad[0, 1] = (bad[0, 1] + 1) % o.nrows
    with pytest.raises(AssertionError):
        tr.check_log(o, stream, starts, bad, olog)


def test_u_windows_hit_in_the_reference():
    """reads that hold U windows (the byte-string kernel's only way to a hit on a union table) give informative hits"""
    rng = random.Random(5)
    strain = _synth.rand_dna(rng, 4000)
    recs, wins = [], []
    for _ in range(40):
        u, w = _synth.u_window(rng, strain)
        recs.append(_synth.rand_dna(rng, rng.randrange(0, 20)) + u + _synth.rand_dna(rng, rng.randrange(0, 20)))
        wins.append(w)
    stream = b"\n".join(recs) + b"\n"
    o = tr.OracleStrain(strain + b"\n")
    informative = np.zeros(o.nrows, dtype=bool)
    informative[[o.row_of[w] for w in wins]] = True
    tally, log = o.tally(stream, tr.starts_of(recs), informative)
    assert (tally[:, 1] >= 1).all() and sum(log.values()) >= len(recs)
    assert all(b"U" in r.upper() for r in recs)
