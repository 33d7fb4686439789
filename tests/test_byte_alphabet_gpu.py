"""The scan's decision about a byte -- a base, a hard breaker, or a byte for the byte-string kernel -- over all 256 byte values, in
every form that makes it: sk_decode16 (the single kernel's phase 1), sk_decode4 (the partitioned pipeline and the candidate form),
sk_chunk_has_odd_byte, sk_is_acgt / sk_is_hard_break and the complement map in sk_scan_wide, with the short odd-chunk list that
sends the byte-string kernel over the whole batch, in COUNT, TALLY and union form.  Expected values are the CPU oracle's, always.

Worlds (tests/_synth.py; tests/test_byte_alphabet_host.py asserts on the oracle's side that they hold what they claim and have power):
  A  one foreign byte in a 93-base strain read, every value at every phase of the 16-byte chunk: 4096 (byte, phase) reads.  The 16
     windows on either side are what catches a byte that spoils the decode of its neighbours in the 32-bit word.
  B  two foreign bytes side by side, every ordered pair of 30 representative bytes on every byte of a word: 3600 reads.
  C  the alphabet on the strain's side: 254 strain records with one byte of every value (but NUL and the separator) in the middle
     -- about 7.5 k byte-string keys --, read back with that byte replaced by every c of 0..255, forward and from the other strand:
     65024 reads (6 MB) per strand.  The oracle's pass over one strand takes 0.6 s on one CPU core (measured when this was written), far below the 10 s at which c would have been thinned, so every c is kept.

NUL is a hard breaker where the oracle ends a C string: the oracle reads N in its place (_for_oracle)."""
import functools
import random

import numpy as np
import pytest

import _oracle
import _synth
import _tally_ref as tr
import strainer2_amd as sk
from test_byte_alphabet_host import _for_oracle, _stream
from test_tally_forms_gpu import _single_forms, _type_col, _union_forms      # every TALLY form of the scan

pytestmark = pytest.mark.gpu


def _expect(sstream, data):
    """(the oracle's keys in row order, its counts of `data`)"""
    t = _oracle.OracleTable()
    assert t.build_stream(sstream, short_policy=1) == 0
    t.scan_stream(_for_oracle(data), 1)
    okeys, oc = t.rows()
    t.close()
    return okeys, oc[:, 1].copy()


@functools.lru_cache(maxsize=None)
def _world(name):
    strain, recs, cases = {"a": _synth.alphabet_world_a, "b": _synth.alphabet_world_b}[name]()
    data = _stream(recs)
    okeys, want = _expect(strain + b"\n", data)
    assert int(want.sum()) > 31 * len(cases)
    want.setflags(write=False)
    return strain + b"\n", data, okeys, want, cases


@pytest.mark.parametrize("odd_list_cap", [0, 3])
@pytest.mark.parametrize("pipeline", [1, 2])
@pytest.mark.parametrize("text_stage", [1, 0])
@pytest.mark.parametrize("name", ["a", "b"])
def test_count_one_and_two_foreign_bytes(name, text_stage, pipeline, odd_list_cap):
    sstream, data, okeys, want, cases = _world(name)
    if name == "a":
        assert {(b, j) for b, j, _i, _w in cases} == {(b, j) for b in range(256) for j in range(16)}
    ks = sk.Keyset.from_stream(sstream)
    assert ks.keys() == okeys
    with sk.KmerContext(0) as c:
        c.set_option("text_stage", text_stage)
        c.set_option("pipeline", pipeline)
        c.set_option("odd_list_cap", odd_list_cap)
        c.load_keyset(ks, 4)
        c.scan_stream(data, 1)
        got = c.counts(1)
    ks.close()
    assert np.array_equal(got, want), np.nonzero(got != want)[0][:10]


def test_count_world_a_resident():
    """World A through the device-resident entry point (sk_scan_device), so the resident path sees every byte as well"""
    sstream, data, okeys, want, _ = _world("a")
    ks = sk.Keyset.from_stream(sstream)
    assert ks.keys() == okeys
    with sk.KmerContext(0) as c:
        c.load_keyset(ks, 4)
        buf = c.dev_alloc(len(data))
        c.dev_upload(buf, np.frombuffer(data, dtype=np.uint8))
        c.scan_device(buf, len(data), 1)
        c.sync()
        c.dev_free(buf)
        got = c.counts(1)
    ks.close()
    assert np.array_equal(got, want), np.nonzero(got != want)[0][:10]


@functools.lru_cache(maxsize=None)
def _world_c(reverse):
    records = _synth.alphabet_world_c()
    sstream = _stream([r for _, r in records])
    data = _synth.alphabet_world_c_reads(records, reverse)
    okeys, want = _expect(sstream, data)
    wide = np.array([bool(set(k) - set(b"ACGT")) for k in okeys])
    # every record read back forward hits its 31 wide keys at least (but N, n, the eight bases, and U in part); from the other strand
    # the oracle decides which c match -- some do
    assert int(want[wide].sum()) > (7000 if not reverse else 1000), int(want[wide].sum())
    want.setflags(write=False)
    return sstream, data, okeys, want


@pytest.mark.parametrize("odd_list_cap", [0, 3])
@pytest.mark.parametrize("reverse", [False, True], ids=["forward", "reverse"])
def test_count_alphabet_on_the_strains_side(reverse, odd_list_cap):
    sstream, data, okeys, want = _world_c(reverse)
    ks = sk.Keyset.from_stream(sstream)
    assert ks.keys() == okeys
    with sk.KmerContext(0) as c:
        c.set_option("odd_list_cap", odd_list_cap)
        c.load_keyset(ks, 4)
        c.scan_stream(data, 1)
        got = c.counts(1)
    ks.close()
    assert np.array_equal(got, want), np.nonzero(got != want)[0][:10]


def test_tally_and_union_forms_on_world_a():
    """World A at phases 0, 3, 12 and 15 (1020 reads: a separator inside a record is outside TALLY's contract, record starts define
    the records) through every TALLY form of one table and of a union of two, the second strain sharing half the first's text; one
    row in five is informative"""
    strain, recs, cases = _synth.alphabet_world_a(phases=(0, 3, 12, 15), leave_out=b"\n")
    assert len(cases) == 255 * 4
    rng = random.Random(4604)
    strains = [strain, strain[:300] + _synth.rand_dna(rng, 300)]
    stream, starts = _stream(recs), tr.starts_of(recs)
    ostream = _for_oracle(stream)
    slots = 4096                                                      # (a small first table on both sides: the oracle's per-record passes stay cheap)
    ctxs, sets, orcs, refs = [], [], [], []
    try:
        for g in strains:
            ks = sk.Keyset.from_stream(g + b"\n", initial_slots=slots, default_val=1, incr=0)
            o = tr.OracleStrain(g + b"\n", capacity=slots)
            assert ks.keys() == o.keys
            informative = np.arange(o.nrows) % 5 == 0
            c = sk.KmerContext(0)
            c.load_keyset(ks, 6)
            c.set_counts(0, _type_col(informative))
            ctxs.append(c)
            sets.append(ks)
            orcs.append(o)
            refs.append(o.tally(ostream, starts, informative))
        assert all(int(r[0][:, 1].sum()) > 1000 for r in refs)
        for s, c in enumerate(ctxs):
            for name, t, h in _single_forms(c, stream, starts, False):
                tr.check_single(orcs[s], ostream, starts, refs[s], t, h, (s, name))
        with sk.KmerUnion(ctxs, 0, 2) as u:
            for name, t, h in _union_forms(u, stream, starts, False):
                for s in range(len(ctxs)):
                    tr.check_single(orcs[s], ostream, starts, refs[s], t[:, s, :], h[h[:, 0] == s][:, 1:], (s, name))
    finally:
        for c in ctxs:
            c.close()
        for k in sets:
            k.close()
