"""Every TALLY form of the scan (strain_detect's per-record tallies and log of informative hits) against the oracle-built
reference of tests/_tally_ref.py: tallies exactly, the log as a multiset, entry by entry.

Forms: sk_tally_batch (single kernel, pipeline 2, a three-entry odd-chunk list); a batch with sk_tally_launch and the
dense or the sparse collection, from bytes and from the host-packed form; the union table from bytes and packed, with the
default odd-chunk list and a three-entry one (the byte-string kernel then walks the whole batch).  Worlds with junk hold
U windows that hit for certain (the byte-string kernel's one way to a union hit: sk_scan_wide<TALLY, UNION>), IUPAC
letters and '\\r'; worlds without are the packed forms' too.  Then the edges of record attribution (sk_record_of), the
packed form's last chunk, a log that runs over, a batch refilled in both forms, and the informative-row bitmap."""
import random

import numpy as np
import pytest

import _synth
import _tally_ref as tr
import strainer2_amd as sk
from strainer2_amd.native import TallyBatch

pytestmark = pytest.mark.gpu


def _load(g, ncols=6):
    """(context, key set, oracle strain) of one strain; the product's rows must be the oracle's"""
    ks = sk.Keyset.from_stream(g + b"\n", default_val=1, incr=0)
    o = tr.OracleStrain(g + b"\n")
    assert ks.keys() == o.keys
    c = sk.KmerContext(0)
    c.load_keyset(ks, ncols)
    return c, ks, o


def _type_col(informative):
    t = np.ones(len(informative), dtype=np.uint32)
    t[informative] = 2
    return t


def _sparse_to_dense(recs, nrec):
    assert len(np.unique(recs[:, 0])) == len(recs) and (recs[:, 1] > 0).all(), "sparse: a record twice or one without hits"
    t = np.zeros((nrec, 2), dtype=np.uint32)
    t[recs[:, 0]] = recs[:, 1:]
    return t


def _single_forms(c, stream, starts, packable, value=2):
    """(name, tally, hits) of every single-table form on one batch (type column 0, informative `value`)"""
    nrec = len(starts)
    yield ("tally_batch",) + c.tally_batch(stream, starts, 0, value)
    for opt, val in (("pipeline", 2), ("odd_list_cap", 3)):
        c.set_option(opt, val)
        try:
            yield (f"tally_batch {opt}={val}",) + c.tally_batch(stream, starts, 0, value)
        finally:
            c.set_option(opt, 0)
    with TallyBatch(c) as b:
        for packed in ((False, True) if packable else (False,)):
            b.fill(stream, starts, packed=packed)
            c.tally_launch(b, 0, value)
            t, h, n = c.tally_collect()
            assert n == len(h)
            yield f"launch+collect packed={packed}", t, h
            c.tally_launch(b, 0, value)
            r, h, n = c.tally_collect_sparse()
            assert n == len(h)
            yield f"launch+sparse packed={packed}", _sparse_to_dense(r, nrec), h


def _union_forms(u, stream, starts, packable):
    """(name, tally[nrec, members, 2], hits[n, 3]) of the union forms"""
    yield ("union",) + u.tally_batch(stream, starts)
    if packable:
        yield ("union packed",) + u.tally_batch(stream, starts, packed=True)
    u.set_option("odd_list_cap", 3)
    try:
        yield ("union odd_list_cap=3",) + u.tally_batch(stream, starts)
    finally:
        u.set_option("odd_list_cap", 0)


def _world(seed):
    rng = random.Random(seed)
    n = 1 + seed % 4
    strains = _synth.tally_strains(rng, seed, n)
    junk = seed % 2 == 1
    recs, uk = _synth.tally_reads(rng, strains, rng.choice([250, 400, 550]), junk)
    if junk:
        assert uk, "a junk world without U windows"
    stream = b"\n".join(recs) + b"\n"
    return rng, strains, stream, tr.starts_of(recs), uk, junk


@pytest.mark.parametrize("seed", range(16))
def test_tally_forms_against_the_oracle(seed):
    rng, strains, stream, starts, uk, junk = _world(seed)
    ctxs, sets, refs, orcs = [], [], [], []
    try:
        for g in strains:
            c, ks, o = _load(g)
            informative = np.zeros(o.nrows, dtype=bool)
            informative[rng.sample(range(o.nrows), max(1, o.nrows // rng.choice([3, 5, 20])))] = True
            for w in uk:                                               # the U windows' rows are informative where they are keys
                if w in o.row_of:
                    informative[o.row_of[w]] = True
            c.set_counts(0, _type_col(informative))
            ctxs.append(c)
            sets.append(ks)
            orcs.append(o)
            refs.append(o.tally(stream, starts, informative))
        assert sum(int(r[0][:, 1].sum()) for r in refs) > 0
        for s, c in enumerate(ctxs):
            for name, t, h in _single_forms(c, stream, starts, not junk):
                tr.check_single(orcs[s], stream, starts, refs[s], t, h, (seed, s, name))
        with sk.KmerUnion(ctxs, 0, 2) as u:
            for name, t, h in _union_forms(u, stream, starts, not junk):
                for s in range(len(ctxs)):
                    tr.check_single(orcs[s], stream, starts, refs[s], t[:, s, :], h[h[:, 0] == s][:, 1:], (seed, s, name))
    finally:
        for c in ctxs:
            c.close()
        for k in sets:
            k.close()


# ---- edges, against the numpy reference (A/C/G/T reads: positions known exactly) -------------------------------------
def _edge_check(strains, recs, rng, union=True, what=""):
    stream = b"\n".join(recs) + b"\n"
    starts = tr.starts_of(recs)
    ctxs, sets, wants = [], [], []
    try:
        for g in strains:
            ks = sk.Keyset.from_stream(g + b"\n", default_val=1, incr=0)
            c = sk.KmerContext(0)
            c.load_keyset(ks, 6)
            informative = np.zeros(ks.nrows, dtype=bool)
            informative[rng.sample(range(ks.nrows), ks.nrows // 3)] = True
            c.set_counts(0, _type_col(informative))
            ctxs.append(c)
            sets.append(ks)
            wants.append(tr.canonical_tally(ks.packed(), informative, stream, starts))
        for s, c in enumerate(ctxs):
            for name, t, h in _single_forms(c, stream, starts, True):
                tr.check_exact(wants[s], t, h, (what, s, name))
        if union:
            with sk.KmerUnion(ctxs, 0, 2) as u:
                for name, t, h in _union_forms(u, stream, starts, True):
                    for s in range(len(ctxs)):
                        tr.check_exact(wants[s], t[:, s, :], h[h[:, 0] == s][:, 1:], (what, s, name))
    finally:
        for c in ctxs:
            c.close()
        for k in sets:
            k.close()
    return stream, starts, wants


def _piece(rng, g, n):
    a = rng.randrange(len(g) - n)
    s = g[a:a + n]
    return _synth.revcomp(s) if rng.random() < 0.5 else s


def test_record_spanning_several_tiles():
    """a record of 100 kb (four 32 KiB tiles whose tile_first entries are all equal) between short ones"""
    rng = random.Random(11)
    g = _synth.rand_dna(rng, 120_000)
    other = _synth.mutate(rng, g, 0.01)
    recs = [_piece(rng, g, 150) for _ in range(20)] + [_synth.mutate(rng, g[5000:105_000], 0.002)] + [_piece(rng, g, 150) for _ in range(20)]
    stream, starts, wants = _edge_check([g, other], recs, rng, what="long record")
    s, e = starts[20], starts[21]
    assert e - s > 3 * 32768 and int(wants[0][0][20, 1]) > 1000


def test_a_thousand_short_records_in_a_tile_next_to_a_long_one():
    """over a thousand 31-35-base records in one 32 KiB tile next to a 20 kb record: the interpolated guess of sk_record_of
    misses in the tiles they share, and the binary search must finish the job"""
    rng = random.Random(12)
    g = _synth.rand_dna(rng, 40_000)
    short = lambda: _piece(rng, g, rng.choice([31] * 8 + [33, 35]))   # noqa: E731
    recs = [short() for _ in range(1500)] + [g[1000:21_000]] + [short() for _ in range(1200)] + [_synth.revcomp(g[15_000:35_000])] + [short() for _ in range(300)]
    stream, starts, _ = _edge_check([g], recs, rng, what="dense tile")
    per_tile = np.bincount(starts >> 15)
    assert per_tile.max() > 1000


@pytest.mark.parametrize("d", [0, 1, 16, 30, 31, 32, 40, 200])
def test_windows_ending_at_the_tile_edge(d):
    """a record of strain text starting d bytes before the second tile (d = 0: exactly on it; 30 / 31: its first window
    ends at 32768 / 32767), so that strain k-mers end exactly at offsets 32767 and 32768 whenever the record reaches back"""
    rng = random.Random(13 + d)
    g = _synth.rand_dna(rng, 60_000)
    head, off = [], 0
    while 32768 - d - off > 400:                                     # short records up to a few hundred bytes before the edge
        r = _piece(rng, g, 150)
        head.append(r)
        off += len(r) + 1
    head.append(_synth.rand_dna(rng, 32768 - d - off - 1))           # (the next record starts at 32768 - d)
    recs = head + [g[100:500]] + [_piece(rng, g, 200) for _ in range(10)]
    stream, starts, _ = _edge_check([g], recs, rng, what=f"edge d={d}")
    assert int(starts[len(head)]) == 32768 - d
    ks = sk.Keyset.from_stream(g + b"\n", default_val=1, incr=0)
    pos = tr.canonical_tally(ks.packed(), np.ones(ks.nrows, dtype=bool), stream, starts)[1][:, 0]
    ks.close()
    for p in (32767, 32768):
        assert (p in pos) == (p >= 32768 - d + 30), p


def test_records_starting_mid_chunk_and_on_the_chunk_grid():
    """records starting at every offset modulo 16 (so exactly on a 16-byte boundary and mid-chunk), hitting from their
    first window on"""
    rng = random.Random(14)
    g = _synth.rand_dna(rng, 30_000)
    recs, mods = [], set()
    off = 0
    for i in range(400):
        r = _piece(rng, g, rng.randrange(31, 90))
        mods.add(off % 16)
        recs.append(r)
        off += len(r) + 1
    assert mods == set(range(16))
    _edge_check([g, _synth.mutate(rng, g, 0.02)], recs, rng, what="chunk grid")


@pytest.mark.parametrize("tail", range(16))
def test_packed_last_chunk(tail):
    """batch lengths of every residue modulo 16: the last chunk of the packed form is partial.  The last record ends where
    the strain goes on with an A, and holds an N where the strain has an A: were the last chunk's bytes taken as bases
    (code 0 = A), the window over the closing newline and the windows over the N would hit"""
    rng = random.Random(100 + tail)
    g = _synth.rand_dna(rng, 20_000)
    recs = [_piece(rng, g, 100) for _ in range(30)]
    j = next(i for i in range(5000, len(g)) if g[i] == ord("A") and g[i - 5] == ord("A"))
    total = sum(len(r) + 1 for r in recs)
    ln = 60
    while (total + ln + 1) % 16 != tail:
        ln += 1
    last = bytearray(g[j - ln:j])
    last[-5] = ord("N")
    recs.append(bytes(last))
    stream, _, _ = _edge_check([g], recs, rng, what=f"tail {tail}")
    assert len(stream) % 16 == tail


def test_log_overflow_reports_the_true_count_and_relaunch_recovers():
    """hits_cap below the log's length: the true count comes back, what was stored belongs to the log, and a launch with
    room returns the whole log -- dense and sparse, bytes and packed"""
    rng = random.Random(15)
    g = _synth.rand_dna(rng, 8000)
    recs = [_piece(rng, g, 150) for _ in range(300)]
    stream = b"\n".join(recs) + b"\n"
    starts = tr.starts_of(recs)
    ks = sk.Keyset.from_stream(g + b"\n", default_val=1, incr=0)
    informative = np.zeros(ks.nrows, dtype=bool)
    informative[::2] = True
    want = tr.canonical_tally(ks.packed(), informative, stream, starts)
    full = {tuple(x) for x in want[1].tolist()}
    assert len(full) > 1000
    with sk.KmerContext(0) as c:
        c.load_keyset(ks, 4)
        c.set_counts(0, _type_col(informative))
        with TallyBatch(c) as b:
            for packed in (False, True):
                b.fill(stream, starts, packed=packed)
                for sparse in (False, True):
                    c.tally_launch(b, 0, 2, hits_cap=7)
                    t, h, n = c.tally_collect_sparse() if sparse else c.tally_collect()
                    assert n == len(full) and len(h) == 7 and {tuple(x) for x in h.tolist()} <= full, (packed, sparse)
                    c.tally_launch(b, 0, 2, hits_cap=n)
                    t, h, n2 = c.tally_collect_sparse() if sparse else c.tally_collect()
                    tr.check_exact(want, _sparse_to_dense(t, len(starts)) if sparse else t, h, (packed, sparse))
    ks.close()


def test_batch_refilled_as_bytes_and_packed_in_turn():
    """one batch object filled with bytes, then packed, then bytes, ... with batches of different sizes (the way the program
    sends a chunk with an odd byte as bytes and the others packed)"""
    rng = random.Random(16)
    g = _synth.rand_dna(rng, 20_000)
    ks = sk.Keyset.from_stream(g + b"\n", default_val=1, incr=0)
    informative = np.zeros(ks.nrows, dtype=bool)
    informative[rng.sample(range(ks.nrows), ks.nrows // 4)] = True
    with sk.KmerContext(0) as c:
        c.load_keyset(ks, 4)
        c.set_counts(0, _type_col(informative))
        with TallyBatch(c) as b:
            for i, nrec in enumerate([200, 2000, 50, 900, 1, 3000]):
                recs = [_piece(rng, g, rng.choice([31, 80, 150])) for _ in range(nrec)]
                stream = b"\n".join(recs) + b"\n"
                starts = tr.starts_of(recs)
                want = tr.canonical_tally(ks.packed(), informative, stream, starts)
                b.fill(stream, starts, packed=bool(i % 2))
                c.tally_launch(b, 0, 2)
                t, h, _ = c.tally_collect()
                tr.check_exact(want, t, h, (i, nrec))
    ks.close()


def test_informative_bitmap_follows_the_type_column():
    """the bitmap of informative rows is cached per context: after set_counts, sk_counts_set_rows, zero_counts, a COUNT
    scan into the type column and a new informative value, every tally must follow the column as it is now"""
    import _oracle
    rng = random.Random(17)
    g = _synth.rand_dna(rng, 15_000)
    recs = [_piece(rng, g, rng.choice([64, 150])) for _ in range(600)]
    stream = b"\n".join(recs) + b"\n"
    starts = tr.starts_of(recs)
    ks = sk.Keyset.from_stream(g + b"\n", default_val=1, incr=0)
    packed = ks.packed()
    t = _oracle.OracleTable(ncols=2)
    assert t.build_stream(g + b"\n", default=1, incr=0, short_policy=1) == 0
    assert t.rows()[0] == ks.keys()

    def check(c, typ, value, what):
        want = tr.canonical_tally(packed, typ == value, stream, starts)
        for name, tl, h in _single_forms(c, stream, starts, True, value):
            tr.check_exact(want, tl, h, (what, name))

    with sk.KmerContext(0) as c:
        c.load_keyset(ks, 4)
        typ = _type_col(np.arange(ks.nrows) % 3 == 0)
        c.set_counts(0, typ)
        check(c, typ, 2, "first")
        typ = _type_col(np.arange(ks.nrows) % 3 == 1)                  # every informative row changes
        c.set_counts(0, typ)
        check(c, typ, 2, "set_counts")
        rows = np.array(rng.sample(range(ks.nrows), ks.nrows // 2), dtype=np.uint32)
        c.set_counts_rows(0, rows, 2)
        typ[rows] = 2
        check(c, typ, 2, "set_counts_rows")
        c.zero_counts(0)
        typ[:] = 0
        check(c, typ, 2, "zero_counts")
        more = g[:9000] + b"\n" + g[3000:7000] + b"\n"                 # counts 1 and 2 in the type column, by a COUNT scan
        c.scan_stream(more, 0)
        t.scan_stream(more, 1)
        typ = t.counts()[:, 1].copy()
        assert np.array_equal(c.counts(0), typ) and (typ == 2).sum() > 1000
        check(c, typ, 2, "COUNT scan")
        check(c, typ, 1, "informative value 1")
    ks.close()
