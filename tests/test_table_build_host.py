"""The premises of tests/test_table_build_gpu.py, on the CPU.  The model of the device's table builder (tests/_build_model.py) is
code that can be wrong: for every world it must give, row by row in order, the keys and first positions of the host builder in
strain order, and the oracle's key set.  And every world must hold the edge of the builder it is named for: the rank map's block
count, start bits in the places of a block that take different paths, blocks without a bit, keys first seen on the other strand,
the rows of a repeat, nstarts on the step of the slot count."""
import numpy as np
import pytest

import _build_model as bm
import _oracle
import _regions_model
import _synth
import strainer2_amd as sk
from test_coverage_regions_gpu import STRAIN_ORDER

K = bm.K
ALL = list(bm.WORLDS) + list(bm.STEP_WORLDS)
LETTERS_MAX_BASES = 200000                                             # keys as Python lists of letters: not for 1.1 Mbase


def _stream(name):
    return b"\n".join(bm.records(name)) + b"\n"


@pytest.mark.parametrize("name", ALL)
def test_model_equals_the_host_builder_in_order(name):
    m = bm.model(name)
    ks = sk.Keyset.from_stream(_stream(name), initial_slots=STRAIN_ORDER, default_val=1, incr=0)
    try:
        assert ks.nrows == m.nrows and ks.nwide == 0
        assert np.array_equal(ks.packed(), m.keys), np.nonzero(ks.packed() != m.keys)[0][:10]
        assert np.array_equal(ks.first_pos().astype(np.int64), m.pos)
        okeys, _ = bm.oracle_rows(bm.records(name))
        assert np.array_equal(np.sort(okeys), np.sort(m.keys))
        assert np.array_equal(okeys[bm.rows_of(m.keys, okeys)], m.keys)
        if m.nbases <= LETTERS_MAX_BASES:
            letters = bm.key_bytes(m.keys)
            assert ks.keys() == letters
            assert np.array_equal(_regions_model.keys_of(letters), m.keys)          # (a second packing of the same letters)
    finally:
        ks.close()
    assert (np.diff(m.pos) > 0).all() and m.first.sum() == m.nrows and m.start.sum() == m.nstarts
    text = b"".join(bm.kept(bm.records(name))).upper()
    for row in {0, m.nrows - 1, m.nrows // 2}:                          # a row by hand: the window at its place, on the strand the model names
        w = text[m.pos[row]: m.pos[row] + K]
        assert bm.key_bytes(m.keys[row: row + 1])[0] == (w if m.fwd[row] else _synth.revcomp(w))


def test_model_on_a_text_by_hand():
    """four records whose windows, keys, strands and first places can be read off"""
    a = b"A" * 31
    m = bm.build([a + b"C", b"G" + b"T" * 31, b"ACGT" * 7 + b"AC", b"ACGTN" * 8])
    # record 1: A31 (key T31: the larger strand), A30 C (its reverse complement G T30 is larger); record 2: G T30 again -- no row --,
    # then T31 again; record 3 has 30 bases: in the text, no window; record 4: an N in every window
    assert m.nbases == 32 + 32 + 30 + 40 and m.nstarts == 4 and m.nrows == 2
    assert bm.key_bytes(m.keys) == [b"T" * 31, b"G" + b"T" * 30] and m.pos.tolist() == [0, 1] and m.fwd.tolist() == [False, False]
    assert np.nonzero(m.start)[0].tolist() == [0, 1, 32, 33]
    assert bm.build([b"ACGT" * 7 + b"AC"]).nrows == 0 and bm.build([b"ACGT" * 7 + b"A"]).nbases == 0


# ---- every world's own premise ------------------------------------------------------------------------------------------------------------
def _bits(m):
    return m.block_bits()


@pytest.mark.parametrize("L", bm.ONE_RECORD)
def test_one_record_worlds(L):
    """text lengths around the 16-base words of the text (nbases / 16 + 4 of them) and the 64-base blocks of the rank map; the last
    window is a row; the last 15 places have no 16-mer for level 1 and the last 23 no 24-mer for level 2 (sk_grid_insert_text)"""
    m = bm.model("one%d" % L)
    assert m.nbases == L and m.nstarts == m.nrows == L - 30 and m.pos[-1] == L - K
    assert m.nblk == {31: 2, 32: 2, 47: 2, 48: 2, 63: 2, 64: 3, 65: 3, 94: 3, 95: 3, 127: 3, 128: 4, 129: 4}[L]
    assert {L % 16 for L in bm.ONE_RECORD} >= {0, 1, 15} and {L % 64 for L in bm.ONE_RECORD} >= {0, 1, 63}
    if L >= 95:
        b = _bits(m)
        assert b[0, 31] and b[0, 32] and b[0, 63] and b[1, 0]             # both words of a block, and the step to the next block


def test_thirty_ones_world():
    """one window per record, a start every 31 positions (a record of 30 bases shifts the rest): every place of a block, and blocks
    whose high word has a bit behind bits of the low word (the .y popcount of sk_first_pos_from_rank)"""
    m = bm.model("thirty_ones")
    recs = bm.records("thirty_ones")
    assert sorted({len(r) for r in recs}) == [30, 31] and sum(len(r) == 31 for r in recs) == 2000 == m.nstarts == m.nrows
    assert m.nbases == 2000 * 31 + 20 * 30
    assert set(np.diff(m.pos).tolist()) == {31, 61}
    assert set((m.pos % 64).tolist()) == set(range(64))
    b = _bits(m)
    assert (b[:, :32].any(axis=1) & b[:, 32:].any(axis=1)).sum() > 100 and b[:, 31].any() and b[:, 32].any() and b[:, 63].any() and b[:, 0].any()


def test_n_runs_world():
    """N runs of 1, 40 and 200 and a lower-case stretch: whole blocks without a start bit, windows of lower case, a stretch of 30
    bases between two N (no window)"""
    m = bm.model("n_runs")
    (g,) = bm.records("n_runs")
    runs = sorted(len(x) for x in bytes(c if c in b"Nn" else 32 for c in g).split())
    assert runs == [1, 1, 1, 40, 200]
    b = _bits(m)
    assert (~b[:-2].any(axis=1)).sum() >= 2                                          # (besides the two blocks behind the text)
    low = np.frombuffer(g, dtype=np.uint8) >= 97
    assert (m.start & low[: m.nbases]).sum() > 400 and g.count(b"n" * 200) == 1
    assert m.nstarts == m.nrows == sum(max(len(x) - 30, 0) for x in g.upper().replace(b"N", b" ").split())


def test_repeat_worlds():
    """thousands of windows, one or a few keys: the rows are those of the first period, in the first period's places"""
    m = bm.model("poly_a")
    assert (m.nstarts, m.nrows, m.pos.tolist(), m.fwd.tolist()) == (4970, 1, [0], [False])
    for p in bm.TANDEM:
        m = bm.model("tandem%d" % p)
        assert m.nbases == 4096 + p and m.nstarts == m.nbases - 30 and m.nrows == p and m.pos.tolist() == list(range(p))
    assert not bm.model("tandem64").fwd.all() and bm.model("tandem64").fwd.any()


def test_strands_world():
    """the windows of revcomp(a[500:900]) come first in the text: where a holds them again they are no rows, and their keys stand
    in the text's first 370 windows in the form a does not have them in; the second record's copies are no rows either"""
    m = bm.model("strands")
    r1, r2 = bm.records("strands")
    assert m.nbases == len(r1) + len(r2) and m.nstarts == m.nbases - 60
    assert m.nstarts - m.nrows == 370 + 270 + 270 + (50 - 30)                        # a[500:900], a[100:400], a[2000:2300], a[2950:]
    first370 = m.pos < 370
    assert first370.sum() == 370
    in_a = bm.build([r1[400:]])                                                       # a alone: the same keys, on the other strand
    at = {int(k): bool(f) for k, f in zip(in_a.keys, in_a.fwd)}
    assert all(at[int(k)] != bool(f) for k, f in zip(m.keys[first370], m.fwd[first370]))
    assert (~m.fwd).sum() > 1000 and m.fwd.sum() > 1000
    b = _bits(m)
    assert (b[:, 31] & b[:, 32]).any()
    dup = m.start & ~m.first
    assert dup[400 + 500: 400 + 869].all() and dup[len(r1): len(r1) + 270].all()


@pytest.mark.parametrize("nblk", bm.RANK_NBLK)
@pytest.mark.parametrize("r", [0, 63])
def test_rank_scan_worlds(nblk, r):
    """sk_build_rank_scan gives each of its 1024 threads per = ceil(nblk / 1024) blocks: per of 1, 2 and 3, threads without a block,
    a last slice that is partial, and blocks whose popcounts differ (copies in the second half of the text)"""
    m = bm.model("rank%d_r%d" % (nblk, r))
    assert m.nblk == nblk and m.nbases == 64 * (nblk - 2) + r
    per = -(-nblk // 1024)
    assert per == {1023: 1, 1024: 1, 1025: 2, 2048: 2, 2049: 3, 3000: 3}[nblk]
    busy = -(-nblk // per)
    assert (busy < 1024) == (nblk not in (1024, 2048)) and (nblk % per != 0) == (nblk == 1025)
    pop = _bits(m).sum(axis=1)
    half = nblk // 2
    assert pop[:half].mean() > 63 and pop[half:-2].mean() < 56 and len(set(pop.tolist())) > 20
    assert pop.sum() == m.nrows and (pop[-2:].sum() == 0 if r == 0 else pop[-1] == 0)


def test_big_world():
    """more positions than the 4096 x 256 threads of sk_first_pos_from_rank, more rank blocks than 16 x 1024 (per = 17 in
    sk_build_rank_scan, its last slice partial), and one window in twenty a copy"""
    m = bm.model("big")
    assert m.nbases == bm.BIG > 4096 * 256 and m.nblk > 16 * 1024
    per = -(-m.nblk // 1024)
    assert per == 17 and m.nblk % per != 0 and -(-m.nblk // per) < 1024
    assert 0.03 * m.nstarts < m.nstarts - m.nrows < 0.06 * m.nstarts
    assert (m.pos >= 4096 * 256).sum() > 3000                                         # rows whose position the second turn of the loop finds
    assert (~m.fwd).sum() > 400000 and m.fwd.sum() > 400000


def test_world_without_a_window():
    recs = bm.EMPTY_WORLD()
    m = bm.build(recs)
    assert min(len(r) for r in recs) == 31 and m.nbases == sum(len(r) for r in recs) and m.nstarts == 0 and m.nrows == 0
    t = _oracle.OracleTable(capacity=16384)
    assert t.build_stream(b"\n".join(recs) + b"\n", default=1, incr=0, short_policy=1) == 0 and t.size == 0
    t.close()


@pytest.mark.parametrize("pct,slots", bm.SLOT_STEPS)
def test_slot_count_step_worlds(pct, slots):
    """nstarts on the step of `slots * table_load_pct < nstarts * 100`, one over it and one under; and as many windows in five rows"""
    top = bm.most_starts(slots, pct)
    assert slots * pct >= top * 100 and slots * pct < (top + 1) * 100
    if (pct, slots) == (90, 1024):
        assert top == 921
    for tag, n, want in (("top", top, slots), ("over", top + 1, 2 * slots), ("under", top - 1, slots), ("tandem", top, slots)):
        m = bm.model("step%d_%d_%s" % (pct, slots, tag))
        assert bm.load_pct("step%d_%d_%s" % (pct, slots, tag)) == pct
        assert m.nstarts == n and bm.slot_count(m.nstarts, pct) == want
        assert m.nrows == (5 if tag == "tandem" else n)


def test_scan_streams_hold_what_the_issue_lists():
    for name in ("one31", "thirty_ones", "strands", "big"):
        recs = bm.kept(bm.records(name))
        text = b"".join(recs)
        reads = bm.scan_stream_of(name).split(b"\n")
        assert reads[-1] == b"" and text[:80] in reads and text[-80:] in reads
        if name == "big":
            assert len(reads) - 1 == 4 + 200 and max(map(len, reads)) <= 250
        else:
            assert all(r in reads and _synth.revcomp(r) in reads for r in recs[:50])
        if name in ("thirty_ones", "strands"):
            at = len(recs[0])
            assert text[max(at - 40, 0): at + 40] in reads and sum(len(r) == 80 for r in reads) >= len(recs) - 3
