"""The premises of tests/test_stage2_worlds_gpu.py, on the CPU: every world of tests/_stage2_worlds.py is what it claims to be, holds
what gives it power over stage 2 of the scan kernel, and the oracle counts in it what the construction planned.  The set model
(every 31-mer of the strain's records, either strand) is a second, plain statement of what a window counts; the oracle is the one
the GPU tests compare with."""
import pytest

import _stage2_worlds as w2
import _synth

K = w2.K


def _oracle_total(w, m=0):
    return int(w.count_refs[m][1].sum())


def test_redraw_conditions_hold_on_the_first_draw():
    """no repeated 16-mer (shift), only the planted repeats (runs), distinct keys (the difference-array strains), no seam window
    that is a key (the unions of ends): random strains of these sizes pass at once"""
    assert w2.shift_world().redraws == 0 and w2.runs_world().redraws == 0
    assert [w2.diff_strain(n)[0] for n in w2.DIFF_NROWS] == [0] * len(w2.DIFF_NROWS)
    assert [w2.ends_union_world(p).redraws for p in w2.ENDS_UNIONS] == [0] * len(w2.ENDS_UNIONS)
    with pytest.raises(AssertionError):
        w2.redraw(1, lambda rng: 0, lambda x: False)                   # (and a condition that never holds fails loudly)


def test_stream_places_reads_by_phase():
    w = w2.shift_world()
    for r in w.notes["reads"]:
        assert (r["off"] + r["at"]) % 16 == r["phase"]
        assert w.stream[r["off"]:r["off"] + len(r["laid"]) + 1] == r["laid"] + b"\n" and w.stream[r["off"] - 1] == 10
    assert len(w.stream) % w2.TILE == w2.TAIL and len(w.stream) > 3 * w2.TILE


# ---- shift --------------------------------------------------------------------------------------------------------------------------------
def test_shift_world():
    """512 reads, every kind at every place of a chunk from both strands behind a short and a long near side.  Power: behind its
    breakpoint every read has at least 150 - 30 - 2 windows that are k-mers of the strain and hold a base that differs from the
    text on the near side's diagonal (the far side's first base, the read's first off-diagonal one, opens the first of them) --
    a substitution gives no such window.  The oracle counts exactly what the construction plans."""
    w = w2.shift_world()
    g, kset, reads = w.strains[0][0], w.ksets[0], w.notes["reads"]
    assert w2.canonical_16mers_distinct(g)
    assert len(reads) == 16 * 2 * len(w2.SHIFT_KINDS) * len(w2.SHIFT_NEAR) == 512
    assert {(r["kind"], r["near"], r["phase"], r["rev"]) for r in reads} == \
        {(k, n, p, v) for k in w2.SHIFT_KINDS for n in w2.SHIFT_NEAR for p in range(16) for v in (False, True)}
    assert w2.SHIFT_NEAR[0] // 16 + 1 < w2.ANCHOR_CH <= w2.SHIFT_NEAR[1] // 16 - 2     # one seed before the breakpoint / a later one too
    for r in reads:
        read, a, bp, far0 = r["read"], r["a"], r["bp"], r["far0"]
        assert read[:bp] == g[a - r["near"]:a] and read[bp] != g[a]                # the first off-diagonal base
        assert len(read) - far0 == w2.SHIFT_FAR
        off_diagonal = {i for i in range(bp, len(read)) if a + i - bp >= len(g) or read[i] != g[a + i - bp]}
        planted = [i for i in range(far0, len(read) - K + 1) if read[i:i + K] in kset and off_diagonal & set(range(i, i + K))]
        assert len(planted) >= w2.SHIFT_FAR - 30 - 2, (r["kind"], len(planted))
        assert sum(x in kset for x in w2.windows(read)) == r["planted"], r["kind"]  # no window extends across the breakpoint by accident
        assert not any(read[i:i + K] in kset for i in range(bp - K + 1, far0) if i + K > bp)
    plan = sum(r["planted"] for r in reads)
    assert plan == 256 * (70 + 120) + 256 * (170 + 120)
    assert w2.model_total(w.stream, kset) == plan
    assert _oracle_total(w) == plan
    assert _oracle_total(w, 1) > 0                                                # the union's second member: half the strain


# ---- ends ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", w2.ENDS_LENGTHS)
def test_ends_world(L):
    """the reads' windows are all the oracle counts: every read holds its piece's windows and no other.  Power, for strains of at
    least 48 bases, by the kernel's own arithmetic: among the chunks that hold a window of the strain there is, along the strain and
    against it, one whose 48 bases lie wholly inside the text, one whose 48 start below position 0, one whose 48 end beyond it"""
    w = w2.ends_world(L)
    g, reads = w.strains[0][0], w.notes["reads"]
    assert len(g) == L and len(reads) == 64 * len(w2.end_pieces(L))
    plan = sum(r["b"] - r["a"] - 30 for r in reads)
    assert w2.model_total(w.stream, w.ksets[0]) == plan and _oracle_total(w) == plan > 0
    cases = set()
    for r in reads:
        assert (_synth.revcomp(r["laid"]) if r["rev"] else r["laid"])[r["lo"]:r["hi"]] == g[r["a"]:r["b"]]
        for against, tq in w2.chunk_triples(r, L):
            cases.add((against, "below" if tq < 0 else "beyond" if tq + 48 > L else "inside"))
    if L >= 48:
        assert cases == {(d, c) for d in (False, True) for c in ("inside", "below", "beyond")}, sorted(cases)
    else:
        assert not any(c == "inside" for _, c in cases)                           # (the text stage can verify nothing: all one by one)


def test_chunk_triples_by_hand():
    """a 48-base strain read whole at stream offset 32 (its windows start at 32..49): chunk 3 (windows that start at 33..48) has its
    48 bases at 32..79, the text's 0..47; chunk 2 (17..32) has them 16 bases before the text, chunk 4 (49..64) 16 behind"""
    r = dict(off=32, lo=0, hi=48, a=0, b=48, rev=False)
    assert w2.chunk_triples(r, 48) == [(False, -16), (False, 0), (False, 16)]
    r["rev"] = True                                                              # against: the window at 32 is the text's at 17; the same chunks
    assert w2.chunk_triples(r, 48) == [(True, 16), (True, 0), (True, -16)]


@pytest.mark.parametrize("pair", w2.ENDS_UNIONS)
def test_ends_union_world(pair):
    """a read that runs off one member's end into the next one's start, as the members stand end to end and as the union's text
    holds them (zeros, read as A, fill each member's share): the windows across the seam are keys of no member, the windows of
    either side are, and each member's own end reads are there"""
    w = w2.ends_union_world(pair)
    assert [len(s[0]) for s in w.strains] == list(pair)
    crossers = w2.seam_crossers(w)
    assert len(crossers) >= 2 * 30 and not any(x in ks for x in crossers for ks in w.ksets)
    (bare, n1, at2), (padded, _, at2p) = w.notes["seams"]
    g1, g2 = w.strains[0][0], w.strains[1][0]
    assert bare == g1[-40:] + g2[:40] and padded[n1:at2p] == b"A" * w2.union_pad(len(g1)) and 64 <= at2p - n1 < 128
    assert (len(g1) + at2p - n1) % 64 == 0
    for m, g in enumerate((g1, g2)):
        plan = sum(r["b"] - r["a"] - 30 for r in w.notes["reads"][m]) + 2 * 32 * (min(40, len(g)) - 30)
        assert w2.model_total(w.stream, w.ksets[m]) == plan and _oracle_total(w, m) == plan > 0


# ---- seams --------------------------------------------------------------------------------------------------------------------------------
def test_seams_world():
    """reads that equal the 2-bit text across a record junction or an N.  The crossing windows are keys nowhere (all three junction
    reads have some) -- but in the X N Y strains the windows of X[-20:] b Y[:20] are keys where variant b holds them again"""
    w = w2.seams_world()
    recs = w.strains[0]
    assert [len(r) for r in recs] == list(w2.SEAM_RECORDS)
    text = b"".join(recs)
    nowhere = 0
    for read in w.notes["junctions"]:
        assert read in text and not any(read in r for r in recs)
        miss = [x for x in w2.windows(read) if x not in w.ksets[0]]
        assert len(miss) >= 30                                                    # (every window across the junction)
        nowhere += 1
    assert nowhere >= 3
    elsewhere = 0
    for v, c in enumerate(b"ACGT"):
        (strain,) = w.strains[1 + v]
        x, y = strain[:200], strain[201:401]
        assert strain[200:201] == b"N" and strain.endswith(x[-20:] + bytes([c]) + y[:20]) and len(strain) == 200 + 1 + 200 + 300 + 41
        for b, read in zip(b"ACGT", w.notes["ns"]):
            assert read == x[-40:] + bytes([b]) + y[:40]
            across = [read[i:i + K] for i in range(10, 41)]                       # the windows that hold the base at the N's place
            keys = [q for q in across if q in w.ksets[1 + v]]
            assert len(keys) == (11 if b == c else 0)
            elsewhere += b == c
            assert sum(q in w.ksets[1 + v] for q in w2.windows(read)) == 20 + len(keys)
    assert elsewhere == 4
    want = [w2.model_total(w.stream, ks) for ks in w.ksets]
    assert want[0] > 0 and want[1:] == [32 * (4 * 20 + 11)] * 4
    assert [_oracle_total(w, m) for m in range(5)] == want
    for m in range(1, 5):                                                         # counted at their real rows: those of the later place
        keys, col = w.count_refs[m]
        later = {min(q, _synth.revcomp(q)) for q in w2.windows(w.strains[m][0][-41:])}
        rows = [i for i, k in enumerate(keys) if min(k, _synth.revcomp(k)) in later]
        assert len(rows) == 11 and (col[rows] == 32).all()


# ---- runs ---------------------------------------------------------------------------------------------------------------------------------
def test_runs_world():
    """three 31-mers twice (the second copies at 0, 15 and 7 modulo 16: the hole in the rank bits on a chunk's first window, its last,
    an inner one -- at every phase of the reads over them).  One tile holds 150-base reads of two rows' indices over 200 times, and
    another over 200 different ones: more than 256 indices for the tile's table of 256"""
    w = w2.runs_world()
    g, stream = w.strains[0][0], w.stream
    assert [p % 16 for _, p in w2.RUNS_REPEATS] == [0, 15, 7]
    for a, p in w2.RUNS_REPEATS:
        assert g[a:a + K] == g[p:p + K] and a < p
    keys, col = w.count_refs[0]
    assert len(keys) == len(g) - 30 - 3                                          # a repeat has no row of its own
    for (seam, phase) in w2.RUNS_SEAMS:
        (off, read), = [f for f in w.notes["fixed"] if f[0] == seam - 208 + phase]
        assert off % 16 == phase and off < seam - 150 and off + 400 > seam + 150 and stream[off:off + 401] == read + b"\n"
        assert seam % 8192 == 0 and read in g
    assert sum(s % w2.TILE == 0 for s, _ in w2.RUNS_SEAMS) == 6 and {p for _, p in w2.RUNS_SEAMS} == {0, 1, 15}
    for (off, n), reads in ((w2.RUNS_SAME, [w.notes["same"]] * w2.RUNS_SAME[1]), (w2.RUNS_DIFFERENT, w.notes["different"])):
        assert len(reads) == n and stream[off - 1] == 10 and stream[off:off + 151 * n] == b"".join(r + b"\n" for r in reads)
        tile = off // w2.TILE
        inside = [r for i, r in enumerate(reads) if (off + 151 * i) // w2.TILE == tile == (off + 151 * i + 150) // w2.TILE]
        assert len(inside) > 200                                                 # (a tile holds 217 records of 151 bytes: the rest is in the next)
        if len(set(reads)) > 1:
            assert len(set(inside)) == len(inside) and 2 * len(inside) > 256     # a first and a behind-the-last index each
    assert w2.model_total(stream, w.ksets[0]) == _oracle_total(w) > 100000
    first, last = min(g[:K], _synth.revcomp(g[:K])), min(g[-K:], _synth.revcomp(g[-K:]))
    rows = {min(k, _synth.revcomp(k)): i for i, k in enumerate(keys)}
    assert col[rows[first]] >= 6 and col[rows[last]] >= 6                       # the text's first and last k-mer: the rank map's first and last row


# ---- the difference array -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nrows", w2.DIFF_NROWS)
def test_diff_strains_have_the_rows_asked_for(nrows):
    _, g = w2.diff_strain(nrows)
    assert len(g) == nrows + 30 and len(w2.kmer_set([g])) == 2 * nrows
