"""Worlds for stage 2 of the scan kernel (sk_scan_grid from "Seed and verify, a CHUNK per lane" on), the set
model their premises are checked with, and the runner that takes a world through every form of the kernel.  TEST INFRASTRUCTURE,
imported by tests/test_stage2_worlds_host.py (premises, no GPU), tests/test_stage2_worlds_gpu.py and tests/test_quarter_shift_gpu.py.

Stage 2 seeds one table probe per stretch of surviving chunks, compares each chunk's 48 bases with the strain's 2-bit text on the
seed's diagonal, turns verified windows into rows through the rank map and counts runs of rows.  Random reads with substitutions
cannot show a mistake in four places of it, and each world here is built around one of them:

  shift   reads that leave the seed's diagonal for another one (deletions, insertions, jumps, the other strand): the windows behind
          the breakpoint mismatch on the diagonal AND are k-mers of the strain, so rejecting one too many is a wrong count
  ends    strains of 31..129 bases (and one of 4000) read at every phase from both strands, whole and by their ends: the 48 bases
          of a chunk lie across position 0 or across the text's end, and text lengths sit on 16- and 64-base boundaries
  seams   reads that equal the 2-bit text where it is no k-mer of the strain: across the junction of two records, and with the
          stored code at an N's place; in four variants of the strain the crossing k-mer also exists elsewhere as a real key
  runs    (COUNT) repeats that split a run of rows at a chunk's first, last and an inner window, a neighbour chunk on another
          diagonal, the same indices and more than 256 of them in one tile's table of indices, runs across wave and tile seams

A world is strains, a record stream of whole 32 KiB tiles and a ragged tail of 11 bytes, and what was planted where."""
import functools
import random

import numpy as np

import _oracle
import _synth
import _tally_ref as tr

K = 31
TILE = 32768
TAIL = 11
SLOTS = 16384                          # first size of the tables on both sides (the row order follows it)
REDRAWS = 20
ANCHOR_CH = 8                          # SK_ANCHOR_CH: one seed per this many chunks of a stretch


class Stream:
    """a record stream laid out by offset: reads at chosen places, random records (no strain) between them"""

    def __init__(self, rng, size=None):
        self.rng, self.buf, self.size = rng, bytearray(), size

    def fill_to(self, off):
        gap = off - len(self.buf)
        assert gap == 0 or gap >= 2, (off, len(self.buf))
        while gap:
            n = min(gap, self.rng.randrange(42, 122))
            if gap - n == 1:
                n -= 1
            self.buf += _synth.rand_dna(self.rng, n - 1) + b"\n"
            gap -= n

    def at(self, off, read):
        self.fill_to(off)
        self.buf += read + b"\n"
        return off

    def at_phase(self, phase, read, at=0):
        """the read's base `at` lands on a stream offset that is `phase` modulo 16"""
        phase = (phase - at) % 16
        off = len(self.buf) + (phase - len(self.buf)) % 16
        return self.at(off + 16 if off - len(self.buf) == 1 else off, read)

    def done(self):
        """filled up to the size given, or to the next whole tile and a ragged tail"""
        size = self.size
        if size is None:
            size = -(-(len(self.buf) + 2) // TILE) * TILE + TAIL
        self.fill_to(size)
        return bytes(self.buf)


def other(rng, *not_these):
    return bytes([rng.choice(sorted(set(b"ACGT") - set(not_these)))])


def comp(b):
    return _synth.revcomp(bytes([b]))[0]


def type_col(informative):
    t = np.ones(len(informative), dtype=np.uint32)
    t[informative] = 2
    return t


# ---- the set model ------------------------------------------------------------------------------------------------------------------------
def kmer_set(records):
    """every 31-mer of the strain's records, either strand (a record is cut where it holds a byte that is no base)"""
    s = set()
    for r in records:
        run = 0
        for i, b in enumerate(r):
            run = run + 1 if b in b"ACGT" else 0
            if run >= K:
                w = r[i - K + 1:i + 1]
                s.add(w)
                s.add(_synth.revcomp(w))
    return s


def windows(read):
    return [read[i:i + K] for i in range(len(read) - K + 1)]


def model_total(stream, kset):
    return sum(w in kset for rec in stream.split(b"\n") for w in windows(rec))


def canonical_16mers_distinct(g):
    seen = set()
    for i in range(len(g) - 15):
        w = g[i:i + 16]
        w = min(w, _synth.revcomp(w))
        if w in seen:
            return False
        seen.add(w)
    return True


def canonical_kmers_distinct(g):
    ws = windows(g)
    return len({min(w, _synth.revcomp(w)) for w in ws}) == len(ws)


def redraw(seed, draw, ok):
    """draw(random.Random(seed + i)) for the first i <= REDRAWS whose draw passes ok; returns (i, the draw)"""
    for i in range(REDRAWS + 1):
        x = draw(random.Random(seed + i))
        if ok(x):
            return i, x
    raise AssertionError(f"no draw passed its condition in {REDRAWS} redraws from seed {seed}")


def flanked(rng, g, a, b, n=20):
    """g[a:b] behind and before n random bases; the bases next to it continue the strain on neither strand"""
    l, r = (g[a - 1],) if a else (), (g[b],) if b < len(g) else ()
    head = _synth.rand_dna(rng, n - 1) + other(rng, *l, *map(comp, r))
    tail = other(rng, *r, *map(comp, l)) + _synth.rand_dna(rng, n - 1)
    return head + g[a:b] + tail


class World:
    """strains (each a list of records), the stream, and what the builder noted about its reads"""

    def __init__(self, name, strains, stream, notes=None, redraws=0):
        assert stream.endswith(b"\n") and (len(stream) - TAIL) % TILE == 0, len(stream)
        self.name, self.strains, self.stream, self.notes, self.redraws = name, strains, stream, notes or {}, redraws
        self.sstreams = [b"\n".join(recs) + b"\n" for recs in strains]
        self.starts = np.array([0] + [i + 1 for i in range(len(stream) - 1) if stream[i] == 10], dtype=np.uint32)
        assert (np.diff(self.starts) >= 2).all()

    @functools.cached_property
    def ksets(self):
        return [kmer_set(recs) for recs in self.strains]

    @functools.cached_property
    def count_refs(self):
        """per strain: (the oracle's keys in row order, its COUNT column of the stream)"""
        out = []
        for ss in self.sstreams:
            t = _oracle.OracleTable(capacity=SLOTS)
            assert t.build_stream(ss, default=1, incr=0, short_policy=1) == 0
            t.scan_stream(self.stream, 1)
            keys, counts = t.rows()
            want = counts[:, 1].copy()
            want.setflags(write=False)
            t.close()
            out.append((keys, want))
        return out

    @functools.cached_property
    def tally_refs(self):
        """per strain: (tally reference, oracle strain, informative rows)"""
        out = []
        for ss in self.sstreams:
            o = tr.OracleStrain(ss, capacity=SLOTS)
            informative = np.arange(o.nrows) % 5 == 0
            out.append((o.tally(self.stream, self.starts, informative), o, informative))
        return out


# ---- world `shift` ------------------------------------------------------------------------------------------------------------------------
SHIFT_KINDS = ("del1", "del2", "del3", "del16", "ins1", "ins2", "jump", "flip")
SHIFT_NEAR = (100, 200)                # fewer than ANCHOR_CH chunks before the breakpoint (one seed, the wrong one behind it), and more
SHIFT_FAR = 150


def shift_read(rng, g, a, near, kind):
    """(g[a-near:a] and what the strain holds behind a shift of `kind`, the index of the first base behind the breakpoint, the
    index of the first of the SHIFT_FAR strain bases of the far side), or None where a base next to the breakpoint would let a
    window extend across it: the far side's first base is not g[a], and the base the far side's diagonal expects before it is
    not g[a-1] (as _window_read of tests/test_quarter_shift_gpu.py chooses its flanks)"""
    head = g[a - near:a]
    if kind.startswith("ins"):
        n = int(kind[3:])
        ins = other(rng, g[a], g[a - 1]) if n == 1 else other(rng, g[a]) + other(rng, g[a - 1])
        return head + ins + g[a:a + SHIFT_FAR], near, near + n
    if kind.startswith("del"):
        b = a + int(kind[3:])
        far, before = g[b:b + SHIFT_FAR], g[b - 1]
    else:
        b = a + 1200 if a < 2000 else a - 1400                         # more than 1 kbp away
        far, before = (g[b:b + SHIFT_FAR], g[b - 1]) if kind == "jump" else (_synth.revcomp(g[b:b + SHIFT_FAR]), comp(g[b + SHIFT_FAR]))
    if far[0] == g[a] or before == g[a - 1]:
        return None
    return head + far, near, near


def shift_reads(rng, g):
    """the 512 reads: (read as laid into the stream, index of its base that goes to the phase, planted windows, the read as
    constructed, index of its first off-diagonal base, index of its far side's first strain base, a, near, kind)"""
    out, n = [], 0
    for near in SHIFT_NEAR:
        for kind in SHIFT_KINDS:
            for phase in range(16):
                for rev in (False, True):
                    a = 250 + (211 * n) % 3300
                    n += 1
                    while True:
                        r = shift_read(rng, g, a, near, kind)
                        if r:
                            break
                        a += 1
                    read, bp, far0 = r
                    laid, at = (_synth.revcomp(read), len(read) - bp) if rev else (read, bp)
                    out.append(dict(laid=laid, at=at, phase=phase, planted=near - 30 + SHIFT_FAR - 30, read=read, bp=bp, far0=far0,
                                    a=a, near=near, kind=kind, rev=rev))
    return out


def _strain_pair(rng, n=4000):
    g = _synth.rand_dna(rng, n)
    return g, g[:n // 2] + _synth.rand_dna(rng, n - n // 2)


@functools.lru_cache(maxsize=None)
def shift_world():
    redraws, (g, g2) = redraw(5100, _strain_pair, lambda x: canonical_16mers_distinct(x[0]))
    rng = random.Random(5150)
    s = Stream(rng)
    reads = shift_reads(rng, g)
    for r in reads:
        r["off"] = s.at_phase(r["phase"], r["laid"], at=r["at"])
    return World("shift", [[g], [g2]], s.done(), {"reads": reads}, redraws)


# ---- world `ends` -------------------------------------------------------------------------------------------------------------------------
ENDS_LENGTHS = (31, 32, 47, 48, 49, 63, 64, 65, 79, 80, 95, 96, 111, 112, 127, 128, 129, 4000)


def end_pieces(L):
    """the pieces of a strain of L bases that its reads are made of: the whole, and from 80 bases on its first and last 60"""
    return [(0, L)] + ([(0, 60), (L - 60, L)] if L >= 80 else [])


def ends_reads(rng, g, whole=True):
    """every piece bare and flanked, at 16 phases, from both strands: dicts with the read as laid into the stream, where in it the
    piece lies, and where in the strain"""
    out = []
    for a, b in end_pieces(len(g)):
        if not whole and (a, b) == (0, len(g)) and len(g) >= 80:
            continue
        for flank in (0, 20):
            for phase in range(16):
                for rev in (False, True):
                    read = flanked(rng, g, a, b, flank) if flank else g[a:b]
                    out.append(dict(laid=_synth.revcomp(read) if rev else read, phase=phase, lo=flank, hi=flank + b - a, a=a, b=b, rev=rev))
    return out


def ends_strain(L):
    return _synth.rand_dna(random.Random(5200 + L), L)


@functools.lru_cache(maxsize=None)
def ends_world(L):
    g = ends_strain(L)
    rng = random.Random(5300 + L)
    s = Stream(rng)
    reads = ends_reads(rng, g)
    for r in reads:
        r["off"] = s.at_phase(r["phase"], r["laid"])
    return World(f"ends{L}", [[g]], s.done(), {"reads": reads})


def chunk_triples(r, L):
    """the kernel's arithmetic for a placed read of ends_reads: for every chunk that holds a window of the strain piece, (whether the
    read runs against the strain, tq = the lowest text position of the 48 bases of chunks ch-1, ch, ch+1 on the seed's diagonal).
    x0 = ch*16 - 16; along the strain a window at stream offset xs and text position tp gives the diagonal D = tp - xs and
    tq = D + x0, against it D = tp + 30 + xs and tq = D - x0 - 47 (sk_scan_grid; offsets relative to any tile: they cancel)."""
    first, last = r["off"] + r["lo"], r["off"] + r["hi"] - K          # stream offsets of the piece's first and last window
    if last < first:
        return []
    if not r["rev"]:
        dg = r["a"] - first                                            # the window at `first` is the text's at a
    else:
        dg = (r["b"] - K) + 30 + first                                 # the window at `first` is the text's last one of the piece
    out = []
    for ch in range((first + 15) // 16 - 1, (last + 15) // 16 + 1):
        if any(first <= ch * 16 - 15 + j <= last for j in range(16)):  # window j of chunk ch starts 15 - j bases before the chunk
            x0 = ch * 16 - 16
            out.append((r["rev"], dg - x0 - 47 if r["rev"] else dg + x0))
    return out


def union_pad(n):
    """bases of code 0 between a member's text of n bases and the next member's in a union's text (sk_union_create: each member's
    share is n rounded up to whole rank blocks of 64, and one block more)"""
    return (n + 63) // 64 * 64 + 64 - n


ENDS_UNIONS = ((47, 4000), (4000, 47), (4000, 129), (129, 4000))


def _ends_union(pair):
    def draw(rng):
        g1, g2 = _synth.rand_dna(rng, pair[0]), _synth.rand_dna(rng, pair[1])
        s = Stream(rng)
        seams = []
        for mid in (b"", b"A" * union_pad(len(g1))):                  # the members end to end, and as the union's text holds them
            read = g1[-40:] + mid + g2[:40]
            for phase in range(16):
                for rev in (False, True):
                    s.at_phase(phase, _synth.revcomp(read) if rev else read)
            seams.append((read, min(40, len(g1)), len(read) - min(40, len(g2))))
        reads = [ends_reads(rng, g, whole=False) for g in (g1, g2)]
        for rs in reads:
            for r in rs:
                r["off"] = s.at_phase(r["phase"], r["laid"])
        return World("ends%d+%d" % pair, [[g1], [g2]], s.done(), {"seams": seams, "reads": reads})
    return draw


def seam_crossers(w):
    """the windows of a union world's seam reads that lie in neither side alone"""
    out = []
    for read, n1, at2 in w.notes["seams"]:
        out += [read[i:i + K] for i in range(len(read) - K + 1) if i + K > n1 and i < at2]
    return out


@functools.lru_cache(maxsize=None)
def ends_union_world(pair):
    def ok(w):
        return not any(x in ks for x in seam_crossers(w) for ks in w.ksets)
    redraws, w = redraw(5400 + 7 * ENDS_UNIONS.index(pair), _ends_union(pair), ok)
    w.redraws = redraws
    return w


# ---- world `seams` ------------------------------------------------------------------------------------------------------------------------
SEAM_RECORDS = (200, 31, 45, 300)


@functools.lru_cache(maxsize=None)
def seams_world():
    """strain 0: four records; strains 1..4: X N Y Z X[-20:] c Y[:20] for c = A, C, G, T -- for one of them the text holds c at the
    N's place, and in each the k-mers of X[-20:] c Y[:20] are real keys at the later place"""
    rng = random.Random(5500)
    recs = [_synth.rand_dna(rng, n) for n in SEAM_RECORDS]
    X, Y, Z = (_synth.rand_dna(rng, n) for n in (200, 200, 300))
    strains = [recs] + [[X + b"N" + Y + Z + X[-20:] + bytes([c]) + Y[:20]] for c in b"ACGT"]
    text = b"".join(recs)
    s = Stream(rng)
    junctions, ns = [], []
    at = 0
    for n in SEAM_RECORDS[:-1]:
        at += n
        junctions.append(text[at - 40:at + 40])
    for b in b"ACGT":
        ns.append(X[-40:] + bytes([b]) + Y[:40])
    for read in junctions + ns:
        for phase in range(16):
            for rev in (False, True):
                s.at_phase(phase, _synth.revcomp(read) if rev else read)
    return World("seams", strains, s.done(), {"junctions": junctions, "ns": ns})


# ---- world `runs` -------------------------------------------------------------------------------------------------------------------------
RUNS_REPEATS = ((300, 1008), (1300, 2015), (2300, 3015))              # (first copy, second copy: its place is 0, 15 and 7 modulo 16)
RUNS_SEAMS = ((8192, 0), (16384, 0), (TILE, 0), (2 * TILE, 0), (24576, 1), (TILE + 8192, 1), (TILE + 16384, 15), (TILE + 24576, 15),
              (3 * TILE, 1), (5 * TILE, 1), (7 * TILE, 15), (8 * TILE, 15))   # (a wave's or a tile's seam, the phase of the read's start)
RUNS_SAME, RUNS_DIFFERENT = (3 * TILE + 256, 400), (5 * TILE + 256, 300)       # (where the block of 150-base reads starts, how many)


def _runs_strain(rng):
    g = bytearray(_synth.rand_dna(rng, 4000))
    for a, p in RUNS_REPEATS:
        g[p:p + K] = g[a:a + K]
        g[p - 1], g[p + K] = other(rng, g[a - 1])[0], other(rng, g[a + K])[0]    # (the repeat is these 31 bases and no more)
    return bytes(g)


def _runs_strain_ok(g):
    ws = [min(w, _synth.revcomp(w)) for w in windows(g)]
    return len(set(ws)) == len(ws) - len(RUNS_REPEATS)                # the planted k-mers twice, every other one once


@functools.lru_cache(maxsize=None)
def runs_world():
    redraws, g = redraw(5600, _runs_strain, _runs_strain_ok)
    rng = random.Random(5650)
    both = lambda r: (r, _synth.revcomp(r))
    floating = []                                                      # (phase or None, read)
    for n in (64, 79, 80, 81, 400):                                    # 1: exact copies over each planted repeat (its second copy: the hole)
        for _, p in RUNS_REPEATS:
            for phase in range(16):
                a = min(max(p + 15 - n // 2, 0), len(g) - n)
                for r in both(g[a:a + n]):
                    floating.append((phase, r))
    for near in SHIFT_NEAR:                                            # 2: a 16-base deletion: consecutive chunks, another diagonal
        for phase in range(16):
            a = 400 + 97 * phase + near
            while shift_read(rng, g, a, near, "del16") is None:
                a += 1
            read, bp, _ = shift_read(rng, g, a, near, "del16")
            floating += [(phase - bp, read), (phase - (len(read) - bp), _synth.revcomp(read))]
    for _ in range(3):                                                 # 5: runs that end behind the last row, and begin at the first
        for r in both(g[-80:]) + both(g[:80]):
            floating.append((None, r))
    fixed = []
    for seam, phase in RUNS_SEAMS:                                     # 4: a 400-base read across a seam
        a = 100 + 250 * len(fixed)
        fixed.append((seam - 208 + phase, g[a:a + 400]))
    same = g[1500:1650]
    fixed.append((RUNS_SAME[0], b"\n".join([same] * RUNS_SAME[1])))    # 3: the same two indices over and over in a tile
    different = [g[10 * i + 7:10 * i + 157] for i in range(RUNS_DIFFERENT[1])]
    fixed.append((RUNS_DIFFERENT[0], b"\n".join(different)))           #    and more indices than the table holds
    long = g[500:3500]
    fixed.append((8 * TILE + 512, long + b"\n" + _synth.revcomp(long)))   # 4: stretches longer than a round of 64 chunks
    fixed.sort()
    s = Stream(rng)
    floating.reverse()
    for off, read in fixed + [(None, None)]:                           # the reads without a place of their own go between the others
        while floating and (off is None or len(s.buf) + 20 + len(floating[-1][1]) + 3 <= off):
            phase, r = floating.pop()
            if phase is None:
                s.at(len(s.buf), r)
            else:
                s.at_phase(phase % 16, r)
        if off is not None:
            s.at(off, read)
    return World("runs", [[g]], s.done(), {"same": same, "different": different, "fixed": fixed}, redraws)


# ---- the difference array's geometry ------------------------------------------------------------------------------------------------------
DIFF_NROWS = (1, 2, 4094, 4095, 4096, 4097, 8191, 8192, 8193)         # nrows + 1 entries around multiples of SK_DIFF_PER_BLOCK (4096)


@functools.lru_cache(maxsize=None)
def diff_strain(nrows):
    """(redraws, a random strain of nrows + 30 bases whose k-mers are all distinct as canonical keys)"""
    return redraw(5700 + nrows, lambda rng: _synth.rand_dna(rng, nrows + K - 1), canonical_kmers_distinct)


# ---- a world in every form ----------------------------------------------------------------------------------------------------------------
def device_buildable(w):
    """every strain of the world holds only what build_from_text takes: A/C/G/T/N in either case (no U, no IUPAC letter)"""
    return all(set(r) <= set(b"ACGTNacgtn") for recs in w.strains for r in recs)


def run_built_on_the_device(w, main=0, tally=True, union=True):
    """the form "built on the device": every table comes from build_from_text(records) -- the builder's own text, rank map, orientation
    bits and filters, rows in strain order and no row permutation on the device (d_inv == NULL in the union's resolve step and in
    sk_first_pos_from_rank).  Counts and logged rows are taken to the oracle's rows by key.  COUNT, the host-packed form, resident
    twice (both lanes), one TALLY launch; union: the TALLY launch of a union whose members were ALL built on the device."""
    import _build_model as bm
    import strainer2_amd as sk
    assert device_buildable(w)
    stream, starts = w.stream, w.starts
    packed, odd = sk.pack_stream(stream)
    assert not odd
    members = range(len(w.strains)) if union else [main]
    ctxs, orow = {}, {}
    try:
        for m in members:
            c = sk.KmerContext(0)
            ctxs[m] = c
            n = c.build_from_text(w.strains[m], 6, 1)
            okeys = w.count_refs[m][0]
            dev = bm.key_bytes(bm.exported_keys(c))
            row_of = {k: i for i, k in enumerate(okeys)}
            assert n == len(okeys) == len(row_of) and sorted(dev) == sorted(okeys), (w.name, m, "the device's key set is not the oracle's")
            orow[m] = np.array([row_of[k] for k in dev], dtype=np.int64)      # the oracle's row of every row of the device
            assert (np.diff(c.first_pos().astype(np.int64)) > 0).all()
            if tally:
                c.set_counts(0, type_col(w.tally_refs[m][2])[orow[m]])
        c, want = ctxs[main], w.count_refs[main][1].astype(np.int64)[orow[main]]

        def same(got, what, times=1):
            assert np.array_equal(got, times * want), (w.name, "built on the device", what, np.nonzero(got != times * want)[0][:10])

        c.scan_stream(stream, 1)
        same(c.counts(1), "COUNT")
        buf = c.dev_alloc(len(packed))
        c.dev_upload(buf, packed)
        c.scan_device_packed(buf, len(stream), 2)
        c.sync()
        c.dev_free(buf)
        same(c.counts(2), "PACKED")
        buf = c.dev_alloc(len(stream))
        c.dev_upload(buf, np.frombuffer(stream, dtype=np.uint8))
        c.scan_device(buf, len(stream), 3)
        c.scan_device(buf, len(stream), 3)
        c.sync()
        c.dev_free(buf)
        same(c.counts(3), "RESIDENT twice", 2)
        if tally:
            ref, o, _ = w.tally_refs[main]
            t, h = c.tally_batch(stream, starts, 0, 2)
            h = np.stack([h[:, 0].astype(np.int64), orow[main][h[:, 1]]], axis=1) if len(h) else h
            tr.check_single(o, stream, starts, ref, t, h, (w.name, "built on the device", "TALLY"))
        if union:
            with sk.KmerUnion([ctxs[m] for m in members], 0, 2) as u:
                t, h = u.tally_batch(stream, starts)
                for m in members:
                    ref, o, _ = w.tally_refs[m]
                    hm = h[h[:, 0] == m][:, 1:].astype(np.int64)
                    hm[:, 1] = orow[m][hm[:, 1]]
                    tr.check_single(o, stream, starts, ref, t[:, m, :], hm, (w.name, "built on the device", "UNION", m))
    finally:
        for c in ctxs.values():
            c.close()


def run_every_form(w, main=0, tally=True, union=True, built="host"):
    """world w's stream against its strain `main`: COUNT with text_stage 1 and 0, pipeline 2, resident on the device (scanned twice:
    both lanes see it), the host-packed form on the device; tally: one TALLY launch; union: the TALLY launch of a union of all
    the world's strains, each member credited exactly.  text_stage 0 uses none of stage 2's text and rank map: the control.
    built="device": the form run_built_on_the_device, whose tables the device builds itself, instead of these."""
    if built == "device":
        return run_built_on_the_device(w, main, tally, union)
    assert built == "host"
    import strainer2_amd as sk
    stream, starts = w.stream, w.starts
    packed, odd = sk.pack_stream(stream)
    assert not odd
    members = range(len(w.strains)) if union else [main]
    ctxs, sets = {}, {}
    try:
        for m in members:
            ks = sk.Keyset.from_stream(w.sstreams[m], initial_slots=SLOTS, default_val=1, incr=0)
            sets[m] = ks
            assert ks.keys() == w.count_refs[m][0], "row order differs from the oracle"
            c = sk.KmerContext(0)
            ctxs[m] = c
            c.load_keyset(ks, 6)
            if tally:
                c.set_counts(0, type_col(w.tally_refs[m][2]))
        c, want = ctxs[main], w.count_refs[main][1]

        def same(got, what, times=1):
            assert np.array_equal(got, times * want.astype(np.int64)), (w.name, what, np.nonzero(got != times * want)[0][:10])

        with sk.KmerContext(0) as c0:                                  # the control first: a world the oracle and the plain path disagree on is wrong itself
            c0.set_option("text_stage", 0)
            c0.load_keyset(sets[main], 4)
            c0.scan_stream(stream, 1)
            same(c0.counts(1), "COUNT text_stage 0")
        c.scan_stream(stream, 1)
        same(c.counts(1), "COUNT")
        with sk.KmerContext(0) as c2:
            c2.set_option("pipeline", 2)
            c2.load_keyset(sets[main], 4)
            c2.scan_stream(stream, 1)
            same(c2.counts(1), "COUNT pipeline 2")
        buf = c.dev_alloc(len(packed))
        c.dev_upload(buf, packed)
        c.scan_device_packed(buf, len(stream), 2)
        c.sync()
        c.dev_free(buf)
        same(c.counts(2), "PACKED")
        buf = c.dev_alloc(len(stream))
        c.dev_upload(buf, np.frombuffer(stream, dtype=np.uint8))
        c.scan_device(buf, len(stream), 3)
        c.scan_device(buf, len(stream), 3)
        c.sync()
        c.dev_free(buf)
        same(c.counts(3), "RESIDENT twice", 2)
        if tally:
            ref, o, _ = w.tally_refs[main]
            t, h = c.tally_batch(stream, starts, 0, 2)
            tr.check_single(o, stream, starts, ref, t, h, (w.name, "TALLY"))
        if union:
            with sk.KmerUnion([ctxs[m] for m in members], 0, 2) as u:
                t, h = u.tally_batch(stream, starts)
                for m in members:
                    ref, o, _ = w.tally_refs[m]
                    tr.check_single(o, stream, starts, ref, t[:, m, :], h[h[:, 0] == m][:, 1:], (w.name, "UNION", m))
    finally:
        for c in ctxs.values():
            c.close()
        for k in sets.values():
            k.close()
