"""The scan's quarter-shifted level-1 question (sk_scan_grid; the rule and its model: tests/test_quarter_shift_model.py) on the GPU:
worlds built around the chunks it is asked about, in every form of the kernel, against the oracle.

A world is a stream of three 32 KiB tiles and a ragged tail of 11 bytes -- a first, an inner and a last tile, a halo on both sides --
over a strain of a few kbp; between the reads that matter lie random ones (whose chunks pass level 1 only by chance).  Window j of
a chunk has j bases left of it and 15 - j right of it (j >= 8: the side of the -8 / -4 questions, j <= 7: of the +8 / +4 ones).

  a      every j = 0..15: a read whose one strain window sits at j of a chunk, the rest of it random, at every phase 0..15 of the
         read's start, from both strands: 512 reads, 512 counted windows
  b      close misses: a strain 16-mer on the chunk and another at -8 or +8, and no strain 16-mer at -4 / +4 -- chimeras of the two
         places of an 8-mer the strain holds twice, and strain reads with one substituted base at every offset -12..27 of a chunk
  cn cu  a foreign byte at each of the 4 borrowed positions on either side of a chunk, next to a strain window that starts right
         behind it or ends right before it: N and a newline (cn), U (cu: the byte-string kernel's windows are part of the counts)
  d0..d3 the chunk at the first place of a tile and the chunk at the last place of one (their neighbour is the halo record), the
         stream's first chunk and its last whole one: world a's read for j = 0 and j = 15, either strand

Forms: COUNT with text_stage 1 and 0, the host-packed form on the device (scan_device_packed; not cu: a packed batch holds no byte
for the byte-string kernel), one TALLY launch, and the TALLY launch of a union of two strains (whose path keeps level 2 alone)."""
import functools
import random

import numpy as np
import pytest

import _oracle
import _synth
import _tally_ref as tr
import strainer2_amd as sk
from _stage2_worlds import Stream as _Stream, other as _other, type_col as _type_col
from test_quarter_shift_model import ACGT, _verdict

pytestmark = pytest.mark.gpu

TILE = 32768
SIZE = 3 * TILE + 11
SLOTS = 16384                          # first size of the tables on both sides (the row order follows it)
K = 31


def _window_read(rng, strain, a, pre, post, rev):
    """a read whose ONE strain window is strain[a:a+31] (reverse-complemented if rev), behind `pre` random bases and before `post`:
    the bases next to the window are neither strand's next base of the strain"""
    w = strain[a:a + K]
    l, r = strain[a - 1], strain[a + K]
    cl, cr = _synth.revcomp(bytes([l]))[0], _synth.revcomp(bytes([r]))[0]
    head = (_synth.rand_dna(rng, pre - 1) + _other(rng, l, cr)) if pre else b""
    tail = (_other(rng, r, cl) + _synth.rand_dna(rng, post - 1)) if post else b""
    return head + (_synth.revcomp(w) if rev else w) + tail


def _strains(rng):
    """the strain (4 kbp; twelve of its 8-mers occur twice) and a second one that shares half its text"""
    g = bytearray(_synth.rand_dna(rng, 4000))
    twice = []
    for i in range(12):
        a, b = 100 + 300 * i, 190 + 300 * i
        g[b:b + 8] = g[a:a + 8]
        twice.append((a, b))
    g = bytes(g)
    return g, g[:2000] + _synth.rand_dna(rng, 2000), twice


def _world_a(rng, g, twice, s):
    n = 0
    for j in range(16):
        for phase in range(16):
            for rev in (False, True):
                pre = 16 + (-j - phase) % 16                          # the window starts j bases before a chunk
                s.at_phase(phase, _window_read(rng, g, 40 + (37 * n) % 3900, pre, rng.randrange(17, 25), rev))
                n += 1
    return n


def _world_b(rng, g, twice, s):
    for rep in range(6):
        for a, b in twice:
            for x, y in ((a, b), (b, a)):
                for rev in (False, True):
                    # X P Y: up to P as at x, behind P as at y.  P begins a chunk (X P is its -8 question, left alone when Y is short)
                    # or lies 8 bases into one (P Y is its +8 question, left alone when X is short)
                    pre, post = rng.choice([8, 12, 20, 31]), rng.choice([8, 12, 20, 31])
                    r = g[x - pre:x + 8] + g[y + 8:y + 8 + post]
                    p_at = post if rev else pre
                    s.at_phase((rng.choice([0, 8]) - p_at) % 16, _synth.revcomp(r) if rev else r)
    for d in range(-12, 28):                                          # one substituted base at every place of a chunk, in a 90-base strain read
        for rev in (False, True):
            a = rng.randrange(100, 3800)
            r = bytearray(g[a:a + 90])
            r[40] = _other(rng, r[40])[0]
            r = bytes(r)
            at = 49 if rev else 40
            s.at_phase((d - at) % 16, _synth.revcomp(r) if rev else r)
    return 0


def _world_c(foreign):
    def build(rng, g, twice, s):
        for byte in foreign:
            for p in range(4):
                for side in ("left", "right"):
                    for rev in (False, True):
                        # a 31-base strain window that ends right before the byte (left: the byte is borrowed base p of the chunk
                        # behind the window's last whole chunk) or starts right behind it, within a longer strain read
                        a = rng.randrange(100, 3800)
                        r = bytearray(g[a:a + 80])
                        r[40] = byte
                        r = bytes(r)
                        at = 39 if rev else 40
                        want = (12 + p) if side == "left" else p       # place of the byte in its chunk
                        s.at_phase((want - at) % 16, _flip(r, byte) if rev else r)
        if foreign == b"U":                                           # windows with a U that hit for certain, the U at each of those places
            for p in range(4):
                for side in ("left", "right"):
                    w = None
                    while w is None:
                        w = _synth.u_window(rng, g)
                    i = w[0].upper().index(b"U")
                    s.at_phase(((12 + p if side == "left" else p) - i) % 16, w[0])
        return 0
    return build


def _flip(r, byte):
    """the reverse complement of a read that holds one foreign byte, which stays what it is"""
    i = r.index(bytes([byte]))
    return _synth.revcomp(r[i + 1:]) + bytes([byte]) + _synth.revcomp(r[:i])


def _world_d(j, rev):
    def build(rng, g, twice, s):
        n = 0
        if j == 0:                                                    # the stream's first chunk: the window starts the stream
            s.at(0, _window_read(rng, g, 500, 0, 20, rev))
            n += 1
        for chunk in (TILE, 3 * TILE - 16 - TILE):                    # first place of the inner tile; last place of the inner tile
            pre = 20
            s.at(chunk - j - pre, _window_read(rng, g, 900 + chunk % 1000, pre, 20, rev))
            n += 1
        if j == 15:                                                   # the last whole chunk: the window ends with the last tile
            s.at(3 * TILE - 16 - j - 20, _window_read(rng, g, 2500, 20, 0, rev))
            n += 1
        return n
    return build


_WORLDS = {"a": _world_a, "b": _world_b, "cn": _world_c(b"N\n"), "cu": _world_c(b"U"),
           **{f"d{k}": _world_d((0, 15)[k >> 1], bool(k & 1)) for k in range(4)}}


@functools.lru_cache(maxsize=None)
def _world(name):
    """(strains, stream, record starts, per strain: (COUNT column, tally reference, oracle strain, informative rows))"""
    rng = random.Random(4710 + sorted(_WORLDS).index(name))
    g, g2, twice = _strains(rng)
    s = _Stream(rng, SIZE)
    single = _WORLDS[name](rng, g, twice, s)
    stream = s.done()
    assert len(stream) == SIZE and stream.endswith(b"\n")
    starts = np.array([0] + [i + 1 for i in range(len(stream) - 1) if stream[i] == 10], dtype=np.uint32)
    assert (np.diff(starts) >= 2).all()
    refs = []
    for x in (g, g2):
        t = _oracle.OracleTable(capacity=SLOTS)
        assert t.build_stream(x + b"\n", default=1, incr=0, short_policy=1) == 0
        t.scan_stream(stream, 1)
        want = t.counts()[:, 1].copy()
        want.setflags(write=False)
        t.close()
        o = tr.OracleStrain(x + b"\n", capacity=SLOTS)
        informative = np.arange(o.nrows) % 5 == 0
        refs.append((want, o.tally(stream, starts, informative), o, informative))
    if single:
        assert int(refs[0][0].sum()) == single, "every planted read holds exactly one window of the strain"
    assert int(refs[0][0].sum()) > 0
    if name == "b":                                                   # power, by the model: chunks that only the quarter-shifted question prunes
        s16 = {g[i:i + 16] for i in range(len(g) - 15)}
        s16 |= {_synth.revcomp(w) for w in s16}
        padded = b"\n" * 16 + stream + b"\n" * 21
        n = 0
        for c in range(len(stream) // 16):
            prev, cw, nxt = (padded[16 * (c + d):16 * (c + d) + 16] for d in range(3))
            if not set(cw) - ACGT and cw in s16:
                al, ar, al8, ar8 = _verdict(prev, cw, nxt, s16.__contains__)
                n += (al8 or ar8) and not (al or ar)
        assert n >= 72, n                                             # (288 chimeras; half have a far side too short to pass on its own: a quarter at least)
    if name == "cu":                                                  # power: the windows that hold a U add to the counts
        t = _oracle.OracleTable(capacity=SLOTS)
        assert t.build_stream(g + b"\n", default=1, incr=0, short_policy=1) == 0
        t.scan_stream(stream.replace(b"U", b"N").replace(b"u", b"N"), 1)
        assert int(t.counts()[:, 1].sum()) + 8 <= int(refs[0][0].sum())
        t.close()
    return (g, g2), stream, starts, refs


@pytest.mark.parametrize("name", sorted(_WORLDS))
def test_world_in_every_form(name):
    strains, stream, starts, refs = _world(name)
    packed, odd = sk.pack_stream(stream)
    assert odd == (name == "cu")
    ctxs, sets = [], []
    try:
        for x, (want, _, o, informative) in zip(strains, refs):
            ks = sk.Keyset.from_stream(x + b"\n", initial_slots=SLOTS, default_val=1, incr=0)
            assert ks.keys() == o.keys
            sets.append(ks)
            c = sk.KmerContext(0)
            c.load_keyset(ks, 6)
            c.set_counts(0, _type_col(informative))
            ctxs.append(c)
        c, want = ctxs[0], refs[0][0]
        c.scan_stream(stream, 1)
        got = c.counts(1)
        assert np.array_equal(got, want), ("COUNT", np.nonzero(got != want)[0][:10])
        with sk.KmerContext(0) as c0:
            c0.set_option("text_stage", 0)
            c0.load_keyset(sets[0], 4)
            c0.scan_stream(stream, 1)
            got = c0.counts(1)
        assert np.array_equal(got, want), ("COUNT text_stage 0", np.nonzero(got != want)[0][:10])
        if not odd:
            buf = c.dev_alloc(len(packed))
            c.dev_upload(buf, packed)
            c.scan_device_packed(buf, len(stream), 2)
            c.sync()
            c.dev_free(buf)
            got = c.counts(2)
            assert np.array_equal(got, want), ("PACKED", np.nonzero(got != want)[0][:10])
        t, h = c.tally_batch(stream, starts, 0, 2)
        tr.check_single(refs[0][2], stream, starts, refs[0][1], t, h, (name, "TALLY"))
        with sk.KmerUnion(ctxs, 0, 2) as u:
            t, h = u.tally_batch(stream, starts)
            for m in range(2):
                tr.check_single(refs[m][2], stream, starts, refs[m][1], t[:, m, :], h[h[:, 0] == m][:, 1:], (name, "UNION", m))
    finally:
        for c in ctxs:
            c.close()
        for k in sets:
            k.close()
