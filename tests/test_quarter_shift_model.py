"""The scan's quarter-shifted level-1 question (sk_scan_grid), as a model in Python: what the rule covers,
what a foreign byte among the borrowed bases does to it, and -- against the oracle -- that a chunk it prunes has no counted window.

A chunk is 16 bases on the 16-base grid.  The 16 windows (31 bases) that hold chunk c whole are numbered j = 0..15: window j has j
bases left of the chunk and 15 - j right of it.  A clean chunk that passed level 1 asks about the 16-mers at shift -8 (`al`: stands
for the windows j >= 8) and +8 (`ar`: j <= 7); a side that passed then asks about the 16-mer at shift -4 or +4; a side that is left
goes on to level 2.  Level 1 holds every 16-mer of the strain, so the model's level 1 is the exact set: any real filter prunes less.
No GPU is needed here."""
import random

import numpy as np
import pytest

import _oracle
import _synth

K = 31
ACGT = frozenset(b"ACGT")


def _holders(lo, hi):
    """the windows j of the chunk at [0, 16) that hold the bases [lo, hi) whole"""
    return {j for j in range(16) if -j <= lo and hi <= -j + K}


def _mask(chunk):
    """the kernel's mask of a chunk: bit i <=> byte i is no A/C/G/T"""
    return sum(1 << i for i, b in enumerate(chunk) if b not in ACGT)


def _verdict(prev, cw, nxt, has16):
    """(al, ar, al8, ar8) of the clean chunk cw between its neighbours: the sides left after the quarter-shifted questions, and after
    the half-shifted ones alone.  The validity of borrowed bases is read off the neighbours' masks, as the kernel does."""
    ivp, ivn = _mask(prev), _mask(nxt)
    al8 = (ivp >> 8) == 0 and has16(prev[8:] + cw[:8])
    ar8 = (ivn & 0xFF) == 0 and has16(cw[8:] + nxt[:8])
    al = al8 and (ivp >> 12) == 0 and has16(prev[12:] + cw[:12])
    ar = ar8 and (ivn & 0xF) == 0 and has16(cw[4:] + nxt[:4])
    return al, ar, al8, ar8


def _live(prev, nxt):
    """the live windows j of a clean chunk, by the definition: all 31 bases are A/C/G/T"""
    ctx = prev + b"A" * 16 + nxt
    return {j for j in range(16) if not set(ctx[16 - j:16 - j + K]) - ACGT}


def _live_kernel(prev, nxt):
    """the same from the masks, by the kernel's run-of-31 bit trick (its bit k is the window ENDING at chunk start + 15 + k: j = 15 - k)"""
    v = ~(_mask(prev) | (_mask(nxt) << 32)) & 0x0000FFFFFFFFFFFF
    rr = v & (v << 1)
    rr &= rr << 2
    rr &= rr << 4
    rr &= rr << 8
    rr &= rr << 15
    live = (rr >> 31) & 0xFFFF
    return {15 - k for k in range(16) if (live >> k) & 1}


def test_coverage_of_the_shifted_16_mers():
    for j in range(16):
        assert (j in _holders(-4, 12)) == (j >= 4)
        assert (j in _holders(4, 20)) == (j <= 11)
        assert (j in _holders(-8, 8)) == (j >= 8)
        assert (j in _holders(8, 24)) == (j <= 7)
    # every window `al` stands for holds the 16-mer at -4 as well, every one `ar` stands for the one at +4; the two sides are all 16
    assert _holders(-8, 8) <= _holders(-4, 12) and _holders(8, 24) <= _holders(4, 20)
    assert _holders(-8, 8) | _holders(8, 24) == set(range(16)) and not _holders(-8, 8) & _holders(8, 24)


@pytest.mark.parametrize("byte", [b"N", b"\n", b"U"])
@pytest.mark.parametrize("p", range(4))
@pytest.mark.parametrize("side", ["left", "right"])
def test_a_foreign_byte_among_the_borrowed_bases(side, p, byte):
    """position p of the 4 bases borrowed from a neighbour is no A/C/G/T: that side's question is "absent" whatever the filter says
    (a saturated one here), the windows this removes all hold the byte, no window that holds it is live, and the other side's
    verdict does not move"""
    clean = b"ACGTTGCAAGCTTCGA"
    if side == "left":
        prev, nxt, at = clean[:12 + p] + byte + clean[13 + p:], clean, -4 + p
    else:
        prev, nxt, at = clean, clean[:p] + byte + clean[p + 1:], 16 + p
    al, ar, al8, ar8 = _verdict(prev, clean, nxt, lambda s: True)
    assert (al, ar) == ((False, True) if side == "left" else (True, False))
    removed = _holders(-8, 8) if side == "left" else _holders(8, 24)
    holding = _holders(at, at + 1)
    assert removed <= holding
    assert holding == ({j for j in range(16) if j >= 4 - p} if side == "left" else {j for j in range(16) if j <= 14 - p})
    assert not holding & _live(prev, nxt)
    assert _live_kernel(prev, nxt) == _live(prev, nxt) == set(range(16)) - holding


def test_live_windows_from_the_masks_are_the_definition():
    rng = random.Random(4701)
    for _ in range(2000):
        prev, nxt = (bytes(rng.choice(b"ACGT" if rng.random() < 0.93 else b"N\nU") for _ in range(16)) for _ in range(2))
        assert _live_kernel(prev, nxt) == _live(prev, nxt)


def _world(seed):
    """(strain, stream): a few-kbp strain in which some 8-mers occur twice, and reads of it -- exact, with substitutions, chimeras of
    the two places of a repeated 8-mer, with N -- between random ones"""
    rng = random.Random(seed)
    strain = bytearray(_synth.rand_dna(rng, 4000))
    twice = []
    for i in range(12):                                               # the 8-mer at a is planted at b as well
        a, b = 100 + 300 * i, 150 + 300 * i + 40
        strain[b:b + 8] = strain[a:a + 8]
        twice.append((a, b))
    strain = bytes(strain)
    recs, off = [], 0
    for _ in range(260):
        x = rng.random()
        ln = rng.randrange(31, 151)
        a = rng.randrange(len(strain) - ln)
        rev = rng.random() < 0.5
        if x < 0.25:
            r = strain[a:a + ln]
        elif x < 0.55:
            r = _synth.mutate(rng, strain[a:a + ln], rng.choice([0.01, 0.03, 0.08]))
        elif x < 0.75:                                                # X P Y: up to P from one place, from P on from the other
            a, b = rng.choice(twice)
            if rng.random() < 0.5:
                a, b = b, a
            pre, post = rng.randrange(8, 40), rng.randrange(8, 40)
            r = strain[a - pre:a + 8] + strain[b + 8:b + 8 + post]
            # a filler record (too short for a window) puts P at the start of a chunk (X P is its -8 question) or 8 bases into one
            # (P Y is its +8 question)
            at = post if rev else pre
            fill = (rng.choice([0, 8]) - (off + at) - 1) % 16
            recs.append(_synth.rand_dna(rng, fill))
            off += fill + 1
        elif x < 0.85:
            r = bytearray(strain[a:a + ln])
            r[rng.randrange(ln)] = ord("N")
            r = bytes(r)
        else:
            r = _synth.rand_dna(rng, ln)
        recs.append(_synth.revcomp(r) if rev else r)
        off += len(r) + 1
    return strain, b"\n".join(recs) + b"\n"


@pytest.mark.parametrize("seed", range(6))
def test_a_pruned_chunk_has_no_counted_window(seed):
    strain, stream = _world(seed)
    s16 = {strain[i:i + 16] for i in range(len(strain) - 15)}
    s16 |= {_synth.revcomp(w) for w in s16}
    has16 = s16.__contains__
    # the counted windows, here and by the oracle
    t = _oracle.OracleTable(capacity=16384)
    assert t.build_stream(strain + b"\n") == 0
    t.scan_stream(stream, 1)
    keys, counts = t.rows()
    t.close()
    row = {}
    for i, k in enumerate(keys):
        row[k] = row[_synth.revcomp(k)] = i
    mine = np.zeros(len(keys), dtype=np.int64)
    counted = set()                                                   # stream offsets at which a counted window starts
    for p in range(len(stream) - K + 1):
        r = row.get(stream[p:p + K])
        if r is not None:
            mine[r] += 1
            counted.add(p)
    assert np.array_equal(mine, counts[:, 1]), "the model's counted windows are not the oracle's"
    assert len(counted) > 2000
    pad = b"\n" * 16
    padded = pad + stream + b"\n" * (-len(stream) % 16) + pad
    pruned_by_quarter = with_windows = 0
    for c in range((len(stream) + 15) // 16):
        prev, cw, nxt = (padded[16 * (c + d):16 * (c + d) + 16] for d in range(3))
        if set(cw) - ACGT:
            continue
        al, ar, al8, ar8 = _verdict(prev, cw, nxt, has16)
        left = {j for j in range(8, 16) if 16 * c - j in counted}
        right = {j for j in range(0, 8) if 16 * c - j in counted}
        with_windows += bool(left | right)
        if left:
            assert has16(cw) and al, (seed, c, sorted(left))
        if right:
            assert has16(cw) and ar, (seed, c, sorted(right))
        pruned_by_quarter += has16(cw) and (al8 or ar8) and not (al or ar)
    # power: about 50 chimeras a world; one is pruned by the quarter-shifted question alone when the far side of P is too short to pass
    # on its own (under 24 of its 8..39 bases: about half of them)
    assert with_windows > 150 and pruned_by_quarter >= 5, (with_windows, pruned_by_quarter)
