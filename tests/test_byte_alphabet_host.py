"""The byte alphabet, the half that needs no GPU: the worlds of tests/test_byte_alphabet_gpu.py (tests/_synth.py: alphabet_world_a,
_b, _c) are what they claim to be and have power -- asserted on the oracle's side, so that a degenerate world cannot pass in
silence --, the host's key-set builder gives the oracle's keys in the oracle's row order for a strain that holds every byte value
(the signed djb2 replay, the complement of bytes at or above 0x80), and the host pre-pack (sk_pack_stream) makes of World A's
stream what its contract says.

NUL: DESIGN.md section 2 defines it as a hard breaker, the oracle's upcase and has_enn stop there as a C string does (it would
leave lower case behind a NUL as it is).  The oracle is therefore fed the stream with every NUL turned into N (_for_oracle): the
offsets stay, and a window that holds N is never counted -- the documented rule, nothing else."""
import os
import subprocess
import sys

import numpy as np
import pytest

import _oracle
import _synth
import strainer2_amd as sk

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = 4096                      # slots of an oracle table that is only asked for sums (the row order is nobody's business there)


def _for_oracle(data: bytes) -> bytes:
    """NUL is a hard breaker; the oracle ends a C string there.  N in its place: same offsets, and a
    window with N is never counted, which is the rule."""
    return data.replace(b"\0", b"N")


def _stream(recs) -> bytes:
    return b"\n".join(recs) + b"\n"


def _offsets(recs):
    return np.cumsum([0] + [len(r) + 1 for r in recs[:-1]])


class _Alone:
    """what a read adds to the oracle's counters when it is scanned on its own"""

    def __init__(self, sstream, capacity=SMALL):
        self.t = _oracle.OracleTable(capacity=capacity, ncols=2)
        assert self.t.build_stream(sstream, short_policy=1) == 0
        self.keys = self.t.rows()[0]
        self.now = np.zeros(len(self.keys), dtype=np.int64)

    def rows(self, read: bytes):
        """the per-row differences"""
        self.t.scan_stream(_for_oracle(read) + b"\n", 1)
        now = self.t.counts()[:, 1].astype(np.int64)
        d, self.now = now - self.now, now
        return d

    def hits(self, read: bytes) -> int:
        return int(self.rows(read).sum())


def test_world_a_holds_every_byte_at_every_phase_and_has_power():
    strain, recs, cases = _synth.alphabet_world_a()
    stream, off = _stream(recs), _offsets(recs)
    assert 380_000 < len(stream) < 500_000
    seen = set()
    for b, j, i, was in cases:
        at = int(off[i]) + _synth.ALPHABET_AT
        assert stream[at] == b and at % 16 == j and len(recs[i]) == _synth.ALPHABET_READ and was in b"ACGT"
        seen.add((b, j))
    assert seen == {(b, j) for b in range(256) for j in range(16)}             # all 4096 (byte, phase) pairs
    assert all(len(r) < 31 and not set(r) - set(b"ACGT") for k, r in enumerate(recs) if k % 2 == 0)    # the fillers: no window, no foreign byte
    # power, by the oracle: the strain's windows are all keys, a hard breaker costs exactly the 31 windows that hold it, the base
    # that was there (either case) costs none, and some U in place of a T is found through the reverse strand
    o = _Alone(strain + b"\n")
    assert len(o.keys) == len(strain) - 30                                     # (600 random bases: no k-mer twice)
    t = _oracle.OracleTable(capacity=SMALL)
    assert t.build_stream(strain + b"\n") == 0
    t.scan_stream(_for_oracle(stream), 1)
    assert int(t.counts()[:, 1].sum()) > 32 * len(cases)
    u_hits, own = [], []
    for b, j, i, was in cases:
        if j == 5 and b in b"Nn\n\0":
            assert o.hits(recs[i]) == 32, b
        if j == 4 and b & 0x5F == was:                                        # (even phases: the byte stands where "its" base stood)
            assert o.hits(recs[i]) == (63 if b in b"ACGTacgt" else 32), b
            own.append(b)
        if b in b"Uu":
            assert was == ord("T")
            u_hits.append(o.hits(recs[i]))
    assert bytes(own) == bytes([0x41, 0x43, 0x47, 0x54, 0x61, 0x63, 0x67, 0x74, 0xC1, 0xC3, 0xC7, 0xD4, 0xE1, 0xE3, 0xE7, 0xF4])
    assert len(u_hits) == 32 and min(u_hits) >= 32 and max(u_hits) > 32, u_hits
    # (the thinned world of the TALLY tests)
    _, recs4, cases4 = _synth.alphabet_world_a(phases=(0, 3, 12, 15), leave_out=b"\n")
    off4 = _offsets(recs4)
    assert {(b, int(off4[i] + _synth.ALPHABET_AT) % 16) for b, j, i, _w in cases4} == {(b, j) for b in range(256) if b != 10 for j in (0, 3, 12, 15)}
    assert b"\n" not in b"".join(recs4)


def test_world_b_holds_every_pair_on_every_byte_of_a_word():
    strain, recs, cases = _synth.alphabet_world_b()
    stream, off = _stream(recs), _offsets(recs)
    pairs = _synth.ALPHABET_PAIR_SET
    assert len(pairs) == len(set(pairs)) == 30 and len(cases) == 30 * 30 * 4 and len(stream) < 500_000
    seen, mods = set(), set()
    for k, (b1, b2, m) in enumerate(cases):
        at = int(off[2 * k + 1]) + _synth.ALPHABET_AT
        assert stream[at] == b1 and stream[at + 1] == b2 and at % 16 == m
        seen.add((b1, b2, at % 4))
        mods.add(m)
    assert seen == {(b1, b2, w) for b1 in pairs for b2 in pairs for w in range(4)}
    assert mods == set(range(16))                                              # (so the pair also straddles two chunks)
    t = _oracle.OracleTable(capacity=SMALL)
    assert t.build_stream(strain + b"\n") == 0
    t.scan_stream(_for_oracle(stream), 1)
    assert int(t.counts()[:, 1].sum()) > 31 * len(cases)                       # 16 windows in front of the pair, 15 behind it


def test_world_c_keys_are_the_oracles_in_the_oracles_order():
    """a strain with every byte value but NUL and the separator: byte-string keys through the complement map (K -> '.', bytes at
    or above 0x80 -> -1), oriented by signed compare, placed by the signed djb2 -- Keyset.from_stream against the oracle's table"""
    records = _synth.alphabet_world_c()
    assert [b for b, _ in records] == [b for b in range(1, 256) if b != 10]
    assert all(len(r) == 91 and r[45] == b and not set(r[:45] + r[46:]) - set(b"ACGT") for b, r in records)
    sstream = _stream([r for _, r in records])
    ks = sk.Keyset.from_stream(sstream)
    t = _oracle.OracleTable()
    assert t.build_stream(sstream, short_policy=1) == 0
    okeys, ocounts = t.rows()
    assert ks.keys() == okeys
    assert np.array_equal(ks.first_count(), ocounts[:, 0])
    wide = np.array([bool(set(k) - set(b"ACGT")) for k in okeys])              # rows only the byte-string kernel can reach
    assert ks.nwide == int(wide.sum()) and 7000 < ks.nwide < 8000
    # power: the record's own read (c == b) hits through the windows that hold b -- except for the b no key holds, which the
    # oracle reports as N and n; a, c, g, t, A, C, G, T make plain keys, every other byte at least one wide one
    o = _Alone(sstream, capacity=100_000)
    owide = np.array([bool(set(k) - set(b"ACGT")) for k in o.keys])
    keyless, plain, partly = [], [], []
    for b, r in records:
        d = o.rows(r)
        assert int(d.sum()) in (30, 61), b
        if int(d.sum()) == 30:                                                 # the 15 + 15 windows beside b and nothing else
            keyless.append(b)
        elif not d[owide].any():
            plain.append(b)
        elif int(d[owide].sum()) < 31:                                         # some windows' keys are wide, some plain
            partly.append(b)
    assert bytes(keyless) == b"Nn"
    assert bytes(plain) == b"ACGTacgt"
    assert bytes(partly) == b"Uu"                                              # (U complements to A: where the other strand wins, the key is plain)
    ks.close()


def _contract(stream: bytes):
    """sk_pack_stream's contract, stated once more: per 16-byte chunk a code word -- two bits a byte, first byte highest, A 0 C 1
    G 2 T 3 in either case, 0 for any other byte -- and a mask with bit i set iff byte i is none of ACGTacgt (or lies beyond the end)"""
    code = np.full(256, 4, dtype=np.uint32)
    for ch, v in zip(b"ACGTacgt", (0, 1, 2, 3, 0, 1, 2, 3)):
        code[ch] = v
    n = len(stream)
    c = np.full((n + 15) // 16 * 16, 4, dtype=np.uint32)
    c[:n] = code[np.frombuffer(stream, dtype=np.uint8)]
    c = c.reshape(-1, 16)
    words = ((c & 3) << (2 * (15 - np.arange(16, dtype=np.uint32)))).sum(axis=1, dtype=np.uint32)
    masks = ((c == 4).astype(np.uint32) << np.arange(16, dtype=np.uint32)).sum(axis=1, dtype=np.uint32)
    return words, masks.astype(np.uint16)


@pytest.mark.parametrize("simd", ["1", "0"])
def test_host_pre_pack_of_world_a(simd, tmp_path):
    """the one place where the host's and the device's decision about a byte could drift apart: sk_pack_stream over World A's
    stream (every byte value at every chunk phase), the vector path and the table path (chosen once per process: a child each)"""
    _, recs, _ = _synth.alphabet_world_a()
    stream = _stream(recs)
    out = str(tmp_path / "packed.bin")
    code = ("import sys; sys.path[:0] = [%r, %r]; import _synth, strainer2_amd as sk\n"
            "s = b'\\n'.join(_synth.alphabet_world_a()[1]) + b'\\n'\n"
            "p, odd = sk.pack_stream(s); assert odd; p.tofile(%r)\n" % (REPO, os.path.join(REPO, "tests"), out))
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=dict(os.environ, SK_PACK_SIMD=simd))
    assert p.returncode == 0, p.stderr[-800:]
    packed = np.fromfile(out, dtype=np.uint8)
    nch = (len(stream) + 15) // 16
    assert len(packed) == 6 * nch
    words, masks = _contract(stream)
    assert np.array_equal(np.frombuffer(packed[:4 * nch].tobytes(), dtype="<u4"), words)
    assert np.array_equal(np.frombuffer(packed[4 * nch:].tobytes(), dtype="<u2"), masks)
    # and `odd` byte by byte: a chunk of pure bases around one byte is odd iff that byte is none of ACGTacgtNn and the separator
    for b in range(256):
        _, odd = sk.pack_stream(b"ACGTACG" + bytes([b]) + b"ACGTACGTACGT")
        assert odd == (b not in b"ACGTacgtNn\n"), b
