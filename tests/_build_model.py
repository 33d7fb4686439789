"""Python model of what the table builder on the device leaves behind (sk_table_build_from_text), and the worlds its tests run on.
TEST INFRASTRUCTURE, imported by tests/test_table_build_host.py (the model against the host builder and the oracle, every world's
premise; no GPU) and tests/test_table_build_gpu.py.  The model holds nothing of the library; the helpers at the end ask the
oracle and a context for their keys.

The rule is that of native.KmerContext.build_from_text and dk_record (sk_host.c): records of 30 bases or more form the text, end to
end; a window starts where 31 A/C/G/T bases (either case) of ONE record follow; any other byte stands in the text as code 0.  Rows
are numbered by first occurrence along the text.  A key is what Keyset.packed and skh_keyset_key hold: A 0, C 1, G 2, T 3, the
first base in the highest of 62 bits, the larger of the window and its reverse complement."""
import functools
import random

import numpy as np

import _synth

K = 31
_CODE = np.full(256, 4, dtype=np.uint8)
for _i, _c in enumerate(b"ACGT"):
    _CODE[_c] = _CODE[_c | 0x20] = _i


class Built:
    """nbases, nstarts; keys (uint64), pos (their first text positions, ascending) and fwd (the key is the window as it stands there,
    not its reverse complement) in row order; start[p]: a window starts at p; first[p]: ... and is its key's first"""

    @property
    def nrows(self):
        return len(self.keys)

    @property
    def nblk(self):
        return self.nbases // 64 + 2                                   # the rank map's blocks (sk_table_build_from_text_steps)

    def block_bits(self):
        """the rank map's 64 bits per block as the builder must leave them: [nblk, 64] of bool"""
        b = np.zeros(self.nblk * 64, dtype=bool)
        b[: self.nbases] = self.first
        return b.reshape(self.nblk, 64)


def kept(records):
    return [bytes(r) for r in records if len(r) >= K - 1]


def build(records):
    m = Built()
    seqs = kept(records)
    text = np.frombuffer(b"".join(seqs), dtype=np.uint8)
    n = m.nbases = len(text)
    m.start = np.zeros(n, dtype=bool)
    m.first = np.zeros(n, dtype=bool)
    m.keys, m.pos, m.fwd, m.nstarts = np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.int64), np.zeros(0, dtype=bool), 0
    if n < K:
        return m
    code = _CODE[text]
    bad = np.concatenate([[0], np.cumsum(code > 3)])
    nw = n - K + 1
    ok = bad[K:] - bad[:nw] == 0
    end = 0
    for s in seqs:
        end += len(s)
        ok[max(end - K + 1, 0): min(end, nw)] = False                 # (a window of one record: none runs into the next)
    c = (code & 3).astype(np.uint64)
    fwd = np.zeros(nw, dtype=np.uint64)
    rc = np.zeros(nw, dtype=np.uint64)
    for j in range(K):                                                 # the 2-bit packing, rolled over every window at once
        fwd = (fwd << np.uint64(2)) | c[j: j + nw]
        rc |= (np.uint64(3) - c[j: j + nw]) << np.uint64(2 * j)
    idx = np.nonzero(ok)[0]
    m.nstarts = len(idx)
    m.start[:nw] = ok
    uk, at = np.unique(np.maximum(fwd, rc)[idx], return_index=True)   # (return_index: each key's first place among idx)
    order = np.argsort(at, kind="stable")
    m.keys, m.pos = uk[order], idx[at[order]]
    m.fwd = fwd[m.pos] > rc[m.pos]
    m.first[m.pos] = True
    return m


def key_bytes(keys):
    """the 31 letters of packed keys, as Keyset.keys() spells them"""
    keys = np.asarray(keys, dtype=np.uint64)
    out = np.empty((len(keys), K), dtype=np.uint8)
    lut = np.frombuffer(b"ACGT", dtype=np.uint8)
    for i in range(K):
        out[:, i] = lut[((keys >> np.uint64(2 * (K - 1 - i))) & np.uint64(3)).astype(np.int64)]
    return [bytes(r) for r in out]


def slot_count(nstarts, load_pct):
    """the slots sk_table_build_from_text_steps takes for nstarts windows"""
    lg = 10
    while (1 << lg) * load_pct < nstarts * 100 and lg < 31:
        lg += 1
    return 1 << lg


def most_starts(slots, load_pct):
    """the largest nstarts that still gets `slots` slots: the loop above stops at slots * load_pct >= nstarts * 100"""
    return slots * load_pct // 100


# ---- the worlds: name -> records ----------------------------------------------------------------------------------------------------------
ONE_RECORD = (31, 32, 47, 48, 63, 64, 65, 94, 95, 127, 128, 129)
RANK_NBLK = (1023, 1024, 1025, 2048, 2049, 3000)
TANDEM = (2, 3, 7, 64)
BIG = 1048576 + 4321
SLOT_STEPS = tuple((pct, slots) for pct in (50, 90) for slots in (1024, 2048))


def _dna(rng, n):
    """_synth.rand_dna for long texts: numpy's generator, seeded from rng"""
    return np.frombuffer(b"ACGT", dtype=np.uint8)[np.random.default_rng(rng.getrandbits(32)).integers(0, 4, n)].tobytes()


def _one(L):
    return [_synth.rand_dna(random.Random(7100 + L), L)]


def _thirty_ones():
    """2,000 records of exactly 31 bases, and after every 97th one of 30: no window, but its 30 bases move every later start"""
    rng = random.Random(7200)
    recs = []
    for i in range(2000):
        recs.append(_synth.rand_dna(rng, 31))
        if i % 97 == 96:
            recs.append(_synth.rand_dna(rng, 30))
    return recs


def _n_runs():
    rng = random.Random(7300)
    d = _synth.rand_dna
    return [d(rng, 300) + b"N" + d(rng, 250) + b"N" * 40 + d(rng, 333) + b"n" * 200 + d(rng, 40) + b"N" + d(rng, 30) + b"N" + d(rng, 500).lower()
            + d(rng, 200)]


def _poly_a():
    return [b"A" * 5000]


def _tandem(period):
    rng = random.Random(7400 + period)
    while True:
        unit = _synth.rand_dna(rng, period)
        if len(set(unit)) > 1 and all(unit != unit[i:] + unit[:i] for i in range(1, period)):   # (its period is `period`, no less)
            return (unit * (4096 // period + 2))[: 4096 + period]


def _strands():
    """revcomp(a[500:900]) before a: those keys are first seen on the other strand; a second record repeats pieces of the first, on
    both strands: duplicates, which must not get a rank bit"""
    rng = random.Random(7500)
    a = _synth.rand_dna(rng, 3000)
    return [_synth.revcomp(a[500:900]) + a, a[100:400] + _synth.rand_dna(rng, 200) + _synth.revcomp(a[2000:2300]) + a[2950:] + _synth.rand_dna(rng, 64)]


def _copied(rng, n, share, piece=(40, 400)):
    """n random bases of which about `share` are copies (one in three from the other strand) of places earlier in the text"""
    out = bytearray(_dna(rng, n))
    copied, at = 0, n // 8
    while copied < share * n:
        ln = rng.randrange(*piece)
        at += rng.randrange(ln, int(ln * (1 - share) / share * 2))
        if at + ln > n:
            at = n // 8 + rng.randrange(1000)
            continue
        src = rng.randrange(0, at - ln)
        seg = bytes(out[src:src + ln])
        out[at:at + ln] = _synth.revcomp(seg) if rng.random() < 0.34 else seg
        copied += ln
        at += ln
    return bytes(out)


def _rank(nblk, r):
    """nbases = 64 (nblk - 2) + r; the second half repeats slices of the first, so the blocks' popcounts differ"""
    n = 64 * (nblk - 2) + r
    rng = random.Random(7600 + 2 * nblk + (r > 0))
    half = n // 2
    first = _dna(rng, half)
    out = bytearray(first + _dna(rng, n - half))
    at = half + 17
    while at + 300 < n:
        ln = rng.randrange(31, 200)
        src = rng.randrange(0, half - ln)
        out[at:at + ln] = first[src:src + ln]
        at += ln + rng.randrange(20, 300)
    return [bytes(out)]


def _big():
    return [_copied(random.Random(7700), BIG, 0.05)]


def _no_window():
    """records of 31 bases and more with an N every 20 bases: a text, and not one window"""
    rng = random.Random(7800)
    out = []
    for n in (31, 64, 257, 1000):
        g = bytearray(_synth.rand_dna(rng, n))
        g[19::20] = b"N" * len(g[19::20])
        out.append(bytes(g))
    return out


def distinct_text(nstarts, seed):
    """one record of nstarts windows, all of them different keys"""
    for i in range(20):
        g = _synth.rand_dna(random.Random(seed + i), nstarts + K - 1)
        if build([g]).nrows == nstarts:
            return [g]
    raise AssertionError("no text of distinct keys in 20 draws")


def step_tandem(nstarts):
    """one record of nstarts windows that is one tandem repeat of period 5: many windows, five keys (a period's shifts)"""
    return [(b"ACGTT" * (nstarts // 5 + 8))[: nstarts + K - 1]]


def _steps():
    out = {}
    for pct, slots in SLOT_STEPS:
        top = most_starts(slots, pct)
        for d, tag in ((0, "top"), (1, "over"), (-1, "under")):
            out["step%d_%d_%s" % (pct, slots, tag)] = functools.partial(distinct_text, top + d, 7900 + pct + slots + d)
        out["step%d_%d_tandem" % (pct, slots)] = functools.partial(step_tandem, top)
    return out


WORLDS = {}
for _L in ONE_RECORD:
    WORLDS["one%d" % _L] = functools.partial(_one, _L)
WORLDS.update({"thirty_ones": _thirty_ones, "n_runs": _n_runs, "poly_a": _poly_a})
for _p in TANDEM:
    WORLDS["tandem%d" % _p] = functools.partial(lambda p: [_tandem(p)], _p)
WORLDS["strands"] = _strands
for _b in RANK_NBLK:
    for _r in (0, 63):
        WORLDS["rank%d_r%d" % (_b, _r)] = functools.partial(_rank, _b, _r)
WORLDS["big"] = _big
STEP_WORLDS = _steps()                                                 # (their context takes the table_load_pct of their name)
EMPTY_WORLD = _no_window


@functools.lru_cache(maxsize=None)
def records(name):
    return tuple((WORLDS.get(name) or STEP_WORLDS[name])())


@functools.lru_cache(maxsize=None)
def model(name):
    return build(records(name))


def load_pct(name):
    return int(name[4:6]) if name.startswith("step") else 50


def scan_stream_of(name, rng=None):
    """the reads of a world's scan: the strain's records and their reverse complements, the first and last 80 bases of the text,
    the 80 bases around every record junction -- the big world: those ends, and 200 reads drawn from the text and at random"""
    recs = kept(records(name))
    text = b"".join(recs)
    reads = [text[:80], text[-80:], _synth.revcomp(text[:80]), _synth.revcomp(text[-80:])]
    if name == "big":
        rng = random.Random(7777)
        for i in range(200):
            ln = rng.choice([31, 47, 100, 150, 250])
            a = rng.randrange(len(text) - ln)
            r = text[a:a + ln] if i % 4 else _synth.rand_dna(rng, ln)
            reads.append(_synth.revcomp(r) if i % 2 else r)
    else:
        reads += list(recs) + [_synth.revcomp(r) for r in recs]
        at = 0
        for r in recs[:-1]:
            at += len(r)
            reads.append(text[max(at - 40, 0):at + 40])
    return b"\n".join(reads) + b"\n"


# ---- the oracle's view of a world, and a context's key list ---------------------------------------------------------------------------------
def oracle_rows(strain_records, scan=None):
    """(packed keys of the oracle's table of these records in ITS row order, its count of the stream `scan` for each): numpy all
    the way, so 1.1 Mbase costs a second"""
    import _oracle
    small = sum(map(len, strain_records)) < 100000
    t = _oracle.OracleTable(capacity=16384) if small else _oracle.OracleTable()
    assert t.build_stream(b"\n".join(strain_records) + b"\n", default=1, incr=0, short_policy=1) == 0
    if scan is not None:
        t.scan_stream(scan, 1)
    n = t.size
    letters = np.zeros((max(n, 1), 32), dtype=np.uint8)
    counts = np.zeros((max(n, 1), t.ncols), dtype=np.uint32)
    _oracle.L.kso_table_rows(t.h, K, letters.ctypes.data, counts.ctypes.data)
    t.close()
    code = _CODE[letters[:n, :K]].astype(np.uint64)
    assert (code < 4).all()
    packed = np.zeros(n, dtype=np.uint64)
    for i in range(K):
        packed = (packed << np.uint64(2)) | code[:, i]
    return packed, counts[:n, 1].astype(np.int64)


def rows_of(keys, among):
    """the index in `among` (distinct packed keys) of every key of `keys`: all of them must be there"""
    order = np.argsort(among, kind="stable")
    at = np.minimum(np.searchsorted(among[order], keys), max(len(among) - 1, 0))
    rows = order[at] if len(among) else np.zeros(0, dtype=np.int64)
    assert len(keys) == 0 or (len(among) and np.array_equal(among[rows], keys)), "a key the other table does not hold"
    return rows


def exported_keys(c, rows=None):
    """sk_table_export_keys of a context whose table was built on the device; rows: sk_table_export_keys_of for those"""
    from strainer2_amd.native import lib
    import ctypes as C
    if rows is None:
        out = np.zeros(max(c.nrows, 1), dtype=np.uint64)
        lib.sk_table_export_keys.argtypes = [C.c_void_p, C.c_void_p]
        assert lib.sk_table_export_keys(c._h, out.ctypes.data) == 0
        return out[: c.nrows]
    rows = np.ascontiguousarray(rows, dtype=np.uint32)
    out = np.zeros(max(len(rows), 1), dtype=np.uint64)
    lib.sk_table_export_keys_of.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
    assert lib.sk_table_export_keys_of(c._h, rows.ctypes.data, len(rows), out.ctypes.data) == 0
    return out[: len(rows)]
