"""Crafted worlds for the hash-addressed structures (tests/test_hash_worlds_host.py, tests/test_hash_worlds_gpu.py).  TEST
INFRASTRUCTURE, imported by the tests only.

tests/native/hash_craft.c searches, with the library's own hash functions, for keys whose first slot is chosen: clusters at the
END of a table, so that linear probing runs over the last slot into slot 0, and walks that are longer than two waves.  The
worlds below put such keys into strains (one 31-base record a key) and into reads, together with absent keys that reach the
table for certain (U windows, _synth.u_window_of).  Model says what the walks in such a table look like; the host test asserts
on it that every world is what it claims to be, the GPU test compares every form of the scan with the oracle on it."""
import atexit
import ctypes as C
import functools
import os
import random
import shutil
import subprocess
import tempfile

import numpy as np

import _synth

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "native", "hash_craft.c")
K = 31
CAP = 4096                              # first size of the host builder's and the oracle's table in the small worlds (the row order follows it)
MAX_TRIES = 1 << 34


@functools.lru_cache(maxsize=None)
def lib():
    d = tempfile.mkdtemp(prefix="hash_craft_")
    atexit.register(shutil.rmtree, d, True)
    so = os.path.join(d, "hash_craft.so")
    subprocess.run(["gcc", "-O2", "-Wall", "-Wextra", "-shared", "-fPIC", SRC, "-o", so], check=True)
    L = C.CDLL(so)
    u64, u32, vp = C.c_uint64, C.c_uint32, C.c_void_p
    L.hc_craft_keys.restype = u64
    L.hc_craft_keys.argtypes = [u64, u32, u32, u32, C.c_int, vp, u32, u64]
    L.hc_slot0.restype = None
    L.hc_slot0.argtypes = [vp, u32, u32, vp]
    L.hc_u_info.restype = None
    L.hc_u_info.argtypes = [vp, u32, vp, vp]
    L.hc_wide_slot0.restype = None
    L.hc_wide_slot0.argtypes = [C.c_char_p, u32, u32, vp]
    L.hc_craft_wide.restype = u64
    L.hc_craft_wide.argtypes = [u64, u32, u32, u32, C.c_char_p, vp, u32, u64]
    L.hc_craft_bin16.restype = u64
    L.hc_craft_bin16.argtypes = [u64, u32, C.POINTER(u32), C.POINTER(u32), u64]
    L.hc_bin16_of.restype = None
    L.hc_bin16_of.argtypes = [u32, C.POINTER(u32), C.POINTER(u32)]
    L.hc_model_insert.restype = None
    L.hc_model_insert.argtypes = [vp, u32, u32, vp, vp]
    L.hc_model_walk.restype = None
    L.hc_model_walk.argtypes = [vp, u32, vp, vp, u32, vp, vp]
    return L


# ---- packed keys <-> bytes ------------------------------------------------------------------------------------------------
def kmer_bytes(k) -> bytes:
    k = int(k)
    return bytes(b"ACGT"[(k >> (2 * (K - 1 - i))) & 3] for i in range(K))


def pack(w: bytes) -> int:
    k = 0
    for b in w:
        k = (k << 2) | b"ACGT".index(b)
    return k


# ---- the searches -----------------------------------------------------------------------------------------------------------
def craft_keys(seed, lg, lo, hi, n, need_u=False):
    """n distinct canonical packed 31-mers whose first slot in a table of 1 << lg slots lies in [lo, hi]; need_u: each can be
    looked up through a U window (_synth.u_window_of)"""
    out = np.zeros(n, dtype=np.uint64)
    tries = lib().hc_craft_keys(seed, lg, lo, hi, int(need_u), out.ctypes.data, n, MAX_TRIES)
    assert tries, "the key search gave up"
    return out


def slot0(keys, lg):
    keys = np.ascontiguousarray(keys, dtype=np.uint64)
    out = np.zeros(len(keys), dtype=np.uint32)
    lib().hc_slot0(keys.ctypes.data, len(keys), lg, out.ctypes.data)
    return out


def u_info(keys):
    """(reachable through a U window?, bit i = a U may stand at base i of the reverse complement) of canonical packed keys"""
    keys = np.ascontiguousarray(keys, dtype=np.uint64)
    ok = np.zeros(len(keys), dtype=np.uint8)
    tm = np.zeros(len(keys), dtype=np.uint32)
    lib().hc_u_info(keys.ctypes.data, len(keys), ok.ctypes.data, tm.ctypes.data)
    return ok.astype(bool), tm


WIDE_LETTERS = b"RYSWBDHV"               # IUPAC codes whose complement is an IUPAC code again (not K: the reference maps it to '.')
WIDE_COMP = bytes.maketrans(b"ACGTRYSWBDHVacgtryswbdhv", b"TGCAYRSWVHDBtgcayrswvhdb")


def craft_wide(seed, wmask, lo, hi, n):
    """n distinct byte-string keys (31 bytes, A/C/G/T and one to three letters of WIDE_LETTERS, in the orientation the library
    stores) whose first slot in an index of wmask + 1 slots lies in [lo, hi]"""
    buf = C.create_string_buffer(32 * n)
    tries = lib().hc_craft_wide(seed, wmask, lo, hi, WIDE_LETTERS, buf, n, MAX_TRIES)
    assert tries, "the byte-string key search gave up"
    return [buf.raw[32 * i:32 * i + K] for i in range(n)]


def wide_slot0(keys, wmask):
    buf = b"".join(k + b"\0" for k in keys)
    out = np.zeros(len(keys), dtype=np.uint32)
    lib().hc_wide_slot0(buf, len(keys), wmask, out.ctypes.data)
    return out


def craft_bin16(seed, want_key):
    """(a 16-mer whose key in the partitioned pipeline's bins is want_key, its partition)"""
    f, p = C.c_uint32(0), C.c_uint32(0)
    tries = lib().hc_craft_bin16(seed, want_key, C.byref(f), C.byref(p), MAX_TRIES)
    assert tries, "the 16-mer search gave up"
    return bytes(b"ACGT"[(f.value >> (2 * (15 - i))) & 3] for i in range(16)), p.value


def bin16_of(w16: bytes):
    """(bin key, partition) of a 16-mer as sk_bin computes them"""
    key, p = C.c_uint32(0), C.c_uint32(0)
    assert len(w16) == 16
    lib().hc_bin16_of(pack(w16), C.byref(key), C.byref(p))
    return key.value, p.value


# ---- the model ----------------------------------------------------------------------------------------------------------------
class Model:
    """A table of nslots slots filled by linear probing: key i starts at first[i]; inserted in the order given (the set of
    occupied slots, and the number of keys that came to rest below their first slot, do not depend on it)."""

    def __init__(self, first, nslots):
        self.first = np.ascontiguousarray(first, dtype=np.uint32)
        self.nslots = nslots
        assert len(self.first) < nslots and (self.first < nslots).all()
        self.table = np.zeros(nslots, dtype=np.uint32)
        self.final = np.zeros(len(self.first), dtype=np.uint32)
        lib().hc_model_insert(self.first.ctypes.data, len(self.first), nslots, self.table.ctypes.data, self.final.ctypes.data)
        self.wrapped = self.final < self.first                       # present keys that ended below their first slot

    def walk(self, q_first, q_id=None):
        """(slots looked at, walked from the last slot to slot 0?) per query; q_id: the key the query is (None: absent ones)"""
        q_first = np.ascontiguousarray(q_first, dtype=np.uint32)
        ids = np.full(len(q_first), -1, dtype=np.int64) if q_id is None else np.ascontiguousarray(q_id, dtype=np.int64)
        ln = np.zeros(len(q_first), dtype=np.uint32)
        wr = np.zeros(len(q_first), dtype=np.uint8)
        lib().hc_model_walk(self.table.ctypes.data, self.nslots, q_first.ctypes.data, ids.ctypes.data, len(q_first), ln.ctypes.data, wr.ctypes.data)
        return ln, wr.astype(bool)

    def present_walks(self):
        return self.walk(self.first, np.arange(len(self.first)))


def slots_log2(nrows, load_pct):
    """the table's size as the library picks it: the smallest power of two from 1024 on that nrows fill to load_pct at most"""
    lg = 10
    while (1 << lg) * load_pct < nrows * 100 and lg < 31:
        lg += 1
    return lg


# ---- table worlds ----------------------------------------------------------------------------------------------------------------
class World:
    pass


def _flank(rng, u):
    return _synth.rand_dna(rng, rng.randrange(0, 40)) + u + _synth.rand_dna(rng, rng.randrange(0, 40))


def crafted_reads(rng, key_recs, joinable, long_recs, absent, nrandom=300, nlong=150):
    """(records, the same without those that hold a U): every key record in both orientations; every absent key as a U window;
    present keys as U windows; pairs of records that are neighbours in the strain joined into one read (`joinable`: indices i
    whose record i + 1 follows it in the strain); pieces of the ordinary records, either strand, some mutated; random reads,
    short and empty ones, lower case"""
    tagged = []
    for w in key_recs:
        tagged += [(False, w), (False, _synth.revcomp(w))]
    for k in absent:
        u = _synth.u_window_of(rng, kmer_bytes(k))
        assert u, "an absent key without a U window"
        tagged.append((True, u if rng.random() < 0.5 else _flank(rng, u)))
    npu = 0
    for w in key_recs:
        u = _synth.u_window_of(rng, w)
        if u:
            npu += 1
            tagged.append((True, u if rng.random() < 0.5 else _flank(rng, u)))
    assert npu >= 32, "too few present keys with a U window"
    for i in joinable:
        j = key_recs[i] + key_recs[i + 1]
        tagged.append((False, j if rng.random() < 0.5 else _synth.revcomp(j)))
    for _ in range(nlong):
        g = long_recs[rng.randrange(len(long_recs))]
        ln = min(len(g), rng.choice([31, 32, 47, 64, 100, 150]))
        a = rng.randrange(len(g) - ln + 1)
        s = _synth.mutate(rng, g[a:a + ln], rng.choice([0.0, 0.0, 0.02]))
        tagged.append((False, _synth.revcomp(s) if rng.random() < 0.5 else s))
    for _ in range(nrandom):
        tagged.append((False, _synth.rand_dna(rng, rng.choice([0, 5, 30, 31, 32, 64, 150]))))
    rng.shuffle(tagged)
    tagged = [(odd, r.lower() if rng.random() < 0.05 else r) for odd, r in tagged]
    return [r for _, r in tagged], [r for odd, r in tagged if not odd]


def _table_world(name, seed, load_pct, lg, width, ncraft, nabsent, fill, nlong=150):
    """one strain whose table has 1 << lg slots at load_pct: ncraft keys (every other one with a U window) whose first slot is
    among the last `width`, one 31-base record each, and ordinary random records of the lengths in `fill` (len - 30 keys each);
    nabsent keys of the same slots that the strain does not hold"""
    w = World()
    w.name, w.seed, w.load_pct, w.lg, w.width = name, seed, load_pct, lg, width
    n = 1 << lg
    w.crafted = np.concatenate([craft_keys(seed, lg, n - width, n - 1, ncraft - ncraft // 2),
                                craft_keys(seed + 1, lg, n - width, n - 1, ncraft // 2, need_u=True)])
    w.absent = craft_keys(seed + 2, lg, n - width, n - 1, nabsent, need_u=True)
    assert len(set(w.crafted.tolist()) | set(w.absent.tolist())) == ncraft + nabsent
    rng = random.Random(seed)
    key_recs = [kmer_bytes(k) for k in w.crafted]
    rng.shuffle(key_recs)
    w.long_recs = [_synth.rand_dna(rng, ln) for ln in fill]
    half = (len(key_recs) // 4) * 2                                   # (even: the joined pairs below stay neighbours)
    w.key_recs = key_recs
    w.strain_recs = key_recs[:half] + w.long_recs + key_recs[half:]
    w.nkeys = ncraft + sum(ln - 30 for ln in fill)
    w.sstream = b"\n".join(w.strain_recs) + b"\n"
    joinable = [i for i in range(0, min(len(key_recs) - 1, 200), 2)]
    w.recs, w.recs_clean = crafted_reads(rng, key_recs, joinable, w.long_recs, w.absent, nlong=nlong)
    w.stream = b"\n".join(w.recs) + b"\n"
    w.stream_clean = b"\n".join(w.recs_clean) + b"\n"
    assert set(w.stream_clean) <= set(b"ACGTacgt\n") and b"U" in w.stream.upper()
    return w


@functools.lru_cache(maxsize=None)
def wrap50():
    """1024 slots at the default load: 300 of 500 keys start in the last 24 slots"""
    return _table_world("wrap50", 5001, 50, 10, 24, 300, 48, [131, 129])


@functools.lru_cache(maxsize=None)
def full90():
    """table_load_pct = 90: 921 keys in 1024 slots, 300 of them starting in the last 24"""
    return _table_world("full90", 5011, 90, 10, 24, 300, 48, [231, 231, 131, 131] + [31] * 17)


SPARSE5_CRAFTED = 200


@functools.lru_cache(maxsize=None)
def sparse5():
    """table_load_pct = 5 and just over 838,861 keys: 2^25 slots, the first slot takes the hash's low byte on top
    (sk_slot0's kh << 24 half); SPARSE5_CRAFTED keys start in the last 32 slots"""
    return _table_world("sparse5", 5021, 5, 25, 32, SPARSE5_CRAFTED, 48, [838_700 + 30], nlong=600)


# ---- the byte-string index ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def wide_wrap():
    """a strain with 12 byte-string keys (a 32-slot index) that all start in its last 4 slots; reads with the keys in both
    orientations and either case, near misses (one IUPAC letter changed) and absent keys of the same slots"""
    w = World()
    w.name, w.wmask, w.lo = "wide_wrap", 31, 28
    both = craft_wide(5031, w.wmask, w.lo, w.wmask, 15)
    w.keys, w.absent = both[:12], both[12:]
    rng = random.Random(5031)
    w.long_recs = [_synth.rand_dna(rng, 400), _synth.rand_dna(rng, 200)]
    w.strain_recs = [w.long_recs[0]] + w.keys[:6] + [w.long_recs[1]] + w.keys[6:]
    w.sstream = b"\n".join(w.strain_recs) + b"\n"
    recs = []
    for k in w.keys:
        rc = k.translate(WIDE_COMP)[::-1]
        recs += [k, rc, k.lower(), _flank(rng, k), _flank(rng, rc)]
        at = [i for i in range(K) if k[i] in WIDE_LETTERS]
        for _ in range(2):                                            # near misses: one IUPAC letter becomes another
            i = rng.choice(at)
            m = bytearray(k)
            m[i] = rng.choice([x for x in WIDE_LETTERS if x != k[i]])
            recs.append(bytes(m))
        i = rng.choice([i for i in range(K) if i not in at])      # and one base becomes another
        m = bytearray(k)
        m[i] = rng.choice([x for x in b"ACGT" if x != k[i]])
        recs.append(bytes(m))
    for k in w.absent:
        recs += [k, k.translate(WIDE_COMP)[::-1], _flank(rng, k)]
    recs += _synth.fuzz_stream(rng, w.long_recs[0], 200, p_junk=0.01, min_len=0, max_len=120).split(b"\n")[:-1]
    rng.shuffle(recs)
    w.recs = recs
    w.stream = b"\n".join(recs) + b"\n"
    return w


# ---- the union ----------------------------------------------------------------------------------------------------------------------
UNION_MEMBERS = 4


@functools.lru_cache(maxsize=None)
def union_wrap():
    """four members of 230 keys each (920 rows: the union gets 1024 slots at table_load_pct = 90 on the first member), 170 of
    each member's keys starting in the last 24 slots of a 1024-slot table -- the union's and, as (h >> 8) & mask addresses
    both, each member's own.  One key is shared by all, 20 by every two neighbours, the rest are a member's own."""
    w = World()
    w.name, w.lg, w.width, w.load_pct = "union_wrap", 10, 24, 90
    n, ns = 1 << w.lg, UNION_MEMBERS
    own_n, pair_n = 129, 20
    pool = np.concatenate([craft_keys(5041, w.lg, n - w.width, n - 1, 1 + ns * pair_n + ns * own_n - 200),
                           craft_keys(5042, w.lg, n - w.width, n - 1, 200, need_u=True)])
    w.absent = craft_keys(5043, w.lg, n - w.width, n - 1, 48, need_u=True)
    assert len(set(pool.tolist()) | set(w.absent.tolist())) == len(pool) + len(w.absent)
    rng = random.Random(5041)
    pool = pool[np.array(rng.sample(range(len(pool)), len(pool)))]
    w.all_key = int(pool[0])
    w.pair = [pool[1 + m * pair_n:1 + (m + 1) * pair_n] for m in range(ns)]
    base = 1 + ns * pair_n
    w.own = [pool[base + m * own_n:base + (m + 1) * own_n] for m in range(ns)]
    w.members = []
    all_key_recs, all_long = [], []
    for m in range(ns):
        mw = World()
        mw.crafted = np.concatenate([[np.uint64(w.all_key)], w.pair[m], w.pair[(m - 1) % ns], w.own[m]]).astype(np.uint64)
        assert len(mw.crafted) == 170
        key_recs = [kmer_bytes(k) for k in mw.crafted]
        rng.shuffle(key_recs)
        mw.key_recs = key_recs
        mw.long_recs = [_synth.rand_dna(rng, 90)]
        mw.strain_recs = key_recs[:84] + mw.long_recs + key_recs[84:]
        mw.sstream = b"\n".join(mw.strain_recs) + b"\n"
        mw.nkeys = 230
        # informative: the key all share, this member's side of the pair it shares with the next one (not the next one's side),
        # and a third of its own
        mw.informative_keys = {w.all_key} | set(w.pair[m].tolist()) | set(w.own[m][::3].tolist())
        w.members.append(mw)
        all_key_recs += key_recs
        all_long += mw.long_recs
    w.union_keys = np.array(sorted({int(k) for mw in w.members for k in mw.crafted}), dtype=np.uint64)
    seen, uniq = set(), []
    for r in all_key_recs:
        if r not in seen:
            seen.add(r)
            uniq.append(r)
    # neighbours in member 0's strain (its first 84 key records stand one behind the other)
    joinable = list(range(0, 82, 2))
    assert uniq[:84] == w.members[0].key_recs[:84]
    w.recs, w.recs_clean = crafted_reads(rng, uniq, joinable, all_long, w.absent, nrandom=300, nlong=100)
    w.stream = b"\n".join(w.recs) + b"\n"
    w.stream_clean = b"\n".join(w.recs_clean) + b"\n"
    return w


# ---- the partitioned pipeline's bins ---------------------------------------------------------------------------------------------------
BIN_TILE = 65536                                                      # SK_BIN_TILE
BIN_NO_ENTRY_KEY = 0xFFFFF                                            # with chunk 4095 in front: the "no entry" word of a segment


@functools.lru_cache(maxsize=None)
def bins():
    """a strain with a tandem repeat of period 16 and with a 16-mer whose bin key is all ones; a batch that holds that 16-mer as
    chunk 4095 of its first bin tile, inside a read that hits, and the repeat over the whole of its third tile (every chunk of
    it falls into one partition, whose segment holds 40)"""
    w = World()
    w.name = "bins"
    rng = random.Random(5051)
    w.x16, w.x_part = craft_bin16(5051, BIN_NO_ENTRY_KEY)
    a, b = _synth.rand_dna(rng, 1500), _synth.rand_dna(rng, 1500)
    g = a + w.x16 + b
    w.unit = _synth.rand_dna(rng, 16)
    w.strain_recs = [g, w.unit * 4]
    w.sstream = b"\n".join(w.strain_recs) + b"\n"
    at = BIN_TILE - 16                                                # chunk 4095 of tile 0
    read = g[len(a) - 60:len(a) + 16 + 60]
    recs, off = [], 0
    while at - 60 - off > 400:
        ln = rng.choice([31, 64, 150])
        s = rng.randrange(len(g) - ln)
        r = g[s:s + ln] if rng.random() < 0.6 else _synth.rand_dna(rng, ln)
        recs.append(_synth.revcomp(r) if rng.random() < 0.5 else r)
        off += len(recs[-1]) + 1
    recs.append(_synth.rand_dna(rng, at - 60 - off - 1))
    off += len(recs[-1]) + 1
    assert off == at - 60
    w.read_index = len(recs)
    recs.append(read)
    off += len(read) + 1
    w.repeat_index = len(recs)
    w.repeat_start = off
    recs.append(w.unit * ((3 * BIN_TILE + 500 - off) // 16))
    recs += [g[100:300], _synth.revcomp(g[1400:1700]), _synth.rand_dna(rng, 100)]
    w.recs = recs
    w.stream = b"\n".join(recs) + b"\n"
    return w
