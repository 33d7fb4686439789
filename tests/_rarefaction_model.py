"""Rarefaction (include/strainer_kmer.h has the rule) in plain Python: the draw of a read pair from its ordinal in the target, T[q] of
a fraction, a pair's class, the keep rule, the subsample of a target's records, and the table's three numbers from a list of hit
lines.  Nothing here calls the library."""
import re

import numpy as np

M32 = 0xFFFFFFFF
MAX = 16
DEFAULT = "1,0.5,0.25,0.125,0.0625,0.03125"
HEADER = b"metagenome\tfraction\tpairs\tunique_kmers\ttotal_hits\n"
_FIELD = re.compile(r"^(\d+\.?\d*|\.\d+)([eE][+-]?\d+)?$")


def draw(i, seed=0):
    """u(i): one 32-bit number per pair ordinal (any non-negative int below 2^64)"""
    x = ((i & M32) ^ (((i >> 32) * 0x9E3779B9) & M32) ^ seed) & M32
    x ^= x >> 16
    x = (x * 0x85EBCA6B) & M32
    x ^= x >> 13
    x = (x * 0xC2B2AE35) & M32
    x ^= x >> 16
    return x


def draws(ordinals, seed=0):
    """draw() over an array of ordinals, as uint64 values below 2^32"""
    i = np.asarray(ordinals, dtype=np.uint64)
    m = np.uint64(M32)
    x = ((i & m) ^ (((i >> np.uint64(32)) * np.uint64(0x9E3779B9)) & m) ^ np.uint64(seed)) & m
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x85EBCA6B)) & m
    x ^= x >> np.uint64(13)
    x = (x * np.uint64(0xC2B2AE35)) & m
    x ^= x >> np.uint64(16)
    return x


def threshold(text):
    """T of one fraction's text"""
    return int(float(text) * 4294967296.0)


def parse_list(text=None):
    """(T, the fields) of a --rarefaction-list; ValueError for everything the rule refuses"""
    fields = (DEFAULT if text is None else text).split(",")
    if not 1 <= len(fields) <= MAX:
        raise ValueError("1 to 16 fractions")
    T = []
    for f in fields:
        if len(f) > 39 or not _FIELD.match(f):
            raise ValueError("not a plain decimal fraction: %r" % f)
        v = float(f)
        if not 0.0 < v <= 1.0:
            raise ValueError("outside (0, 1]: %r" % f)
        t = threshold(f)
        if T and t >= T[-1]:
            raise ValueError("not strictly descending, or two equal T: %r" % f)
        T.append(t)
    return T, fields


def keep(i, t, seed=0):
    """pair i is in the subsample of threshold t"""
    return draw(i, seed) < t


def klass(i, T, seed=0):
    """the number of listed subsamples that hold pair i"""
    u = draw(i, seed)
    return sum(1 for t in T if u < t)


def classes(ordinals, T, seed=0):
    u = draws(ordinals, seed)
    c = np.zeros(len(u), dtype=np.int64)
    for t in T:
        c += u < np.uint64(t)
    return c


def npairs(files, mode):
    """the pairs of a target: every record counts; PE counts the mate-1 file's records, PEI two records a pair (a last record
    without a mate is a pair)"""
    n = len(files[0])
    return (n + 1) // 2 if mode == "PEI" else n


def subsample(files, mode, t, seed=0):
    """files: the target's records per file (PE: two lists, else one).  The records of the pairs in the subsample of threshold t, in
    order, per file."""
    if mode == "PEI":
        return [[r for k, r in enumerate(files[0]) if keep(k // 2, t, seed)]]
    return [[r for k, r in enumerate(f) if keep(k, t, seed)] for f in files]


# the library-level world of tests/test_coverage_rarefaction_gpu.py, built here so that tests/test_coverage_rarefaction_host.py can check
# its premises on the model alone
SIZES = [0, 1, 255, 257, 70001]
LISTS = ["1", "1,0.5", "0.75,0.1", "1,0.9,0.8,0.7,0.6,0.5,0.4,0.3,0.2,0.15,0.1,0.07,0.05,0.03,0.02,0.01"]
SEEDS = [0, 0x9E3779B9]
EDGE = 1 << 32
MIN_HITS = 2


def library_world(which):
    """-> (entries per member of SIZES: (rows, totals, ordinals), pair ranges [(first, n)]).  Ordinals around 0, 2^32 - 1 and 2^32 and
    anywhere below 2^64; totals at, below and above MIN_HITS; every row once where there is room, extras on random rows."""
    rng = np.random.default_rng(1000 + which)
    near = np.concatenate([np.arange(0, 700), np.arange(EDGE - 700, EDGE + 700)]).astype(np.uint64)
    entries = []
    for n in SIZES:
        if not n:
            entries.append((np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.uint64)))
            continue
        rows = np.concatenate([np.arange(n), rng.integers(0, n, min(3 * n, 5000) + 7)]).astype(np.uint32)
        far = rng.integers(0, 1 << 63, len(rows), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, len(rows), dtype=np.uint64)
        ords = np.where(rng.random(len(rows)) < 0.5, rng.choice(near, len(rows)), far).astype(np.uint64)
        totals = rng.choice([0, MIN_HITS, MIN_HITS + 1, 40, 0xFFFFFFFF], len(rows)).astype(np.uint32)
        entries.append((rows, totals, ords))
    ranges = [(0, 1000), (EDGE - 300, 70001), ((1 << 64) - 5000, 5000)]
    return entries, ranges


def world_ordinals(ranges):
    return np.concatenate([np.arange(n, dtype=np.uint64) + np.uint64(first) for first, n in ranges])


def table(lines, T, seed, min_hits, pair_ordinals):
    """lines: (pair ordinal, row, pair total) per hit line of one strain and target; pair_ordinals: the target's pairs.
    -> (pairs[q], unique[q], total[q])"""
    pc = classes(np.asarray(pair_ordinals, dtype=np.uint64), T, seed)
    pairs = [int((pc > q).sum()) for q in range(len(T))]
    if not len(lines):
        return pairs, [0] * len(T), [0] * len(T)
    a = np.asarray(lines, dtype=np.uint64).reshape(-1, 3)
    ok = a[:, 2].astype(np.int64) > min_hits
    c = classes(a[ok, 0], T, seed)
    rows = a[ok, 1]
    return (pairs, [len(np.unique(rows[c > q])) for q in range(len(T))], [int((c > q).sum()) for q in range(len(T))])
