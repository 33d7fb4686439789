"""The background of step 4's numbers (sk_scan_batch, sk_background_finish, sk_union_background_finish, strain_detect
--coverage-background; include/strainer_kmer.h has the rule) in Python: the model every background test compares against.  The
reference has no counterpart.

key_of(window)             a 31-byte window's key text (upper case, the larger of the window and its reverse complement in the
                           reference's complement map), or None for a window with an N
strain_keys(records)       a strain's distinct keys in first-occurrence order
row_counts(keys, records)  c[row]: one per window of any record whose key is the row's
block(counts, inf, D)      uint64[2, 5 + D + 1], the layout of sk_background_finish: row 0 informative, row 1 background; columns
                           kmers, covered_kmers, total_hits, rows above D, hits above D, rows at depth 0..D
check_block(b)             the invariants every block obeys
table(..), spectrum(..)    the two tables' bytes;  parse_table(..), parse_spectrum(..)  the way back"""
import os

import numpy as np

K = 31
HEAD = 5
HEADER = b"strain_name\tmetagenome\tclass\tkmers\tcovered_kmers\ttotal_hits\n"
SPECTRUM_HEADER = b"strain_name\tmetagenome\tclass\tdepth\tkmers\thits\n"
CLASSES = ("informative", "background")

# the reference's complement map (src/BIO_sequence.c:203-213) over the letters the model's worlds use: upper-case K maps to '.',
# U to A -- the quirks the library reproduces
_FROM = b"-.^ATCGBVDHKMNRYSUWX"
_TO = b"-.^TAGCVBHD.KNYRSAWX"
_COMP = bytes.maketrans(_FROM, _TO)


def key_of(window: bytes):
    w = window.upper()
    assert len(w) == K and all(c in _FROM for c in w), "the model knows the complement map's letters only"
    if b"N" in w:
        return None
    return max(w, w.translate(_COMP)[::-1])


def windows(record: bytes):
    """a record shorter than k has no window"""
    for i in range(len(record) - K + 1):
        k = key_of(record[i:i + K])
        if k is not None:
            yield k


def strain_keys(records):
    seen = {}
    for r in records:
        for k in windows(r):
            seen.setdefault(k, len(seen))
    return list(seen)


def row_counts(keys, records):
    row = {k: i for i, k in enumerate(keys)}
    c = np.zeros(len(keys), dtype=np.uint64)
    for r in records:
        for k in windows(r):
            i = row.get(k)
            if i is not None:
                c[i] += 1
    return c


def block(counts, informative, max_depth):
    """counts[row] (any unsigned width), informative[row] (bool) -> the block"""
    counts = np.asarray(counts, dtype=np.uint64)
    informative = np.asarray(informative, dtype=bool)
    D = int(max_depth)
    out = np.zeros((2, HEAD + D + 1), dtype=np.uint64)
    for c, sel in enumerate((informative, ~informative)):
        v = counts[sel]
        deep = v > np.uint64(D)
        out[c, 0] = v.size
        out[c, 1] = int((v > 0).sum())
        out[c, 2] = sum(int(x) for x in v[v > 0])
        out[c, 3] = int(deep.sum())
        out[c, 4] = sum(int(x) for x in v[deep])
        out[c, HEAD:] = np.bincount(v[~deep].astype(np.int64), minlength=D + 1)[: D + 1]
    return out


def check_block(b):
    """bins + deep rows == kmers; sum d * bins + deep hits == total_hits; kmers - bins[0] == covered_kmers"""
    b = np.asarray(b)
    D = b.shape[-1] - HEAD - 1
    for c in range(2):
        o = [int(x) for x in b[c]]
        assert sum(o[HEAD:]) + o[3] == o[0], (c, o[:HEAD])
        assert sum(d * o[HEAD + d] for d in range(D + 1)) + o[4] == o[2], (c, o[:HEAD])
        assert o[0] - o[HEAD] == o[1], (c, o[:HEAD])
        assert o[4] >= o[3] * (D + 1)


def strain_name(hits_file_name):
    n = os.path.basename(hits_file_name)
    return n[:-13] if len(n) >= 13 and n[-12:-3] == "kmer_hits" and n[-2:] == "gz" else n


def table(strain, blocks):
    """blocks: [(metagenome basename, block)] in run order"""
    out = [HEADER]
    for meta, b in blocks:
        for c in range(2):
            out.append(b"%s\t%s\t%s\t%d\t%d\t%d\n" % (strain.encode(), meta.encode(), CLASSES[c].encode(), int(b[c, 0]), int(b[c, 1]), int(b[c, 2])))
    return b"".join(out)


def spectrum(strain, blocks):
    out = [SPECTRUM_HEADER]
    for meta, b in blocks:
        D = b.shape[1] - HEAD - 1
        for c in range(2):
            pre = b"%s\t%s\t%s\t" % (strain.encode(), meta.encode(), CLASSES[c].encode())
            for d in range(D + 1):
                out.append(pre + b"%d\t%d\t%d\n" % (d, int(b[c, HEAD + d]), int(b[c, HEAD + d]) * d))
            out.append(pre + b">%d\t%d\t%d\n" % (D, int(b[c, 3]), int(b[c, 4])))
    return b"".join(out)


def parse_table(raw: bytes):
    """-> {(strain, metagenome, class): (kmers, covered_kmers, total_hits)}, and the keys in file order"""
    lines = raw.split(b"\n")
    assert lines[0] + b"\n" == HEADER and lines[-1] == b"", "header line / final newline"
    out, order = {}, []
    for ln in lines[1:-1]:
        s, m, c, a, b, t = ln.decode().split("\t")
        assert c in CLASSES and (s, m, c) not in out
        out[(s, m, c)] = (int(a), int(b), int(t))
        order.append((s, m, c))
    return out, order


def parse_spectrum(raw: bytes):
    """-> {(strain, metagenome, class): block row as a list [kmers, covered, total, deep rows, deep hits, bins...]}"""
    lines = raw.split(b"\n")
    assert lines[0] + b"\n" == SPECTRUM_HEADER and lines[-1] == b""
    rows = {}
    for ln in lines[1:-1]:
        s, m, c, d, n, h = ln.decode().split("\t")
        rows.setdefault((s, m, c), []).append((d, int(n), int(h)))
    out = {}
    for key, r in rows.items():
        assert r[-1][0].startswith(">") and [x[0] for x in r[:-1]] == [str(i) for i in range(len(r) - 1)], key
        assert int(r[-1][0][1:]) == len(r) - 2
        bins = [x[1] for x in r[:-1]]
        for d, (_, n, h) in enumerate(r[:-1]):
            assert h == n * d, (key, d)
        kmers = sum(bins) + r[-1][1]
        out[key] = [kmers, kmers - bins[0], sum(x[2] for x in r), r[-1][1], r[-1][2]] + bins
    return out


def blocks_of_tables(table_raw, spectrum_raw=None):
    """the table (and the spectrum) of one run, checked against each other: the spectrum's sums are the table's numbers"""
    t, order = parse_table(table_raw)
    for i in range(0, len(order), 2):
        assert order[i][:2] == order[i + 1][:2] and (order[i][2], order[i + 1][2]) == CLASSES, "informative, then background, per target"
    if spectrum_raw is not None:
        sp = parse_spectrum(spectrum_raw)
        assert set(sp) == set(t)
        for key, row in sp.items():
            assert tuple(row[:3]) == t[key], (key, row[:3], t[key])
    return t, order
