"""Recurrence (include/strainer_kmer.h has the rule) in Python: the model every recurrence test compares against.

recurrence(planes)           bool[T, nbits] -> (n[0..T]: bit positions set in exactly m planes, shared[T, T] = planes @ planes.T)
check_tables(hist, shared)   the rule's invariants on a pair of tables
tables_from_hits(text, ..)   the text of a hit list (strain_detect's -o file, decompressed) -> the bytes of both tables"""
import numpy as np

from _spectrum_model import read_hits, strain_name

HIST_HEADER = b"strain_name\tsamples\tseen_in\tinformative_kmers\n"
PAIRS_HEADER = b"strain_name\tmetagenome_a\tmetagenome_b\tshared_informative_kmers\teither_informative_kmers\n"


def recurrence(planes, pairs=True):
    """planes: bool[T, nbits].  Returns (hist, shared): hist[m] = columns with exactly m planes set (m = 0..T), shared[i, j] =
    columns set in planes i and j (None without pairs)"""
    p = np.asarray(planes, dtype=bool)
    T = p.shape[0]
    hist = np.bincount(p.sum(axis=0, dtype=np.int64), minlength=T + 1).astype(np.uint64)
    if not pairs:
        return hist, None
    q = p.astype(np.float64)                                  # (exact: every sum is far below 2^53)
    return hist, np.rint(q @ q.T).astype(np.uint64)


def check_tables(hist, shared, nbits=None):
    hist, shared = np.asarray(hist).astype(np.int64), np.asarray(shared).astype(np.int64)
    diag = np.diagonal(shared)
    assert int((np.arange(len(hist)) * hist).sum()) == int(diag.sum())
    if nbits is not None:
        assert int(hist.sum()) == int(nbits)
    assert np.array_equal(shared, shared.T)
    assert (shared <= np.minimum(diag[:, None], diag[None, :])).all()


def tables_from_hits(text, hits_file_name, min_hits=1):
    """-> (the histogram table's bytes, the pair table's bytes).  I is the total_genome_informative_kmers trailer of the first
    sample, in the main table's order, that has one; without one no 0 line is printed"""
    name = strain_name(hits_file_name).encode()
    order, depth, inf = read_hits(text, min_hits)
    T = len(order)
    kmers = sorted({k for s in order for k in depth.get(s, {})})
    col = {k: i for i, k in enumerate(kmers)}
    planes = np.zeros((T, len(kmers)), dtype=bool)
    for i, s in enumerate(order):
        for k in depth.get(s, {}):
            planes[i, col[k]] = True
    hist, shared = recurrence(planes)
    known = [inf[s] for s in order if s in inf]
    out = [HIST_HEADER]
    if known:
        out.append(b"%s\t%d\t0\t%d\n" % (name, T, known[0] - int(hist[1:].sum())))
    for m in range(1, T + 1):
        if hist[m]:
            out.append(b"%s\t%d\t%d\t%d\n" % (name, T, m, int(hist[m])))
    pr = [PAIRS_HEADER]
    for i in range(T):
        for j in range(i, T):
            sh = int(shared[i, j])
            pr.append(b"%s\t%s\t%s\t%d\t%d\n" % (name, order[i], order[j], sh, int(shared[i, i]) + int(shared[j, j]) - sh))
    return b"".join(out), b"".join(pr)
