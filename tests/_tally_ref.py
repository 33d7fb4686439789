"""TALLY reference (strain_detect's per-record view of the scan) built on the CPU oracle, and the checks of a device
result against it.  TEST INFRASTRUCTURE, imported by the tests only.

For a batch (a record stream and the offsets its records start at) and one strain with a set of informative rows:
  * per record, (windows that hit any key, those whose key is informative): the per-row differences of the oracle's
    counters when the records are scanned one at a time -- so U, IUPAC letters, N, '\\r' and lower case mean what the
    oracle says they mean, nothing is restated here;
  * the log of informative hits as a multiset of (record, row): the informative entries of the same differences.
The positions a device log names are checked separately (check_log): each lies inside its record, and the windows
stream[pos-30:pos+1], scanned by the oracle as reads of their own in one pass, hit exactly the logged rows.

canonical_tally is a second, numpy reference for large batches of A/C/G/T (either case), N and newlines only: it
knows the position of every hit, so it gives the log exactly."""
import collections

import numpy as np

import _oracle

K = 31


def record_bounds(stream, rec_start):
    """(start, end) of every record: a record ends where the next one starts (the last at the end of the stream)"""
    s = np.asarray(rec_start, dtype=np.int64)
    e = np.append(s[1:], len(stream))
    return s, e


def starts_of(recs):
    """offsets of the records of b"\\n".join(recs) + b"\\n\""""
    return np.cumsum([0] + [len(r) + 1 for r in recs[:-1]]).astype(np.uint32)


class OracleStrain:
    """one strain's key set in the oracle (rows in the order the product numbers them: callers assert it)"""

    def __init__(self, sstream, capacity=8000000):
        """capacity: the table's first size (the product's initial_slots: the row order follows it); a small one makes the
        per-record passes over the table cheap"""
        self.t = _oracle.OracleTable(capacity=capacity, ncols=3)
        assert self.t.build_stream(sstream, default=1, incr=0, short_policy=1) == 0
        self.keys = self.t.rows()[0]
        self.nrows = len(self.keys)
        self.row_of = {k: i for i, k in enumerate(self.keys)}
        self._now = self.t.counts().astype(np.int64)             # (the counters as they stand: one fetch per scan)

    def _delta(self, data, col):
        """how column `col` moves when `data` is scanned into it"""
        self.t.scan_stream(data, col)
        now = self.t.counts()[:, col].astype(np.int64)
        d = now - self._now[:, col]
        self._now[:, col] = now
        return d

    def tally(self, stream, rec_start, informative):
        """(tally[nrec, 2], Counter{(record, row): informative hits}) -- informative: bool[nrows]"""
        informative = np.asarray(informative, dtype=bool)
        assert informative.shape == (self.nrows,)
        s, e = record_bounds(stream, rec_start)
        tally = np.zeros((len(s), 2), dtype=np.int64)
        log = collections.Counter()
        if self.nrows == 0:
            return tally, log
        for r in range(len(s)):
            if e[r] - s[r] < K:                                # (no window fits)
                continue
            d = self._delta(stream[s[r]:e[r]], 1)
            assert d.min() >= 0
            tally[r, 0] = d.sum()
            tally[r, 1] = d[informative].sum()
            for row in np.nonzero(d * informative)[0]:
                log[(r, int(row))] += int(d[row])
        return tally, log

    def window_rows(self, stream, pos):
        """Counter{row: hits} of the windows ending at `pos`, each scanned as a read of its own, in one pass"""
        if len(pos) == 0 or self.nrows == 0:
            return collections.Counter()
        data = b"\n".join(stream[p - (K - 1):p + 1] for p in pos) + b"\n"
        d = self._delta(data, 2)
        return collections.Counter({int(r): int(d[r]) for r in np.nonzero(d)[0]})


def check_log(strain, stream, rec_start, hits, want_log, what=""):
    """a device log hits[n, 2] = (window-end offset, row) against the reference multiset want_log{(record, row): n}"""
    hits = np.asarray(hits, dtype=np.int64).reshape(-1, 2)
    s, e = record_bounds(stream, rec_start)
    pos, rows = hits[:, 0], hits[:, 1]
    assert len(np.unique(pos)) == len(pos), (what, "a window logged twice")
    rec = np.searchsorted(s, pos, side="right") - 1
    assert (rec >= 0).all(), what
    assert (pos >= s[rec] + (K - 1)).all() and (pos < e[rec]).all(), (what, "a logged window outside its record")
    got = collections.Counter(zip(rec.tolist(), rows.tolist()))
    assert got == want_log, (what, sorted((got - want_log).items())[:5], sorted((want_log - got).items())[:5])
    assert strain.window_rows(stream, pos.tolist()) == collections.Counter(rows.tolist()), (what, "a logged position does not hit its row")


def check_single(strain, stream, rec_start, want, tally, hits, what=""):
    """one table's result (tally[nrec, 2], hits[n, 2]) against want = strain.tally(...)"""
    wt, wl = want
    assert np.array_equal(np.asarray(tally, dtype=np.int64), wt), (what, np.nonzero((np.asarray(tally) != wt).any(axis=1))[0][:10])
    assert len(hits) == int(wt[:, 1].sum()), what
    check_log(strain, stream, rec_start, hits, wl, what)


# ---- the numpy reference for large batches of A/C/G/T, N and newlines ----------------------------------------------
_CODE = np.full(256, 255, dtype=np.uint8)
for _i, _b in enumerate(b"ACGT"):
    _CODE[_b] = _CODE[_b | 0x20] = _i


def canonical_tally(packed_keys, informative, stream, rec_start):
    """(tally[nrec, 2], log[n, 2] = (window-end offset, row) sorted by offset) of a batch whose bytes are A/C/G/T in either
    case, N/n and newlines: a window is 31 bases in a row, its key the larger of its 2-bit code and its reverse complement's"""
    code = _CODE[np.frombuffer(stream, dtype=np.uint8)]
    assert np.isin(np.frombuffer(stream, dtype=np.uint8)[code == 255], np.frombuffer(b"Nn\n", dtype=np.uint8)).all(), \
        "canonical_tally: A/C/G/T, N and newlines only"
    s, _ = record_bounds(stream, rec_start)
    nrec = len(s)
    tally = np.zeros((nrec, 2), dtype=np.int64)
    n = len(code)
    if n < K:
        return tally, np.zeros((0, 2), dtype=np.int64)
    bad = np.concatenate([[0], np.cumsum(code == 255)])
    ends = np.arange(K - 1, n)
    ok = bad[ends + 1] - bad[ends - (K - 1)] == 0
    ends = ends[ok]
    c = code.astype(np.uint64)
    fwd = np.zeros(len(ends), dtype=np.uint64)
    rc = np.zeros(len(ends), dtype=np.uint64)
    for i in range(K):
        b = c[ends - (K - 1) + i]
        fwd = (fwd << np.uint64(2)) | b
        rc |= (np.uint64(3) - b) << np.uint64(2 * i)
    canon = np.maximum(fwd, rc)
    keys = np.asarray(packed_keys, dtype=np.uint64)
    order = np.argsort(keys, kind="stable")
    sk = keys[order]
    at = np.minimum(np.searchsorted(sk, canon), len(sk) - 1)
    found = sk[at] == canon if len(sk) else np.zeros(len(canon), dtype=bool)
    pos, row = ends[found], order[at[found]]
    rec = np.searchsorted(s, pos, side="right") - 1
    inf = np.asarray(informative, dtype=bool)[row]
    tally[:, 0] = np.bincount(rec, minlength=nrec)
    tally[:, 1] = np.bincount(rec[inf], minlength=nrec)
    return tally, np.stack([pos[inf], row[inf]], axis=1).astype(np.int64)


def check_exact(want, tally, hits, what=""):
    """a device result against canonical_tally's: tallies, and the log entry by entry (sorted)"""
    wt, wl = want
    t = np.asarray(tally, dtype=np.int64)
    assert np.array_equal(t, wt), (what, np.nonzero((t != wt).any(axis=1))[0][:10])
    h = np.asarray(hits, dtype=np.int64).reshape(-1, 2)
    h = h[np.lexsort((h[:, 1], h[:, 0]))]
    assert np.array_equal(h, wl), (what, len(h), len(wl))
