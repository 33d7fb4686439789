"""Python model of strain_detect --coverage-regions (include/strainer_kmer.h has the rule): the records of a strain file, its region
table, every canonical 31-mer's first position along the text, and the table the program must write -- computed from the strain
file, the informative k-mer list and a hit list (what --coverage-depth writes at -o, or the reference's own), with nothing of the
library in it."""
import bisect
import gzip
import os
import re

import numpy as np

K = 31
NO_POS = 0xFFFFFFFF
HEADER = (b"strain_name\tmetagenome\tregion\trecord_name\tregion_informative_kmers\tunique_observed_informative_kmers\t"
          b"total_observed_informative_kmers\tkmer_coverage\tkmer_depth\n")


def model_records(text):
    """(name, sequence) of every record of a FASTA/FASTQ text, by the reference's grammar (src/kseq.h:166-211) for well-formed
    files: a header starts a record, its name ends at the first white space; FASTA sequence lines are joined up to the next header,
    a FASTQ record's quality holds as many bytes as its sequence"""
    lines = text.split(b"\n")
    out, i = [], 0
    while i < len(lines):
        ln = lines[i]
        if not ln or ln[:1] not in (b">", b"@"):
            i += 1
            continue
        name = re.match(rb"\S*", ln[1:]).group(0)
        i += 1
        seq = []
        while i < len(lines) and lines[i][:1] not in (b">", b"@", b"+"):
            seq.append(lines[i].rstrip(b"\r"))
            i += 1
        seq = b"".join(seq)
        if i < len(lines) and lines[i][:1] == b"+":
            i += 1
            q = 0
            while i < len(lines) and q < len(seq):
                q += len(lines[i].rstrip(b"\r"))
                i += 1
        out.append((name, seq))
    return out


def model_regions(records, w):
    """([(text offset, record number from 1, offset in the record, length, record name)], text length)"""
    regs, off = [], 0
    for num, (name, seq) in enumerate(records, 1):
        if len(seq) < K - 1:
            continue
        step = w if w else len(seq)
        for a in range(0, len(seq), step):
            regs.append((off + a, num, a, min(a + step, len(seq)) - a, name))
        off += len(seq)
    return regs, off


_CODE = np.full(256, 4, dtype=np.uint8)
for _i, _c in enumerate(b"ACGT"):
    _CODE[_c] = _i
    _CODE[_c | 0x20] = _i


def keys_of(kmers):
    """canonical 62-bit keys of 31-byte A/C/G/T words (the larger of the word and its reverse complement)"""
    if not len(kmers):
        return np.zeros(0, dtype=np.uint64)
    c = _CODE[np.frombuffer(b"".join(kmers), dtype=np.uint8)].reshape(-1, K).astype(np.uint64)
    assert (c < 4).all()
    fwd = np.zeros(len(c), dtype=np.uint64)
    rc = np.zeros(len(c), dtype=np.uint64)
    for j in range(K):
        fwd = (fwd << np.uint64(2)) | c[:, j]
        rc |= (np.uint64(3) - c[:, j]) << np.uint64(2 * j)
    return np.maximum(fwd, rc)


def first_positions(records):
    """(sorted canonical keys, text position of each key's first window) over the windows of 31 A/C/G/T bases that lie inside one
    kept record"""
    seqs = [s for _, s in records if len(s) >= K - 1]
    text = np.frombuffer(b"".join(seqs), dtype=np.uint8)
    n = len(text)
    if n < K:
        return np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.int64)
    code = _CODE[text]
    cs = np.concatenate([[0], np.cumsum(code > 3)])
    m = n - K + 1
    ok = (cs[K:] - cs[:m]) == 0
    end = 0
    for s in seqs:
        end += len(s)
        ok[max(end - K + 1, 0): min(end, m)] = False           # (windows that would run into the next record)
    c = (code & 3).astype(np.uint64)
    fwd = np.zeros(m, dtype=np.uint64)
    rc = np.zeros(m, dtype=np.uint64)
    for j in range(K):
        fwd = (fwd << np.uint64(2)) | c[j: j + m]
        rc |= (np.uint64(3) - c[j: j + m]) << np.uint64(2 * j)
    canon = np.maximum(fwd, rc)
    idx = np.nonzero(ok)[0]
    uk, first = np.unique(canon[idx], return_index=True)
    return uk, idx[first]


def region_of_pos(pos, starts):
    """region of each text position (NO_POS: the unplaced one, len(starts))"""
    pos = np.asarray(pos, dtype=np.int64)
    starts = np.asarray(starts, dtype=np.int64)
    r = np.searchsorted(starts, pos, side="right") - 1
    return np.where((pos == NO_POS) | (r < 0), len(starts), r)


class StrainModel:
    def __init__(self, strain_text, window):
        self.records = model_records(strain_text)
        self.regions, self.text_bases = model_regions(self.records, window)
        self.starts = np.array([r[0] for r in self.regions], dtype=np.int64)
        self.keys, self.pos = first_positions(self.records)

    def regions_of(self, kmers):
        """region of each k-mer (bytes), len(regions) for one the text does not hold"""
        k = keys_of(kmers)
        at = np.searchsorted(self.keys, k)
        at[at >= len(self.keys)] = 0
        have = len(self.keys) > 0
        found = (self.keys[at] == k) if have else np.zeros(len(k), dtype=bool)
        pos = np.where(found, self.pos[at] if have else 0, NO_POS)
        return region_of_pos(pos, self.starts), k


def _open(path):
    with open(path, "rb") as f:
        gz = f.read(2) == b"\x1f\x8b"
    return gzip.open(path, "rb") if gz else open(path, "rb")


def expected_table(strain_path, inf_path, hits_path, depth_table, window, min_kmer_hits=1):
    """the bytes --coverage-regions must write: targets in the order of the coverage table's lines, regions in text order, only
    regions with an informative row; a hit line counts iff h1 + h2 > min_kmer_hits"""
    with _open(strain_path) as f:
        sm = StrainModel(f.read(), window)
    with _open(inf_path) as f:
        inf = sorted({ln.split(b"\t")[0].strip().upper() for ln in f.read().splitlines() if ln and not ln.startswith(b"#") and len(ln.split(b"\t")[0].strip()) == K})
    nb = len(sm.regions) + 1
    reg, keys = sm.regions_of(inf)
    _, uniq_at = np.unique(keys, return_index=True)
    placed = reg[uniq_at]
    reg_inf = np.bincount(placed[placed < nb - 1], minlength=nb)      # (a listed k-mer the strain does not hold is no row)
    samples, kmers, sidx = {}, [], []
    with _open(hits_path) as f:
        for ln in f.read().splitlines():
            if not ln or ln.startswith(b"#"):
                continue
            fld = ln.split(b"\t")
            if int(fld[1]) + int(fld[3]) > min_kmer_hits:
                sidx.append(samples.setdefault(os.path.basename(fld[0]), len(samples)))
                kmers.append(fld[5])
    uq = np.zeros((len(samples) + 1, nb), dtype=np.int64)
    tot = np.zeros((len(samples) + 1, nb), dtype=np.int64)
    if kmers:
        r, k = sm.regions_of(kmers)
        s = np.array(sidx, dtype=np.int64)
        np.add.at(tot, (s, r), 1)
        pairs = np.unique(np.stack([s.astype(np.uint64), k, r.astype(np.uint64)], axis=1), axis=0)
        np.add.at(uq, (pairs[:, 0].astype(np.int64), pairs[:, 2].astype(np.int64)), 1)
    rows = [ln.split(b"\t") for ln in depth_table.splitlines()[1:]]
    out = [HEADER]
    for row in rows:
        s = samples.get(row[5], len(samples))                  # (a target without a passing line: zeros)
        for r in range(nb):
            if not reg_inf[r]:
                continue
            if r < nb - 1:
                _, num, a, ln, name = sm.regions[r]
                label, rname = b"%d:%d-%d" % (num, a, a + ln), name
            else:
                label, rname = b"unplaced", b"-"
            u, t, d = int(uq[s, r]), int(tot[s, r]), int(reg_inf[r])
            out.append(b"\t".join([row[0], row[5], label, rname, b"%d" % d, b"%d" % u, b"%d" % t, repr(u / d).encode(), repr(t / d).encode()]) + b"\n")
    return b"".join(out)
