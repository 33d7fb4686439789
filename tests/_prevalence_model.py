"""The prevalence rule (include/strainer_kmer.h at sk_item_fold) restated over the CPU oracle: every item of a list is scanned by
OracleTable.scan_file into a zeroed column of its own, and with the item's column v
    prev += (v >= m), kmers_present = sum(v >= m), kmer_hits = sum(v).
TEST INFRASTRUCTURE: ground truth is the oracle run item by item, never the code under test."""
import os

import numpy as np

import _oracle

HEADER = b"#kmer\treference_count\tpangenome_count\tmetagenome_count\tdrug_count\n"
ITEMS_HEADER = b"#list\tline\tfile\tbases\tkmers_present\tkmer_hits\n"


def list_items(list_path, skip=None):
    """(1-based line, text) of every line of the list that is an item: all but the line equal to `skip`"""
    with open(list_path, "rb") as f:
        lines = f.read().split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    return [(i + 1, ln.decode()) for i, ln in enumerate(lines) if skip is None or ln.decode() != skip]


class Model:
    """strain: the -r file; lists: the -A, -B and (or None) -C list files; cwd: the directory the program runs in"""

    def __init__(self, strain, lists, min_count=1, cwd="."):
        here = os.getcwd()
        os.chdir(cwd)
        try:
            self.m = int(min_count)
            self.items = []                       # (list letter, line, file, bases, column)
            per_list = [list_items(p, strain if k == 2 else None) if p else [] for k, p in enumerate(lists)]
            n = sum(len(x) for x in per_list)
            t = _oracle.OracleTable(ncols=1 + n)  # column 0 the reference count, then a zeroed column per item
            assert t.build_file(strain, short_policy=1) == 0      # (a strain record shorter than k - 1 is skipped, as the program skips it)
            col = 1
            for k, its in enumerate(per_list):
                for line, path in its:
                    self.items.append(["ABC"[k], line, path, t.scan_file(path, col), col])
                    col += 1
            self.keys, c = t.rows()
            t.close()
        finally:
            os.chdir(here)
        c = c.astype(np.uint32)
        self.ref = c[:, 0].copy()
        self.with_drug = lists[2] is not None
        self.n_items = [len(x) for x in per_list]
        self.count = np.zeros((len(self.keys), 3), dtype=np.uint32)
        self.prev = np.zeros((len(self.keys), 3), dtype=np.uint32)
        self.records = []                         # (list letter, line, file, bases, kmers_present, kmer_hits)
        for letter, line, path, bases, col in self.items:
            v = c[:, col]
            k = "ABC".index(letter)
            self.count[:, k] += v
            self.prev[:, k] += (v >= self.m).astype(np.uint32)
            self.records.append((letter, line, path, int(bases), int((v >= self.m).sum()), int(v.astype(np.uint64).sum())))

    def _table(self, cols, extra=b""):
        nf = 3 if self.with_drug else 2
        out = [HEADER, extra]
        for r, key in enumerate(self.keys):
            out.append(key + b"\t" + b"\t".join(str(int(np.int32(x))).encode() for x in [self.ref[r]] + list(cols[r, :nf])) + b"\n")
        return b"".join(out)

    def count_table(self):
        """what the program prints on stdout"""
        return self._table(self.count)

    def prevalence_file(self):
        extra = b"#items\t%d\t%d\t%d\n#min_count\t%d\n" % (self.n_items[0], self.n_items[1], self.n_items[2], self.m)
        return self._table(self.prev, extra)

    def items_file(self):
        return ITEMS_HEADER + b"".join(("%s\t%d\t%s\t%d\t%d\t%d\n" % r).encode() for r in self.records)


def check_identities(prevalence_file, items_file, count_table):
    """the sum of kmer_hits is the count column's sum and the sum of kmers_present the prevalence column's, per list"""
    def cols(text):
        rows = [ln.split(b"\t") for ln in text.split(b"\n") if ln and not ln.startswith(b"#")]
        return np.array([[int(x) & 0xFFFFFFFF for x in r[2:]] for r in rows], dtype=np.uint64).reshape(len(rows), -1)
    pc, cc = cols(prevalence_file), cols(count_table)
    present, hits = [0, 0, 0], [0, 0, 0]
    for ln in items_file.split(b"\n")[1:]:
        if ln:
            f = ln.split(b"\t")
            present["ABC".index(f[0].decode())] += int(f[4])
            hits["ABC".index(f[0].decode())] += int(f[5])
    for k in range(pc.shape[1]):
        assert present[k] == int(pc[:, k].sum()), ("kmers_present", k)
        assert hits[k] == int(cc[:, k].sum()), ("kmer_hits", k)
