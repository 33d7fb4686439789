"""The depth spectrum (include/strainer_kmer.h has the rule) in Python: the model every spectrum test compares against.

spectrum(depth, D)         a depth array -> (n[1..D] and n[>D] as D + 1 numbers, hits[>D])
table_from_hits(text, ..)  the text of a hit list (strain_detect's -o file, decompressed) -> the table's bytes
parse_table / main_table   the spectrum table and the main coverage table as dictionaries, for the invariants"""
import os

import numpy as np


def spectrum(depth, D):
    """depth: one count per row.  Returns (bins, deep): bins[d - 1] = rows with count d for 1 <= d <= D, bins[D] = rows with a
    count above D, deep = the sum of the counts above D"""
    depth = np.asarray(depth, dtype=np.int64)
    bins = np.bincount(np.minimum(depth, D + 1), minlength=D + 2)[1:].astype(np.uint64)
    return bins, int(depth[depth > D].sum())


def strain_name(hits_file_name):
    """the script's strain name: the file's basename without a trailing '<any>kmer_hits<any>gz'"""
    n = os.path.basename(hits_file_name)
    return n[:-13] if len(n) >= 13 and n[-12:-3] == "kmer_hits" and n[-2:] == "gz" else n


def read_hits(text, min_hits=1):
    """-> (samples in the main table's order, {sample: {k-mer text: depth}}, {sample: I})"""
    order, depth, evaluated, inf = [], {}, [], {}
    for line in text.split(b"\n"):
        if not line:
            continue
        if line.startswith(b"#"):
            f = line.rstrip().split(b"\t")
            s = os.path.basename(f[0][1:])
            if f[1] == b"total_kmer_evaluated" and s not in evaluated:
                evaluated.append(s)
            if f[1] == b"total_genome_informative_kmers":
                inf[s] = int(f[2])
            continue
        f = line.split(b"\t")
        if not int(f[1]) + int(f[3]) > min_hits:
            continue
        s = os.path.basename(f[0])
        if s not in depth:
            depth[s] = {}
            order.append(s)
        depth[s][f[5]] = depth[s].get(f[5], 0) + 1
    return order + [s for s in evaluated if s not in depth], depth, inf


def table_from_hits(text, hits_file_name, D=255, min_hits=1):
    name = strain_name(hits_file_name).encode()
    order, depth, inf = read_hits(text, min_hits)
    out = [b"strain_name\tmetagenome\tdepth\tinformative_kmers\tobserved_hits\n"]
    for s in order:
        bins, deep = spectrum(list(depth.get(s, {}).values()), D)
        if s in inf:
            out.append(b"%s\t%s\t0\t%d\t0\n" % (name, s, inf[s] - int(bins.sum())))
        for d in range(1, D + 1):
            if bins[d - 1]:
                out.append(b"%s\t%s\t%d\t%d\t%d\n" % (name, s, d, int(bins[d - 1]), d * int(bins[d - 1])))
        if bins[D]:
            out.append(b"%s\t%s\t>%d\t%d\t%d\n" % (name, s, D, int(bins[D]), deep))
    return b"".join(out)


def parse_table(table):
    """-> {sample: [(depth label, informative_kmers, observed_hits)]}, samples in the table's order"""
    lines = table.split(b"\n")
    assert lines[0] == b"strain_name\tmetagenome\tdepth\tinformative_kmers\tobserved_hits" and lines[-1] == b""
    out = {}
    for ln in lines[1:-1]:
        f = ln.split(b"\t")
        assert len(f) == 5
        out.setdefault(f[1], []).append((f[2], int(f[3]), int(f[4])))
    return out


def main_table(table):
    """the main coverage table -> {sample: (unique, total)}, in its order"""
    out = {}
    for ln in table.split(b"\n")[1:]:
        if ln:
            f = ln.split(b"\t")
            out[f[5]] = (int(f[8]), int(f[9]))
    return out


def check_invariants(spectrum_table, coverage_table):
    """per sample of the main table: the bins with depth >= 1 sum to its unique column and the hits to its total column"""
    sp, mt = parse_table(spectrum_table), main_table(coverage_table)
    assert list(sp) == [s for s in mt if s in sp]                # (the main table's order)
    for s, (uq, tot) in mt.items():
        rows = sp.get(s, [])
        assert sum(n for d, n, _ in rows if d != b"0") == max(uq, 0), s
        assert sum(h for _, _, h in rows) == tot, s
        assert all(h == 0 for d, _, h in rows if d == b"0")
