"""Thresholds (include/strainer_kmer.h has the rule) in Python: the model every thresholds test compares against.

numbers(rows, totals, t)   hits as (row or key, pair's total) -> (unique[len(t)], total[len(t)])
table_from_hits(text, ..)  the text of a hit list (strain_detect's -o file, decompressed) -> the table's bytes
parse_table / check_invariants   the table as a dictionary, and the rule's invariants against a main coverage table"""
import os

DEFAULT = (0, 1, 2, 3, 5, 10, 20, 50)
HEADER = b"strain_name\tmetagenome\tmin_kmer_hits\tunique_observed_informative_kmers\ttotal_observed_informative_kmers"


def numbers(keys, totals, thresholds):
    """one (key, total) per hit line -> per threshold t the distinct keys and the lines with total > t"""
    uq, tot = [], []
    for t in thresholds:
        passing = [k for k, h in zip(keys, totals) if int(h) > t]
        uq.append(len(set(passing)))
        tot.append(len(passing))
    return uq, tot


def strain_name(hits_file_name):
    n = os.path.basename(hits_file_name)
    return n[:-13] if len(n) >= 13 and n[-12:-3] == "kmer_hits" and n[-2:] == "gz" else n


def read_hits(text, min_hits=1):
    """-> (samples in the main table's order at min_hits, {sample: [(k-mer text, h1 + h2)]}) -- every hit line, unfiltered"""
    order, lines, evaluated = [], {}, []
    for line in text.split(b"\n"):
        if not line:
            continue
        if line.startswith(b"#"):
            f = line.rstrip().split(b"\t")
            s = os.path.basename(f[0][1:])
            if f[1] == b"total_kmer_evaluated" and s not in evaluated:
                evaluated.append(s)
            continue
        f = line.split(b"\t")
        s = os.path.basename(f[0])
        lines.setdefault(s, []).append((f[5], int(f[1]) + int(f[3])))
        if int(f[1]) + int(f[3]) > min_hits and s not in order:
            order.append(s)
    return order + [s for s in evaluated if s not in order], lines


def table_from_hits(text, hits_file_name, thresholds=DEFAULT, min_hits=1):
    name = strain_name(hits_file_name).encode()
    order, lines = read_hits(text, min_hits)
    out = [HEADER + b"\n"]
    for s in order:
        got = lines.get(s, [])
        uq, tot = numbers([k for k, _ in got], [h for _, h in got], thresholds)
        for t, u, n in zip(thresholds, uq, tot):
            out.append(b"%s\t%s\t%d\t%d\t%d\n" % (name, s, t, u, n))
    return b"".join(out)


def parse_table(table):
    """-> {sample: [(t, unique, total)]}, samples in the table's order"""
    rows = table.split(b"\n")
    assert rows[0] == HEADER and rows[-1] == b""
    out = {}
    for ln in rows[1:-1]:
        f = ln.split(b"\t")
        assert len(f) == 5
        out.setdefault(f[1], []).append((int(f[2]), int(f[3]), int(f[4])))
    return out


def main_table(table):
    """the main coverage table -> {sample: (unique, total)}, in its order"""
    out = {}
    for ln in table.split(b"\n")[1:]:
        if ln:
            f = ln.split(b"\t")
            out[f[5]] = (int(f[8]), int(f[9]))
    return out


def check_invariants(thr_table, coverage_table, thresholds, min_hits=None):
    """the samples and their order are the main table's; one line per threshold, ascending; neither number grows with t;
    unique <= total; the line of the run's own min_hits, if listed, carries the main table's two numbers"""
    th, mt = parse_table(thr_table), main_table(coverage_table)
    assert list(th) == list(mt)
    for s, rows in th.items():
        assert [t for t, _, _ in rows] == list(thresholds), s
        for (_, u0, n0), (_, u1, n1) in zip(rows, rows[1:]):
            assert u1 <= u0 and n1 <= n0, s
        assert all(u <= n for _, u, n in rows), s
        for t, u, n in rows:
            if min_hits is not None and t == min_hits:
                assert (u, n) == (max(mt[s][0], 0), mt[s][1]), s
