"""The read pairs behind step 4's numbers (strain_detect --coverage-support / --support-pairs, sk_covacc_finish_target_support;
include/strainer_kmer.h has the rule) in Python: the model every support test compares against.  The reference has no counterpart;
the emission rule is restated here from its read loop, and the tests anchor it: the lines this model emits for a strain must be the
hit list a --coverage-depth run writes.

An emission is a tuple (target, pair, strain, L, parts, total, rows): pair = the pair's number in its target, L = lines printed,
parts = 1 (the PE1 part printed a line) | 2 (the PE2 part did), total = h1 + h2 of the lines, rows = the lines' bytes.

Strain(genome, informative)        a strain's keys (canonical 31-mers) and its informative subset
read_records(path)                 the sequences of a FASTA/FASTQ file, plain or .gz
walk(strain, s, t, mode, f1, f2)   the emissions of one strain over one target (SE, PE, PEI), short reads carried over
from_records(ns, sides, npairs)    the emissions of a folded run from the sparse records of its launches
InformativeOnly / join_totals      the same walk for genomes too large to hold here: emissions from the informative k-mers, totals from a hit list
tables(emissions, ...)             every number, given min_kmer_hits and a group size
support_file / pairs_file          the two files' bytes"""
import gzip
import os

import numpy as np

K = 31
SUPPORT_HEADER = b"metagenome\tsupporting_pairs\tboth_mates\tlines\n"
PAIRS_HEADER = b"metagenome\tstrain_a\tstrain_b\tpairs\tlines_a\n"
_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def canonical(w: bytes) -> bytes:
    return max(w, w.translate(_COMP)[::-1])


class Strain:
    def __init__(self, genome_records, informative):
        """genome_records: the strain file's sequences; informative: canonical 31-mers (those the strain does not hold count nowhere)"""
        self.keys = set()
        for g in genome_records:
            g = g.upper()
            for i in range(len(g) - K + 1):
                w = g[i:i + K]
                if set(w) <= set(b"ACGT"):
                    self.keys.add(canonical(w))
        self.inf = set(informative) & self.keys

    def tally(self, read):
        """(all hits, informative hits, the informative hits' k-mers in read order) of one read of k bases or more"""
        read = read.upper()
        h, rows = 0, []
        for i in range(len(read) - K + 1):
            w = canonical(read[i:i + K])
            if w in self.keys:
                h += 1
                if w in self.inf:
                    rows.append(w)
        return h, len(rows), rows


class InformativeOnly:
    """A strain known by its informative k-mers alone (no genome in memory): tally() counts informative hits only and reports them as
    the hits too.  An emission needs i1 + i2 >= 1, which implies h1 + h2 >= 1, so walk() finds the same emissions with the same lines'
    k-mers as with the whole key set; their totals are NOT the reference's and must come from elsewhere (join_totals)."""

    def __init__(self, informative):
        self.either = {}
        for c in informative:
            self.either[c] = c
            self.either[c.translate(_COMP)[::-1]] = c

    def tally(self, read):
        read, get = read.upper(), self.either.get
        rows = [c for c in (get(read[i:i + K]) for i in range(len(read) - K + 1)) if c is not None]
        return len(rows), len(rows), rows


def join_totals(emissions, hit_list):
    """the emissions of ONE strain over one or more targets, in file order, as walk() over an InformativeOnly strain gives them, with
    the totals of the hit list a --coverage-depth run wrote for that strain: the list's lines are cut into emissions by walking both
    in step -- the k-mers must agree line for line -- and each emission takes h1 + h2 of its lines"""
    lines = [ln.split(b"\t") for ln in hit_list.split(b"\n") if ln and not ln.startswith(b"#")]
    out, at = [], 0
    for t, j, s, L, parts, _, rows in emissions:
        mine = lines[at:at + L]
        assert len(mine) == L and [x[5] for x in mine] == [r.rstrip(b"\n").split(b"\t")[5] for r in rows], (t, j)
        assert len({tuple(x[:5]) for x in mine}) == 1
        out.append((t, j, s, L, parts, int(mine[0][1]) + int(mine[0][3]), rows))
        at += L
    assert at == len(lines), "the hit list holds lines the walk did not emit"
    return out


def _open(path):
    raw = open(path, "rb").read()
    return gzip.decompress(raw) if raw[:2] == b"\x1f\x8b" else raw


def read_records(path):
    """(sequences, 'fa' or 'fq'): FASTA records may span lines, FASTQ records are four lines"""
    lines = _open(path).split(b"\n")
    out, i = [], 0
    kind = "fq" if lines and lines[0][:1] == b"@" else "fa"
    while i < len(lines):
        ln = lines[i]
        if kind == "fq" and ln[:1] == b"@":
            out.append(lines[i + 1].rstrip(b"\r"))
            i += 4
        elif kind == "fa" and ln[:1] == b">":
            seq, i = [], i + 1
            while i < len(lines) and lines[i][:1] != b">":
                seq.append(lines[i].rstrip(b"\r"))
                i += 1
            out.append(b"".join(seq))
        else:
            i += 1
    return out, kind


def informative_list(path):
    """the k-mers a -a list names: lines of exactly 31 upper-case letters, '#' lines are comments"""
    return {canonical(ln) for ln in _open(path).split(b"\n") if len(ln) == K and not ln.startswith(b"#") and ln == ln.upper()}


def walk(strain, s, t, mode, f1, f2=None, name=None):
    """The reference's pair loop for one strain over one target.  A read of k bases or more refreshes its mate's tallies (and, for
    PE1, the copy of "the PE1 read last seen"); a shorter one refreshes nothing.  With h1 + h2 >= 1 and i1 + i2 >= 1 the copy's
    informative k-mers are printed, then, if THIS pair's PE2 read has k bases or more, that read's.  An odd PEI tail leaves the last
    read without a mate: a FASTA's reader then reports length 0 (no PE2 part), a FASTQ's the stale length -- the reference stops
    there when that is k or more, and so does this model."""
    name = os.fsencode(f1 if name is None else name)          # the lines' first column: the PE1 path as the target list has it
    r1, kind = read_records(f1)
    if mode == "PE":
        r2, _ = read_records(f2)
        assert len(r2) >= len(r1), "PE2 ended first: the reference stops"
        pairs = list(zip(r1, r2))
    elif mode == "PEI":
        pairs = [(r1[i], r1[i + 1] if i + 1 < len(r1) else None) for i in range(0, len(r1), 2)]
        if len(r1) % 2 and kind == "fq":
            assert len(r1[-1]) < K, "an odd FASTQ tail of k bases or more: the reference stops"
    else:
        pairs = [(r, None) for r in r1]
    h1 = i1 = h2 = i2 = 0
    copy, out = [], []
    for j, (a, b) in enumerate(pairs):
        if len(a) >= K:
            h1, i1, copy = strain.tally(a)
        brows = None
        if b is not None and len(b) >= K:
            h2, i2, brows = strain.tally(b)
        if h1 + h2 >= 1 and i1 + i2 >= 1:
            rows = list(copy) + list(brows or [])
            if rows:
                parts = (1 if copy else 0) | (2 if brows else 0)
                lines = [b"%s\t%d\t%d\t%d\t%d\t%s\n" % (name, h1, i1, h2, i2, w) for w in rows]
                out.append((t, j, s, len(rows), parts, h1 + h2, lines))
    return out


def from_records(t, ns, sides, npairs):
    """sides: (recs[n, 3] = {record * ns + member, all, informative}, r0, step) per mate, PE1's first: the emissions of a run in
    which every read has k bases or more (rows: None)"""
    tot = np.zeros((npairs, ns), dtype=np.int64)
    inf = np.zeros((2, npairs, ns), dtype=np.int64)
    for k, (recs, r0, step) in enumerate(sides):
        for key, al, nf in np.asarray(recs).tolist():
            rec, m = divmod(key, ns)
            if rec < r0 or (rec - r0) % step or (rec - r0) // step >= npairs:
                continue
            j = (rec - r0) // step
            tot[j, m] += al
            inf[k, j, m] += nf
    out = []
    for j, m in zip(*np.nonzero(inf.sum(axis=0))):
        parts = (1 if inf[0, j, m] else 0) | (2 if inf[1, j, m] else 0)
        out.append((t, int(j), int(m), int(inf[0, j, m] + inf[1, j, m]), parts, int(tot[j, m]), None))
    return out


class Tables:
    pass


def tables(emissions, ntargets, nstrains, min_kmer_hits, group=32):
    """pairs, lines, both [ntargets, nstrains]; shared, lines_a [ntargets, nstrains, nstrains] with the exclusive numbers on the
    diagonal and zeros between strains of different groups (group = consecutive strains that share a launch)"""
    T = Tables()
    T.pairs, T.lines, T.both = (np.zeros((ntargets, nstrains), dtype=np.uint64) for _ in range(3))
    T.shared, T.lines_a = (np.zeros((ntargets, nstrains, nstrains), dtype=np.uint64) for _ in range(2))
    at = {}
    for t, j, s, L, parts, total, _ in emissions:
        if not total > min_kmer_hits:
            continue
        T.pairs[t, s] += 1
        T.lines[t, s] += L
        T.both[t, s] += 1 if parts == 3 else 0
        at.setdefault((t, j, s // group), []).append((s, L))
    for (t, j, _), who in at.items():
        assert len({s for s, _ in who}) == len(who), "one emission per pair and strain"
        for a, L in who:
            if len(who) == 1:
                T.shared[t, a, a] += 1
                T.lines_a[t, a, a] += L
            for b, _ in who:
                if b != a:
                    T.shared[t, a, b] += 1
                    T.lines_a[t, a, b] += L
    return T


def samples(targets):
    """the targets' samples (basenames) in order of first appearance, and each target's sample"""
    names, of = [], []
    for f in targets:
        b = os.path.basename(f)
        if b not in names:
            names.append(b)
        of.append(names.index(b))
    return names, of


def _by_sample(arr, of, n):
    out = np.zeros((n,) + arr.shape[1:], dtype=np.uint64)
    for t, g in enumerate(of):
        out[g] += arr[t]
    return out


def support_file(T, targets, s):
    """strain s's .coverage_support: the samples in the order of the strain's main table -- those with an emission by the target that
    gave them their first, then the others by first appearance"""
    names, of = samples(targets)
    p, b, ln = (_by_sample(x, of, len(names))[:, s] for x in (T.pairs, T.both, T.lines))
    first = {}
    for t, g in enumerate(of):
        if T.pairs[t, s] and g not in first:
            first[g] = t
    order = sorted(first, key=first.get) + [g for g in range(len(names)) if g not in first]
    return SUPPORT_HEADER + b"".join(b"%s\t%d\t%d\t%d\n" % (names[g].encode(), p[g], b[g], ln[g]) for g in order)


def pairs_file(T, targets, strain_names, group=32):
    names, of = samples(targets)
    sh, la = _by_sample(T.shared, of, len(names)), _by_sample(T.lines_a, of, len(names))
    ns = len(strain_names)
    out = [b"#group\t%d\t%s\n" % (g, "\t".join(strain_names[g * group:(g + 1) * group]).encode()) for g in range((ns + group - 1) // group)]
    out.append(PAIRS_HEADER)
    for t, m in enumerate(names):
        for a in range(ns):
            for b in range(a // group * group, min(ns, (a // group + 1) * group)):
                if a == b or sh[t, a, b]:
                    out.append(b"%s\t%s\t%s\t%d\t%d\n" % (m.encode(), strain_names[a].encode(), strain_names[b].encode(), sh[t, a, b], la[t, a, b]))
    return b"".join(out)
