"""Worlds for the union item fold (sk_union_item_fold; include/strainer_kmer.h): unions of members that SHARE keys, items of reads,
and what every member ALONE sees of every item -- the CPU oracle's table of that member, scanned item by item.  That is what a
member's columns and records must equal after the union's folds.  No device, no library under test: the GPU tests load these
strains, and tests/test_prevalence_multi_host.py checks the premises (shared keys, boundaries, sizes, counts that min_count 2
separates) on the CPU.
TEST INFRASTRUCTURE: ground truth is the oracle run member by member and item by item, never the code under test."""
import gzip
import random

import numpy as np

import _oracle
import _synth

K = 31
SIZES = (4095, 4096, 4097, 8193)                            # total global rows around the fold's 4096 entries per workgroup
ROWS_A, ROWS_C = 1000, 700                                  # (1000, 2000, 2700, 2701: no multiple of 64 or 256)


def _mutate_middle(rng, seq):
    """seq with one base in 40 of its middle third changed"""
    b = bytearray(seq)
    for i in range(len(b) // 3, 2 * len(b) // 3):
        if rng.random() < 0.025:
            b[i] = rng.choice([c for c in b"ACGT" if c != b[i]])
    return bytes(b)


def related(total):
    """five members with `total` rows in all: A, B = A with its middle mutated, C = a reverse-complemented stretch of A and
    bases of its own, E = one window (1 row), D unrelated"""
    rng = random.Random(77000 + total)
    a = _synth.rand_dna(rng, ROWS_A + K - 1)
    b = _mutate_middle(rng, a)
    c = _synth.revcomp(a[200:600]) + _synth.rand_dna(rng, ROWS_C + K - 1 - 400)
    e = _synth.rand_dna(rng, K)
    d = _synth.rand_dna(rng, total - 2 * ROWS_A - ROWS_C - 1 + K - 1)
    return [a, b, c, e, d]


def single():
    return [_synth.rand_dna(random.Random(77001), 600)]


def panel32():
    """32 members of about 40 bases (about 10 rows each): members 1, 5, 9 .. are their neighbour with one base changed near the end,
    members 3, 7, 11 .. hold their neighbour's other strand"""
    rng = random.Random(77032)
    out = []
    for s in range(32):
        if s % 2 == 0:
            out.append(_synth.rand_dna(rng, rng.randint(38, 43)))
        elif s % 4 == 1:
            g = bytearray(out[-1])                          # (the last base but one: all windows but the last two are shared)
            g[-2] = ord("A") if g[-2] != ord("A") else ord("C")
            out.append(bytes(g))
        else:
            out.append(_synth.revcomp(out[-1])[:36] + _synth.rand_dna(rng, 5))
    return out


def reads(rng, strains, n, max_len=120):
    """records of the members (either strand, whole now and then), some with an N or an IUPAC letter inside, noise, and records
    shorter than k"""
    out = []
    for i in range(n):
        strain = strains[rng.randrange(len(strains))]
        x = rng.random()
        if len(strain) <= 64:
            r = strain if x < 0.5 else _synth.revcomp(strain) if x < 0.8 else _synth.rand_dna(rng, K)
        elif x < 0.75:
            ln = rng.randint(K, min(max_len, len(strain)))
            at = rng.randrange(0, len(strain) - ln + 1)
            r = strain[at:at + ln]
            if i % 2:
                r = _synth.revcomp(r)
        elif x < 0.9:
            r = _synth.rand_dna(rng, rng.randint(1, max_len))
        else:
            r = strain[:20]
        if i % 11 == 5 and len(r) > 70:                     # the windows on either side still count
            r = r[:35] + (b"N" if i % 2 else b"R") + r[36:]
        out.append(r)
    return b"\n".join(out) + b"\n"


class World:
    """strains; items a and b of two chunks each; per member the oracle's keys and the columns va, vb (item a, item b) and va1 (item
    a's first chunk alone)"""

    def __init__(self, strains, seed, nreads):
        self.strains = strains
        rng = random.Random(seed)
        self.chunks_a = [reads(rng, strains, nreads) for _ in range(2)]
        self.chunks_b = [reads(rng, strains, nreads) for _ in range(2)]
        self.keys, self.va, self.vb, self.va1 = [], [], [], []
        for s in strains:
            t = _oracle.OracleTable(ncols=4)
            assert t.build_stream(s + b"\n") == 0
            for col, chunks in ((1, self.chunks_a), (2, self.chunks_b), (3, self.chunks_a[:1])):
                for ch in chunks:
                    t.scan_stream(ch, col)
            keys, c = t.rows()
            t.close()
            self.keys.append(keys)
            self.va.append(c[:, 1].astype(np.uint32))
            self.vb.append(c[:, 2].astype(np.uint32))
            self.va1.append(c[:, 3].astype(np.uint32))
        self.rows = [len(k) for k in self.keys]
        self.base = [int(x) for x in np.concatenate([[0], np.cumsum(self.rows)])]      # base[s] .. base[members] = all rows

    def shared(self, i, j):
        """distinct keys members i and j both hold"""
        return len(set(self.keys[i]) & set(self.keys[j]))


# ---- the program's panels (kmer_scrub_count -S): files in a directory
def _mutate(rng, seq, rate):
    b = bytearray(seq)
    for i in range(len(b)):
        if rng.random() < rate:
            b[i] = rng.choice(b"ACGT")
    return bytes(b)


def _fa(path, recs, gz=False):
    body = b"".join(b">r%d\n%s\n" % (i, r) for i, r in enumerate(recs))
    with (gzip.open if gz else open)(path, "wb") as f:
        f.write(body)


def _fq(path, recs):
    with open(path, "wb") as f:
        f.write(b"".join(b"@r%d\n%s\n+\n%s\n" % (i, r, b"I" * len(r)) for i, r in enumerate(recs)))


def _some_reads(rng, seqs, n):
    return [r for r in reads(rng, seqs, n, 100).split(b"\n")[:-1] if r]


def panel(d, seed, nstrains):
    """siblings (strain 1 is strain 0 mutated) and unrelated strains; -A of 5 items, one of them a sibling's genome; -B of 3, one
    .gz; -C names strain 0's genome twice, strain 1's once, and one other file; targets for step 3"""
    rng = random.Random(seed)
    s0 = _synth.rand_dna(rng, 3000)
    seqs = [s0, _mutate(rng, s0, 0.01), _synth.rand_dna(rng, 2500), _synth.revcomp(s0[500:1500]) + _synth.rand_dna(rng, 1200),
            _synth.rand_dna(rng, 900)][:nstrains]
    if nstrains > 4:
        seqs[4] = _mutate(rng, seqs[2], 0.02)
    genomes = []
    for s, g in enumerate(seqs):
        (d / f"s{s}.fa").write_bytes(b">s%d\n" % s + g[:len(g) // 2] + b"\n" + g[len(g) // 2:] + b"\n")
        genomes.append(f"s{s}.fa")
    _fa(d / "a0.fa", [_synth.rand_dna(rng, 300) + s0[200:1400], seqs[2][100:900]])
    _fa(d / "a2.fa", [s0[1200:2600] + _synth.rand_dna(rng, 200)])
    _fq(d / "a3.fq", _some_reads(rng, seqs, 150))
    _fa(d / "a4.fa", [seqs[1][:1000], _synth.revcomp(seqs[2][800:2000])])
    (d / "A.txt").write_text("a0.fa\ns1.fa\na2.fa\na3.fq\na4.fa\n")
    _fq(d / "m0.fq", _some_reads(rng, seqs, 300) + [s0[1000:1100]] * 40)
    _fa(d / "m1.fa.gz", _some_reads(rng, seqs, 200), gz=True)
    _fa(d / "m2.fa", _some_reads(rng, seqs[:1], 120))
    (d / "B.txt").write_text("m0.fq\nm1.fa.gz\nm2.fa\n")
    _fa(d / "d0.fa", [s0[2500:2900], seqs[2][:300]])
    (d / "C.txt").write_text("s0.fa\nd0.fa\ns1.fa\ns0.fa\n")
    _fa(d / "t.fa", _some_reads(rng, seqs, 300))
    (d / "T.txt").write_text("SE\tt.fa\n")
    return genomes


_made = {}


def world(name):
    """'4095' .. '8193', 'single', 'panel32': made once per process"""
    if name not in _made:
        if name == "single":
            _made[name] = World(single(), 1, 40)
        elif name == "panel32":
            _made[name] = World(panel32(), 32, 80)
        else:
            _made[name] = World(related(int(name)), int(name), 120)
    return _made[name]


NAMES = [str(n) for n in SIZES] + ["single", "panel32"]
