"""Support (strain_detect --coverage-support / --support-pairs; include/strainer_kmer.h has the rule) without a device: the ABI surface,
the model (tests/_support_model.py) on hand-made inputs whose numbers are worked out below, the host side of the feature
(strainer2_amd/csrc/sk_host_support.c) driven by tests/native/support_check.c under AddressSanitizer + UBSan against the model's two
files, and the command lines the flags refuse before anything is opened.

The hand-made world: two strains g0 = U0 + C and g1 = U1 + C, U0 / U1 / C random and 120 / 120 / 60 bases long.  Informative in
strain 0: the 31-mers at U0[10] and at C[0]; in strain 1: those at U1[5] and at C[0]."""
import os
import random
import re
import subprocess

import pytest

import _support_model as sm
import _synth
import strainer2_amd as sk
from strainer2_amd import native

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = sk.cli_path("strain_detect")
SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined", "-pthread"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")


class Hand:
    pass


@pytest.fixture(scope="module")
def hand():
    rng = random.Random(5150)
    h = Hand()
    h.U0, h.U1, h.C = _synth.rand_dna(rng, 120), _synth.rand_dna(rng, 120), _synth.rand_dna(rng, 60)
    h.junk = [_synth.rand_dna(rng, 40) for _ in range(4)]
    h.strains = [sm.Strain([h.U0 + h.C], {sm.canonical(h.U0[10:41]), sm.canonical(h.C[0:31])}),
                 sm.Strain([h.U1 + h.C], {sm.canonical(h.U1[5:36]), sm.canonical(h.C[0:31])})]
    assert len(h.strains[0].keys) == 150 and len(h.strains[0].inf) == 2 and len(h.strains[0].keys & h.strains[1].keys) == 30
    return h


def _fa(reads):
    return b"".join(b">r%d\n%s\n" % (i, x) for i, x in enumerate(reads))


def _fq(reads):
    return b"".join(b"@r%d\n%s\n+\n%s\n" % (i, x, b"I" * len(x)) for i, x in enumerate(reads))


def _walk(h, d, mode, files):
    paths = []
    for i, data in enumerate(files):
        paths.append(str(d / ("t%d.%s" % (i, "fq" if data[:1] == b"@" else "fa"))))
        open(paths[-1], "wb").write(data)
    em = []
    for s, st in enumerate(h.strains):
        em += sm.walk(st, s, 0, mode, *paths)
    return em, paths


def test_new_entry_points_and_the_formats_are_declared(repo):
    hdr = open(os.path.join(repo, "include", "strainer_kmer.h")).read()
    syms = subprocess.run(["nm", "-D", "--defined-only", sk.library_path()], capture_output=True, text=True).stdout
    for name in ("sk_covacc_set_support", "sk_covacc_finish_target_support"):
        assert re.search(r"\b%s\(" % name, hdr), name
        assert name in native.ABI_SYMBOLS, name
        assert re.search(r"\bT %s$" % name, syms, re.M), name
    assert re.search(r"\bT sk_covacc_support_timing_$", syms, re.M)
    assert "#define SK_COVACC_SUPPORT_MEMBERS_MAX 1024u" in hdr and native.SK_COVACC_SUPPORT_MEMBERS_MAX == 1024
    assert sm.SUPPORT_HEADER.decode().rstrip("\n").replace("\t", "<TAB>") in hdr
    assert sm.PAIRS_HEADER.decode().rstrip("\n").replace("\t", "<TAB>") in hdr
    for m in ("set_support", "finish_target_support", "support_timing"):
        assert hasattr(sk.CoverageAcc, m), m


def test_one_pair_supports_two_strains(hand, tmp_path):
    """SE, one read C[0:40]: ten 31-mers, all keys of both strains, the first informative in both.  Each strain has one emission at
    pair 0 with L = 1 and total 10: supporting_pairs 1, lines 1, both_mates 0; shared_pairs(0, 1) = 1 with lines_a = 1 both ways, and
    neither strain has an exclusive pair.  With the two strains in groups of one, each pair is exclusive."""
    h = hand
    em, paths = _walk(h, tmp_path, "SE", [_fa([h.C[0:40]])])
    assert [(j, s, L, parts, tot) for _, j, s, L, parts, tot, _ in em] == [(0, 0, 1, 1, 10), (0, 1, 1, 1, 10)]
    assert em[0][6] == [b"%s\t10\t1\t0\t0\t%s\n" % (paths[0].encode(), sm.canonical(h.C[0:31]))]
    T = sm.tables(em, 1, 2, 1)
    assert T.pairs.tolist() == [[1, 1]] and T.lines.tolist() == [[1, 1]] and T.both.tolist() == [[0, 0]]
    assert T.shared[0].tolist() == [[0, 1], [1, 0]] and T.lines_a[0].tolist() == [[0, 1], [1, 0]]
    assert sm.tables(em, 1, 2, 1, group=1).shared[0].tolist() == [[1, 0], [0, 1]]
    assert sm.support_file(T, paths[:1], 0) == sm.SUPPORT_HEADER + b"t0.fa\t1\t0\t1\n"
    assert sm.pairs_file(T, paths[:1], ["a", "b"]) == (b"#group\t0\ta\tb\n" + sm.PAIRS_HEADER + b"t0.fa\ta\ta\t0\t0\nt0.fa\ta\tb\t1\t1\n"
                                                        b"t0.fa\tb\ta\t1\t1\nt0.fa\tb\tb\t0\t0\n")
    assert sm.pairs_file(sm.tables(em, 1, 2, 1, group=1), paths[:1], ["a", "b"], group=1) == (
        b"#group\t0\ta\n#group\t1\tb\n" + sm.PAIRS_HEADER + b"t0.fa\ta\ta\t1\t1\nt0.fa\tb\tb\t1\t1\n")


def test_a_pair_that_passes_only_on_the_sum_and_one_that_does_not_pass(hand, tmp_path):
    """PE.  Pair 0: PE1 = U0[10:43] (three 31-mers, the first informative), PE2 = U0[50:83] (three, none informative): h1 = h2 = 3.
    At min_kmer_hits 4 neither mate passes alone and 3 + 3 = 6 does: one emission, L = 1, through PE1 only.  Pair 1: PE1 = U0[10:42]
    (two 31-mers, one informative), PE2 random: an informative hit and a total of 2 -- an emission at min 0 and 1, none at min 4.
    Strain 1 holds none of these k-mers."""
    h = hand
    em, _ = _walk(h, tmp_path, "PE", [_fa([h.U0[10:43], h.U0[10:42]]), _fa([h.U0[50:83], h.junk[0]])])
    assert [(j, s, L, parts, tot) for _, j, s, L, parts, tot, _ in em] == [(0, 0, 1, 1, 6), (1, 0, 1, 1, 2)]
    for mh, want in ((0, 2), (1, 2), (2, 1), (4, 1), (5, 1), (6, 0)):
        T = sm.tables(em, 1, 2, mh)
        assert T.pairs.tolist() == [[want, 0]] and T.lines.tolist() == [[want, 0]] and T.shared[0, 0, 0] == want, mh


def test_both_mates(hand, tmp_path):
    """PEI, one pair: PE1 = C[0:35] (five 31-mers, one informative), PE2 = the other strand of U0[5:45] (ten, one informative, a key
    of strain 0 only).  Strain 0: h 5 + 10, L = 2, both mates.  Strain 1: PE1 alone (h 5 + 0), L = 1."""
    h = hand
    em, _ = _walk(h, tmp_path, "PEI", [_fq([h.C[0:35], _synth.revcomp(h.U0[5:45])])])
    assert [(j, s, L, parts, tot) for _, j, s, L, parts, tot, _ in em] == [(0, 0, 2, 3, 15), (0, 1, 1, 1, 5)]
    T = sm.tables(em, 1, 2, 1)
    assert T.both.tolist() == [[1, 0]] and T.lines_a[0].tolist() == [[0, 2], [1, 0]]


def test_a_short_read_emits_again(hand, tmp_path):
    """SE: U0[10:50] (ten 31-mers, one informative), then a read of 20 bases, then a random one.  The short read refreshes nothing: the
    tallies (10, 1) and the copy of the read before it are still there, and its pass prints that read's line again -- two emissions,
    two lines, as step 4's total has it.  The random read has k bases: it resets the tallies, and nothing is printed."""
    h = hand
    em, paths = _walk(h, tmp_path, "SE", [_fa([h.U0[10:50], b"ACGT" * 5, h.junk[1]])])
    assert [(j, s, L, parts, tot) for _, j, s, L, parts, tot, _ in em] == [(0, 0, 1, 1, 10), (1, 0, 1, 1, 10)]
    assert em[0][6] == em[1][6]
    T = sm.tables(em, 1, 2, 1)
    assert T.pairs.tolist() == [[2, 0]] and T.lines.tolist() == [[2, 0]]


def test_an_odd_interleaved_tail(hand, tmp_path):
    """PEI with three reads, FASTA: pair 0 = (U0[10:50], random), pair 1 = (U0[0:45], nothing): the reader reports length 0 for the
    missing mate, so the last read is a pair of its own through PE1 -- fifteen 31-mers, one informative.  FASTQ with a short last
    read: PE1 refreshes nothing and emits pair 0's line again; with a last read of k bases or more the reference stops, and so does
    the model."""
    h = hand
    em, _ = _walk(h, tmp_path, "PEI", [_fa([h.U0[10:50], h.junk[2], h.U0[0:45]])])
    assert [(j, s, L, parts, tot) for _, j, s, L, parts, tot, _ in em] == [(0, 0, 1, 1, 10), (1, 0, 1, 1, 15)]
    em, _ = _walk(h, tmp_path, "PEI", [_fq([h.U0[10:50], h.junk[2], b"ACGTACGT"])])
    assert [(j, s, L, parts, tot) for _, j, s, L, parts, tot, _ in em] == [(0, 0, 1, 1, 10), (1, 0, 1, 1, 10)]
    with pytest.raises(AssertionError):
        _walk(h, tmp_path, "PEI", [_fq([h.U0[10:50], h.junk[2], h.U0[0:45]])])


def test_samples_and_their_order(hand, tmp_path):
    """two targets with one basename are one sample; a strain's table lists the samples with an emission by the target that gave
    them their first, then the others"""
    T = sm.tables([(1, 0, 0, 2, 1, 9, None), (2, 0, 0, 1, 1, 9, None), (2, 3, 0, 4, 3, 9, None), (0, 0, 1, 1, 1, 9, None)], 4, 2, 1)
    targets = ["x/a.fa", "b.fa", "y/a.fa", "c.fa"]
    assert sm.support_file(T, targets, 0) == sm.SUPPORT_HEADER + b"b.fa\t1\t0\t2\na.fa\t2\t1\t5\nc.fa\t0\t0\t0\n"
    assert sm.support_file(T, targets, 1) == sm.SUPPORT_HEADER + b"a.fa\t1\t0\t1\nb.fa\t0\t0\t0\nc.fa\t0\t0\t0\n"


# ---------------------------------------------------------------------------------------------------------------------------------
# the host side under the sanitizers
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("sup") / "support_check")
    subprocess.run(["gcc"] + SAN + [os.path.join(REPO, "tests", "native", "support_check.c"), "-o", exe], check=True)
    return exe


@pytest.mark.parametrize("ns,group,seed", [(1, 1, 1), (3, 32, 2), (7, 2, 3), (37, 32, 4), (64, 32, 5), (5, 1, 6)])
def test_merge_and_formatters_against_the_model(checker, tmp_path, ns, group, seed):
    """random runs: emission lists per strain merged run by run, one group's numbers handed in as the device's, targets without an
    emission, two targets with one basename, strains and whole groups without any emission, pairs that support all 32 of a group"""
    rng = random.Random(seed)
    names = ["Genus_species_s%d" % s for s in range(ns)]
    targets = ["d0/m0.fq", "m1.fa", "d1/m0.fq", "empty.fa", "m2.fq.gz"]
    quiet = set(range(group, min(ns, 2 * group))) if ns > group and seed % 2 else {ns - 1} if ns > 2 else set()
    script, em = ["N %d %d" % (ns, group)] + ["S " + n for n in names], []
    for t, path in enumerate(targets):
        script.append("T " + path)
        if path == "empty.fa":
            continue
        for run in range(3):
            script.append("R")
            for j in sorted(rng.sample(range(200), 25)):
                kind = rng.random()
                who = list(range(ns)) if kind < 0.1 else rng.sample(range(ns), min(ns, rng.choice([1, 1, 2, 3])))
                for s in sorted(set(who) - quiet):
                    L, parts = rng.randrange(1, 60), rng.choice([1, 2, 3])
                    script.append("E %d %d %d %d" % (s, j, L, parts))
                    em.append((t, run * 1000 + j, s, L, parts, 5, None))
            script.append("M")
        # a run the device counted: the model's own numbers of one group's strains, handed in as the device returns them
        g0 = rng.randrange((ns + group - 1) // group) * group
        n = min(group, ns - g0)
        dev = [(t, 900000 + j, g0 + m, rng.randrange(1, 9), rng.choice([1, 3]), 5, None)
               for j in range(12) for m in rng.sample(range(n), min(n, rng.choice([1, 2])))]
        dev = [e for e in dev if e[2] not in quiet]
        em += dev
        D = sm.tables([(0, j, s - g0, L, p, tot, None) for _, j, s, L, p, tot, _ in dev], 1, n, 1, group=n)
        script.append("D %d %d %s" % (g0, n, " ".join(str(int(x)) for a in (D.pairs[0], D.lines[0], D.both[0], D.shared[0].ravel(), D.lines_a[0].ravel())
                                                   for x in a)))
    (tmp_path / "script").write_text("\n".join(script) + "\n")
    p = subprocess.run([checker, str(tmp_path / "script"), str(tmp_path / "sup"), str(tmp_path / "pairs")], env=ENV, capture_output=True)
    assert b"runtime error" not in p.stderr and b"AddressSanitizer" not in p.stderr and b"LeakSanitizer" not in p.stderr, p.stderr.decode()[-2000:]
    assert p.returncode == 0, p.stderr.decode()[-1000:]
    T = sm.tables(em, len(targets), ns, 1, group=group)
    want = b"".join(b"== %s\n" % n.encode() + sm.support_file(T, targets, s) for s, n in enumerate(names))
    assert (tmp_path / "sup").read_bytes() == want
    assert (tmp_path / "pairs").read_bytes() == sm.pairs_file(T, targets, names, group=group)
    if ns >= 32:
        assert T.shared[0, 0, 31] > 0 and T.shared[:, 0, 0].sum() > 0
    for s in quiet:
        assert not T.pairs[:, s].any()


# ---------------------------------------------------------------------------------------------------------------------------------
# refusals: one line on stderr, a non-zero status, nothing written.  (--support-pairs with strains no union table can hold is refused
# only once the strains are on the device: tests/test_coverage_support_gpu.py has that one.)
# ---------------------------------------------------------------------------------------------------------------------------------
def _job(d):
    (d / "g.fa").write_bytes(b">g\n" + b"ACGTTGCAAGGCTTAACCGGTTAACCGTAGCTAGCTAGGCTA" * 20 + b"\n")
    (d / "inf.txt").write_bytes(b"#informative\nACGTTGCAAGGCTTAACCGGTTAACCGTAGC\n")
    (d / "T.txt").write_text("SE\tg.fa\n")
    (d / "S.txt").write_text("g.fa\tinf.txt\tGenus_species_a.kmer_hits.gz\ng.fa\tinf.txt\tGenus_species_b.kmer_hits.gz\n")
    return sorted(os.listdir(d))


ONE = ["-r", "g.fa", "-a", "inf.txt", "-B", "T.txt", "-o", "Genus_species_a.kmer_hits.gz"]
MANY = ["-S", "S.txt", "-B", "T.txt"]
REFUSALS = [
    ("alone", ONE + ["--coverage-support"], {}, b"--coverage-support goes with --coverage-depth or --coverage-only"),
    ("alone_file", ONE + ["--coverage-support=x.tsv"], {}, b"--coverage-support goes with --coverage-depth or --coverage-only"),
    ("pairs_alone", MANY + ["--coverage-only", "--support-pairs=p.tsv"], {}, b"--support-pairs goes with --coverage-support"),
    ("pairs_no_name", MANY + ["--coverage-only", "--coverage-support", "--support-pairs"], {}, b"--support-pairs=FILE needs a file name"),
    ("pairs_no_S", ONE + ["--coverage-only", "--coverage-support", "--support-pairs=p.tsv"], {}, b"--support-pairs goes with -S"),
    ("pairs_world", MANY + ["--coverage-depth", "--coverage-support", "--support-pairs=p.tsv"], {"WORLD_SIZE": "2"}, b"--support-pairs is for ONE process"),
    ("pairs_no_union", MANY + ["--coverage-only", "--coverage-support", "--support-pairs=p.tsv"], {"SK_SD_NO_UNION": "1"}, b"SK_SD_NO_UNION is set"),
    ("file_many", MANY + ["--coverage-only", "--coverage-support=x.tsv"], {}, b"--coverage-support=FILE names one file"),
]


@pytest.mark.parametrize("case", REFUSALS, ids=lambda c: c[0])
def test_refusals(tmp_path, case):
    _, argv, env, words = case
    before = _job(tmp_path)
    clean = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "SK_WORLD_SIZE", "SK_SD_NO_UNION", "RANK")}
    p = subprocess.run([EXE] + argv, cwd=tmp_path, capture_output=True, timeout=120, env=dict(clean, **env))
    assert p.returncode != 0 and p.stdout == b""
    assert p.stderr.count(b"\n") == 1 and p.stderr.endswith(b"\n") and words in p.stderr, p.stderr
    assert sorted(os.listdir(tmp_path)) == before
