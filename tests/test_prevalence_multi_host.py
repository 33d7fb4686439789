"""Prevalence for many strains from one pass, the parts that need no device: the premises of the worlds the GPU tests fold
(tests/_prevalence_multi_worlds.py), checked with the oracle on the CPU; kmer_scrub_count -S's refusals of the prevalence words, each
one line, status 1, nothing created, before a genome that does not exist is noticed; and the ABI."""
import os
import re
import subprocess

import numpy as np
import pytest

import _prevalence_multi_worlds as worlds
import strainer2_amd as sk
from strainer2_amd import native

EXE = sk.cli_path()
NEW = ["sk_union_item_fold", "skh_scan_list_many_prevalence"]


# ---------------------------------------------------------------------------------------------------------- the worlds' premises
@pytest.mark.parametrize("total", worlds.SIZES)
def test_related_members_share_keys_and_straddle_the_tiles(total):
    w = worlds.world(str(total))
    assert w.base[-1] == total and len(w.strains) == 5      # the difference array has total + 1 live entries around 4096 per workgroup
    assert w.rows[3] == 1, "one member has exactly one row"
    for b in w.base[1:-1]:
        assert b % 64 and b % 256, "a wave and a workgroup straddle two members"
    # B is A with its middle mutated, C holds a reverse-complemented stretch of A: shared keys, in number; D shares nothing
    assert 500 <= w.shared(0, 1) < w.rows[0]
    assert 300 <= w.shared(0, 2) < w.rows[2]
    assert w.shared(0, 4) == 0 and w.shared(1, 4) == 0
    for v in (w.va, w.vb):
        allv = np.concatenate(v)
        assert (allv >= 2).any() and (allv == 1).any() and (allv == 0).any(), "min_count 2 separates the rows"
        for s in (0, 1, 2, 4):
            assert int(v[s].sum()) > 0, "every member but the one-row one is hit by both items"
    # a shared key is counted alike in every member that holds it: the union may credit any of their rows
    for i, j in ((0, 1), (0, 2)):
        at_j = dict(zip(w.keys[j], w.va[j]))
        both = [(x, at_j[k]) for k, x in zip(w.keys[i], w.va[i]) if k in at_j]
        assert both and all(x == y for x, y in both)
        assert any(x > 0 for x, _ in both), "the items hit shared keys"


def test_the_reads_reach_both_sinks():
    """an N and an IUPAC letter inside records (the latter goes to the byte-string kernel, which adds to the scratch column
    directly), records shorter than k, both strands"""
    w = worlds.world("4096")
    recs = b"".join(w.chunks_a + w.chunks_b).split(b"\n")
    assert any(b"N" in r for r in recs) and any(b"R" in r for r in recs)
    assert any(0 < len(r) < worlds.K for r in recs)
    a = w.strains[0]
    fwd = sum(1 for r in recs if len(r) >= worlds.K and r in a)
    rev = sum(1 for r in recs if len(r) >= worlds.K and worlds._synth.revcomp(r) in a and r not in a)
    assert fwd > 5 and rev > 5


def test_the_panel_of_32_and_the_single_member():
    w = worlds.world("panel32")
    assert len(w.strains) == 32 and all(36 <= len(s) <= 48 for s in w.strains)
    assert sum(w.shared(s, s + 1) > 0 for s in range(0, 32, 2)) >= 12, "neighbours share keys"
    assert int(w.va[31].sum()) > 0 and int(w.vb[31].sum()) > 0, "bit 31 of the mask has something to fold"
    assert len(worlds.world("single").strains) == 1


# ---------------------------------------------------------------------------------------------------------- the ABI
def test_new_entry_points_are_declared_listed_and_exported(repo):
    hdr = open(os.path.join(repo, "include", "strainer_kmer.h")).read()
    syms = subprocess.run(["nm", "-D", "--defined-only", sk.library_path()], capture_output=True, text=True).stdout
    for name in NEW:
        assert re.search(r"\b%s\(" % name, hdr), name
        assert name in native.ABI_SYMBOLS, name
        assert re.search(r"\bT %s$" % name, syms, re.M), name
    for m in ("item_slots", "item_slot", "item_fold"):
        assert hasattr(sk.KmerUnion, m), m


# ---------------------------------------------------------------------------------------------------------- the refusals
def _job(d):
    (d / "A.txt").write_text("a.fa\n")
    (d / "B.txt").write_text("b.fa\n")
    (d / "S.txt").write_text("missing1.fa\tx\nmissing2.fa\ty\n")              # (no genome exists: a refusal comes before that is noticed)
    (d / "SD.txt").write_text("missing1.fa\tx.inf\tx.kmer_hits.gz\nmissing2.fa\ty.inf\ty.kmer_hits.gz\n")


BASE = ["-S", "S.txt", "-A", "A.txt", "-B", "B.txt"]
DETECT = ["-S", "SD.txt", "-A", "A.txt", "-B", "B.txt"]
TAIL = ["--detect", "-B", "T.txt"]
REFUSED = {
    "bare --prevalence": (BASE + ["--prevalence"], b"--prevalence does not go with -S"),
    "empty suffix": (BASE + ["--prevalence="], b"--prevalence does not go with -S"),
    "bare --prevalence-items": (BASE + ["--prevalence=.p", "--prevalence-items"], b"--prevalence-items=SUFFIX"),
    "empty items suffix": (BASE + ["--prevalence=.p", "--prevalence-items="], b"--prevalence-items=SUFFIX"),
    "items without the table": (BASE + ["--prevalence-items=.i"], b"need --prevalence=SUFFIX"),
    "min-count without the table": (BASE + ["--prevalence-min-count", "2"], b"need --prevalence=SUFFIX"),
    "scrub-by prevalence without the table": (DETECT + ["--scrub", "0.05", "--scrub-by", "prevalence"] + TAIL, b"--scrub-by prevalence needs --prevalence=SUFFIX"),
    "scrub-by without --scrub": (BASE + ["--prevalence=.p", "--scrub-by", "prevalence"], b"--scrub-by needs --scrub"),
    "scrub-by count without --scrub": (BASE + ["--scrub-by=count"], b"--scrub-by needs --scrub"),
    "scrub-by something else": (DETECT + ["--prevalence=.p", "--scrub", "0.05", "--scrub-by", "depth"] + TAIL, b"--scrub-by takes count or prevalence"),
    "the sweep by prevalence": (DETECT + ["--prevalence=.p", "--scrub", "0.1,0.05", "--scrub-by", "prevalence"] + TAIL + ["--coverage-only", "--coverage-scrub-sweep"],
                                b"--scrub-by prevalence does not go with a list of fractions"),
    "count 0": (BASE + ["--prevalence=.p", "--prevalence-min-count", "0"], b"--prevalence-min-count needs an integer of at least 1"),
    "count -1": (BASE + ["--prevalence=.p", "--prevalence-min-count=-1"], b"--prevalence-min-count needs an integer of at least 1"),
    "count 1.5": (BASE + ["--prevalence=.p", "--prevalence-min-count", "1.5"], b"--prevalence-min-count needs an integer of at least 1"),
    "count empty": (BASE + ["--prevalence=.p", "--prevalence-min-count="], b"--prevalence-min-count needs an integer of at least 1"),
    "the two suffixes alike": (BASE + ["--prevalence=.p", "--prevalence-items=.p"], b"would be the one file x.p"),
}


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_refused_with_one_line_and_nothing_created(tmp_path, name):
    argv, said = REFUSED[name]
    _job(tmp_path)
    before = sorted(os.listdir(tmp_path))
    p = subprocess.run([EXE] + argv, cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert p.returncode == 1 and p.stdout == b""
    assert said in p.stderr and p.stderr.count(b"\n") == 1 and p.stderr.endswith(b"\n"), p.stderr
    assert b"missing" not in p.stderr
    assert sorted(os.listdir(tmp_path)) == before


def test_names_that_coincide_behind_the_suffix_are_refused(tmp_path):
    """outfiles x and x.p with the suffix .p; an outfile that is another strain's item records; the progress file"""
    _job(tmp_path)
    for strains, extra, name in (("missing1.fa\tx\nmissing2.fa\tx.p\n", ["--prevalence=.p"], b"x.p"),
                                 ("missing1.fa\tx\nmissing2.fa\tx.i\n", ["--prevalence=.p", "--prevalence-items=.i"], b"x.i"),
                                 ("missing1.fa\tx\nmissing2.fa\ty\n", ["--prevalence=.p", "-p", "y.p"], b"y.p")):
        (tmp_path / "S.txt").write_text(strains)
        before = sorted(os.listdir(tmp_path))
        p = subprocess.run([EXE] + BASE + extra, cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
        assert p.returncode == 1 and p.stdout == b""
        assert b"would be the one file " + name in p.stderr and p.stderr.count(b"\n") == 1, p.stderr
        assert b"missing" not in p.stderr
        assert sorted(os.listdir(tmp_path)) == before


def test_the_bare_flags_refusal_says_what_to_give(tmp_path):
    _job(tmp_path)
    p = subprocess.run([EXE] + BASE + ["--prevalence"], cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert b"one file name cannot serve many strains" in p.stderr and b"--prevalence=SUFFIX" in p.stderr


# ---------------------------------------------------------------------------------------------------------- the program's panel
@pytest.mark.parametrize("nstrains", [3, 5])
def test_the_drug_list_really_names_two_different_strains_genomes(tmp_path, nstrains):
    """the -C world of the GPU tests: a line equal to strain 0's genome (twice), one equal to strain 1's, one other file -- so the
    per-strain rule gives every strain another set of items; -A holds a sibling's genome, -B a .gz item"""
    genomes = worlds.panel(tmp_path, 300 + nstrains, nstrains)
    c = (tmp_path / "C.txt").read_text().split("\n")[:-1]
    assert c.count(genomes[0]) == 2 and c.count(genomes[1]) == 1 and genomes[0] != genomes[1]
    others = [ln for ln in c if ln not in genomes]
    assert len(others) == 1 and (tmp_path / others[0]).exists()
    assert [len(model_items(tmp_path, g)) for g in genomes[:3]] == [2, 3, 4]
    a = (tmp_path / "A.txt").read_text().split("\n")[:-1]
    assert len(a) == 5 and genomes[1] in a and genomes[0] not in a
    b = (tmp_path / "B.txt").read_text().split("\n")[:-1]
    assert len(b) == 3 and sum(x.endswith(".gz") for x in b) == 1
    s0, s1 = [b"".join(ln for ln in (tmp_path / g).read_bytes().split(b"\n") if not ln.startswith(b">")) for g in genomes[:2]]
    assert len(s0) == len(s1) and 0 < sum(x != y for x, y in zip(s0, s1)) < len(s0) // 50, "strains 0 and 1 are siblings"


def model_items(d, genome):
    import _prevalence_model as model
    return model.list_items(str(d / "C.txt"), genome)


def test_names_are_compared_over_all_ranks_lines_and_the_class_files(tmp_path):
    """x on one rank and x.p on the other; an outfile that is another strain's class file of the scrub sweep"""
    _job(tmp_path)
    (tmp_path / "S.txt").write_text("missing1.fa\tx\nmissing2.fa\tx.p\n")
    for rank in ("0", "1"):
        before = sorted(os.listdir(tmp_path))
        p = subprocess.run([EXE] + BASE + ["--prevalence=.p"], cwd=str(tmp_path), env=dict(os.environ, WORLD_SIZE="2", RANK=rank),
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
        assert p.returncode == 1 and b"would be the one file x.p" in p.stderr and p.stderr.count(b"\n") == 1, p.stderr
        assert b"missing" not in p.stderr and sorted(os.listdir(tmp_path)) == before
    (tmp_path / "SD.txt").write_text("missing1.fa\tx.inf\tx.kmer_hits.gz\nmissing2.fa\tx.inf.classes\ty.kmer_hits.gz\n")
    before = sorted(os.listdir(tmp_path))
    p = subprocess.run([EXE] + DETECT + ["--prevalence=.p", "--scrub", "0.1,0.05"] + TAIL + ["--coverage-only", "--coverage-scrub-sweep"],
                       cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert p.returncode == 1 and b"would be the one file x.inf.classes" in p.stderr and p.stderr.count(b"\n") == 1, p.stderr
    assert b"missing" not in p.stderr and sorted(os.listdir(tmp_path)) == before
