"""The scrub sweep (include/strainer_kmer.h has the rule), the parts that need no device: the premise itself -- the informative sets
of one strain at descending fractions are nested -- asserted on the EXISTING single-fraction step 2 (the filter oracle, pinned to the
reference script by tests/golden/filter_cases) over the golden cases and over random tables with heavy ties; the new ABI entries
(header, export list, library symbols); the command lines refused before anything is opened, each with one line on stderr, a
non-zero status and nothing written; and the host side (class-file parsing, skc_report_classes) in a stand-alone program under
ASan + UBSan (tests/native/sweep_sanitize.c)."""
import gzip
import json
import os
import random
import re
import subprocess

import pytest

import strainer2_amd as sk
from _sweep_model import LISTS, class_file, classes, numbers_by_class, parse_sweep, sets_by_runs, sweep_table
from strainer2_amd import native
from test_coverage_regions_host import ONE, _job, _refused, _run
from test_sanitizers import ENV, REPO

NEW = ["sk_filter_classes_joint", "sk_filter_classes_above", "sk_covacc_set_classes", "sk_covacc_finish_target_classes", "sk_distinct_classes"]
FCASES = os.path.join(REPO, "tests", "golden", "filter_cases")
ORACLE = os.path.join(REPO, "oracle", "ksf_oracle")
FILTER = sk.cli_path("kmer_scrub_filter")
COV = sk.cli_path("coverage_depth")
BAD_LISTS = ["", ",", "0.5,,0.1", "0.5,", ",0.5", "0.5,0.5", "0.1,0.5", "0.5,0.1,0.2", "1.5", "-0.1", "abc", "0.5x", "nan", "0.5 0.1",
             ",".join("0.%02d" % (90 - i) for i in range(17))]


def test_new_entry_points_are_declared_listed_and_exported(repo):
    hdr = open(os.path.join(repo, "include", "strainer_kmer.h")).read()
    syms = subprocess.run(["nm", "-D", "--defined-only", sk.library_path()], capture_output=True, text=True).stdout
    for name in NEW:
        assert re.search(r"\b%s\(" % name, hdr), name
        assert name in native.ABI_SYMBOLS, name
        assert re.search(r"\bT %s$" % name, syms, re.M), name
    assert "#define SK_SCRUB_SWEEP_MAX 16u" in hdr and native.SK_SCRUB_SWEEP_MAX == 16
    assert ("strain_name<TAB>metagenome<TAB>min_fraction<TAB>genome_num_informative_kmers<TAB>unique_observed_informative_kmers<TAB>"
            "total_observed_informative_kmers") in hdr
    assert "a row is in set q iff class >= q + 1" in hdr
    for m in ("set_classes", "finish_target_classes"):
        assert hasattr(sk.CoverageAcc, m), m
    for m in ("classes_joint", "classes_above"):
        assert hasattr(native.ScrubFilter, m), m
    assert hasattr(sk.KmerContext, "distinct_classes")


# ---------------------------------------------------------------------------------------------------------------------------------
# the model and the premise
# ---------------------------------------------------------------------------------------------------------------------------------
def test_the_model_on_a_few_sets():
    sets = [[b"A", b"C", b"G", b"T"], [b"A", b"G", b"T"], [b"G"]]
    assert classes(sets) == {b"A": 2, b"C": 1, b"G": 3, b"T": 2}
    assert class_file(["0.5", "0.1", "0"], sets) == b"#min_fractions\t0.5,0.1,0\n#post_scrub_kmers\t4,3,1\nA\t2\nC\t1\nG\t3\nT\t2\n"
    with pytest.raises(AssertionError):
        classes([[b"A", b"C"], [b"C", b"A"]])                # the order changed
    with pytest.raises(AssertionError):
        classes([[b"A"], [b"A", b"C"]])                      # the smaller fraction's set is larger
    uq, tot, stray = numbers_by_class([0, 2, 1, 5, 3, 1], [1, 1, 2, 3, 0, 4], 3)
    assert uq.tolist() == [3, 2, 1] and tot.tolist() == [8, 6, 5] and stray == 2
    head = b"strain_name\tspecies_name\tgenus_name\tgenome_num_total_kmers\tgenome_num_informative_kmers\tmetagenome\ta\tb\tu\tt\n"
    t0 = head + b"G_s_x\ts\tG\t90\t40\tm1\t0\t0\t7\t9\nG_s_x\ts\tG\t90\t40\tm2\t0\t0\t-1\t0\n"
    t1 = head + b"G_s_x\ts\tG\t90\t10\tm2\t0\t0\t0\t0\nG_s_x\ts\tG\t90\t10\tm1\t0\t0\t2\t3\n"
    got = sweep_table(["0.5", "0.1"], [t0, t1])
    assert parse_sweep(got) == {b"m1": [("0.5", 40, 7, 9), ("0.1", 10, 2, 3)], b"m2": [("0.5", 40, 0, 0), ("0.1", 10, 0, 0)]}


def _oracle(argv, cwd):
    try:                                                     # (a walk whose column can never keep min_fraction does not end, in the script either)
        p = subprocess.run([ORACLE] + argv, cwd=cwd, capture_output=True, stdin=subprocess.DEVNULL, timeout=3)
    except subprocess.TimeoutExpired:
        return None
    return p.stdout if p.returncode == 0 else None


def _without_m(argv):
    out, skip = [], False
    for a in argv:
        if skip:
            skip = False
        elif a in ("-m", "--min_fraction"):
            skip = True
        elif not (a.startswith("--min_fraction=") or (a.startswith("-m") and len(a) > 2)):
            out.append(a)
    return out


@pytest.mark.parametrize("lst", LISTS)
def test_the_sets_are_nested_over_the_golden_filter_cases(lst):
    """every golden case the reference script finished, rerun at each fraction of the list: nested sets, and a run that succeeds at
    the largest fraction succeeds at every smaller one (the drug-scrub exception is hardest at the largest)"""
    fr = lst.split(",")
    seen = modes = 0
    for name in sorted(os.listdir(FCASES)):
        d = os.path.join(FCASES, name)
        meta = json.load(open(os.path.join(d, "case.json")))
        if meta["returncode"] != 0:
            continue
        argv = _without_m(meta["argv"])
        first = _oracle(argv + ["-m", fr[0]], d)
        if first is None:
            continue                                         # (fails at f0: so does the sweep run)
        sets = sets_by_runs(lambda f: _oracle(argv + ["-m", f], d), fr)
        assert sets is not None, name
        classes(sets)
        seen += 1
        modes += "-i" in argv or "--independent" in argv
    assert seen >= 15 and modes >= 4                         # (no drug case passes 2 x f0 at these lists: the random tables below have a third)


def _random_table(path, rng, n, drug, dup):
    keys = ["".join(rng.choice("ACGT") for _ in range(31)) for _ in range(n)]
    with gzip.GzipFile(path, "wb", mtime=0) as g:
        g.write(b"#kmer\treference_count\tpangenome_count\tmetagenome_count\tdrug_count\n")
        for k in keys + [rng.choice(keys) for _ in range(dup)]:
            line = "%s\t1\t%d\t%d" % (k, rng.choice([0, 0, 1, 1, 1, 2, 7]), rng.choice([0, 1, 1, 2, 2, 2, 3, 50]))
            g.write((line + ("\t%d\n" % (rng.random() < 0.03) if drug else "\n")).encode())


@pytest.mark.parametrize("lst", LISTS + ("0.45,0.2,0.04,0.01,0",))      # (a drug scrub never leaves 2 x 0.9 of a strain)
@pytest.mark.parametrize("drug", [False, True])
@pytest.mark.parametrize("mode", [[], ["-i"]])
def test_the_sets_are_nested_over_random_tables_with_heavy_ties(tmp_path, mode, drug, lst):
    rng = random.Random(len(lst) * 100 + len(mode) * 10 + drug)
    fr = lst.split(",")
    done = 0
    for n, dup in ((1, 0), (40, 3), (3000, 0), (5000, 60)):
        t = str(tmp_path / f"t{n}.gz")
        _random_table(t, rng, n, drug, dup)
        if _oracle(["-s", t, "-m", fr[0]] + mode, str(tmp_path)) is None:
            continue                                         # (the drug scrub leaves too little at f0)
        sets = sets_by_runs(lambda f: _oracle(["-s", t, "-m", f] + mode, str(tmp_path)), fr)
        assert sets is not None
        cl = classes(sets)
        done += 1
        if n >= 3000 and not mode and len(fr) > 2:
            assert len(set(cl.values())) >= 3                # at least three of the sets differ
    if not drug or float(fr[0]) < 0.5:
        assert done >= 3


# ---------------------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------------------
def _filter_refused(tmp_path, argv, word):
    (tmp_path / "t.txt").write_bytes(b"AAAC\t1\t1\t1\n")
    before = sorted(os.listdir(tmp_path))
    p = _run(["-s", "t.txt"] + argv, str(tmp_path), exe=FILTER)
    assert p.returncode == 2 and p.stdout == b"" and p.stderr.count(b"\n") == 1 and word in p.stderr, p.stderr
    assert sorted(os.listdir(tmp_path)) == before
    return p


@pytest.mark.parametrize("argv", [["--min_fraction_list", "0.5,0.1"], ["--min_fraction_list=0.5,0.1"], ["--classes_out", "c.txt"],
                                  ["--classes_out=c.txt"]])
def test_filter_either_flag_without_the_other(tmp_path, argv):
    _filter_refused(tmp_path, argv, b"go together")


@pytest.mark.parametrize("m", [["-m", "0.5"], ["--min_fraction=0.5"], ["-m0.5"]])
def test_filter_the_list_together_with_m(tmp_path, m):
    _filter_refused(tmp_path, ["--min_fraction_list", "0.5,0.1", "--classes_out", "c.txt"] + m, b"replaces --min_fraction")


REASONS = {"": b"an empty field", ",": b"an empty field", "0.5,,0.1": b"an empty field", "0.5,": b"an empty field", ",0.5": b"an empty field",
           "0.5,0.5": b"descend strictly", "0.1,0.5": b"descend strictly", "0.5,0.1,0.2": b"descend strictly", "1.5": b"out of range",
           "-0.1": b"out of range", "abc": b"is no number", "0.5x": b"is no number", "nan": b"is no number", "0.5 0.1": b"is no number"}


@pytest.mark.parametrize("form", ["two", "one"])
@pytest.mark.parametrize("lst", BAD_LISTS)
def test_filter_a_bad_list(tmp_path, lst, form):
    arg = ["--min_fraction_list", lst] if form == "two" else ["--min_fraction_list=" + lst]
    p = _filter_refused(tmp_path, arg + ["--classes_out", "c.txt"], b"--min_fraction_list " + lst.encode() + b": ")
    assert REASONS.get(lst, b"more than 16 fractions") in p.stderr, p.stderr


FUSED = ["-A", "A.txt", "-B", "A.txt"]


@pytest.mark.parametrize("front", [["-r", "g.fa"], ["-S", "S.txt"]])
def test_fused_refusals(tmp_path, front):
    before = _job(tmp_path)
    (tmp_path / "A.txt").write_text("g.fa\n")
    before = sorted(before + ["A.txt"])
    tail = ["--detect", "-B", "T.txt"] + (["-o", "x.kmer_hits.gz"] if front[0] == "-r" else [])
    for argv, word in ((["--scrub", "0.5,0.1"] + tail + ["--coverage-only"], b"goes with --detect ... --coverage-scrub-sweep"),
                       (["--scrub", "0.5,0.1"], b"--scrub"),                # (-S takes no --scrub without --detect at all)
                       (["--scrub", "0.5"] + tail + ["--coverage-only", "--coverage-scrub-sweep"], b"goes with a list of fractions"),
                       (["--scrub", "0.1,0.5"] + tail + ["--coverage-only", "--coverage-scrub-sweep"], b"--scrub 0.1,0.5: 0.5 after 0.1: the list must descend strictly"),
                       (["--scrub", "0.5,"] + tail + ["--coverage-only", "--coverage-scrub-sweep"], b"an empty field"),
                       (["--scrub", "0.5,0.1"] + tail + ["--coverage-only", "--coverage-scrub-sweep", "--scrub-classes", "c"], b"no --scrub-classes")):
        p = _run(front + FUSED + argv, str(tmp_path), exe=sk.cli_path())
        _refused(p, before, tmp_path)
        assert word in p.stderr, (argv, p.stderr)



@pytest.mark.parametrize("flags", [["--coverage-scrub-sweep"], ["--coverage-scrub-sweep=t.tsv"], ["--coverage-scrub-sweep", "--scrub-classes", "c"]])
def test_the_flag_alone_is_refused(tmp_path, flags):
    before = _job(tmp_path)
    p = _run(ONE + flags, str(tmp_path))
    _refused(p, before, tmp_path)
    assert b"--coverage-scrub-sweep goes with --coverage-depth or --coverage-only" in p.stderr


@pytest.mark.parametrize("table", ["--coverage-depth", "--coverage-only"])
def test_classes_without_the_flag_are_refused(tmp_path, table):
    before = _job(tmp_path)
    p = _run(ONE + [table, "--scrub-classes", "c.txt"], str(tmp_path))
    _refused(p, before, tmp_path)
    assert b"--scrub-classes goes with --coverage-scrub-sweep" in p.stderr


GOOD = b"#min_fractions\t0.5,0.1\n#post_scrub_kmers\t1,1\nACGTTGCAAGGCTTAACCGGTTAACCGTAGC\t2\n"


@pytest.mark.parametrize("table", ["--coverage-depth", "--coverage-only"])
def test_a_background_list_is_refused(tmp_path, table):
    before = _job(tmp_path)
    (tmp_path / "inf.txt.classes").write_bytes(GOOD)
    (tmp_path / "bg.txt").write_text("SE\tg.fa\n")
    (tmp_path / "Sg.txt").write_text("g.fa\tinf.txt\tGenus_species_a.kmer_hits.gz\ng.fa\tinf.txt\tGenus_species_b.kmer_hits.gz\tbg.txt\n")
    before = sorted(before + ["inf.txt.classes", "bg.txt", "Sg.txt"])
    for argv in (ONE + ["-g", "bg.txt"], ["-S", "Sg.txt", "-B", "T.txt"]):
        p = _run(argv + [table, "--coverage-scrub-sweep"], str(tmp_path))
        _refused(p, before, tmp_path)
        assert b"does not go with a -g list" in p.stderr and b"nested" in p.stderr


@pytest.mark.parametrize("table", ["--coverage-depth", "--coverage-only"])
@pytest.mark.parametrize("flags", [["--coverage-scrub-sweep=x.tsv"], ["--coverage-scrub-sweep", "--scrub-classes", "inf.txt.classes"]])
def test_file_names_with_several_strains_are_refused(tmp_path, table, flags):
    before = _job(tmp_path)
    (tmp_path / "inf.txt.classes").write_bytes(GOOD)
    before = sorted(before + ["inf.txt.classes"])
    p = _run(["-S", "S.txt", "-B", "T.txt", table] + flags, str(tmp_path))
    _refused(p, before, tmp_path)
    assert b"name one file" in p.stderr


CLASS_FILES = {
    "missing": None,
    "empty": b"",
    "no_header": b"ACGTTGCAAGGCTTAACCGGTTAACCGTAGC\t1\n",
    "bad_list": b"#min_fractions\t0.1,0.5\n#post_scrub_kmers\t1,1\nACGTTGCAAGGCTTAACCGGTTAACCGTAGC\t2\n",
    "class_0": b"#min_fractions\t0.5,0.1\n#post_scrub_kmers\t1,1\nACGTTGCAAGGCTTAACCGGTTAACCGTAGC\t0\n",
    "class_3": b"#min_fractions\t0.5,0.1\n#post_scrub_kmers\t1,1\nACGTTGCAAGGCTTAACCGGTTAACCGTAGC\t3\n",
    "sizes_off": b"#min_fractions\t0.5,0.1\n#post_scrub_kmers\t2,1\nACGTTGCAAGGCTTAACCGGTTAACCGTAGC\t2\n",
    "another_kmer": b"#min_fractions\t0.5,0.1\n#post_scrub_kmers\t1,1\nACGTTGCAAGGCTTAACCGGTTAACCGTAGG\t2\n",
    "one_more": b"#min_fractions\t0.5,0.1\n#post_scrub_kmers\t2,1\nACGTTGCAAGGCTTAACCGGTTAACCGTAGC\t2\nCGTTGCAAGGCTTAACCGGTTAACCGTAGCT\t1\n",
    "none": b"#min_fractions\t0.5,0.1\n#post_scrub_kmers\t0,0\n",
    "twice": b"#min_fractions\t0.5,0.1\n#post_scrub_kmers\t2,2\nACGTTGCAAGGCTTAACCGGTTAACCGTAGC\t2\nACGTTGCAAGGCTTAACCGGTTAACCGTAGC\t2\n",
}


@pytest.mark.parametrize("table", ["--coverage-depth", "--coverage-only"])
@pytest.mark.parametrize("where", ["default", "named", "S"])
@pytest.mark.parametrize("case", sorted(CLASS_FILES))
def test_a_class_file_that_is_missing_malformed_or_inconsistent_is_refused(tmp_path, case, where, table):
    """before a strain is opened or a target read: nothing is written"""
    before = _job(tmp_path)
    name = "other.classes" if where == "named" else "inf.txt.classes"
    if CLASS_FILES[case] is not None:
        (tmp_path / name).write_bytes(CLASS_FILES[case])
        before = sorted(before + [name])
    argv = (["-S", "S.txt", "-B", "T.txt"] if where == "S" else ONE) + [table, "--coverage-scrub-sweep"] + (["--scrub-classes", name] if where == "named" else [])
    p = _run(argv, str(tmp_path))
    _refused(p, before, tmp_path)
    assert b"--coverage-scrub-sweep: class file" in p.stderr and name.encode() in p.stderr


@pytest.mark.parametrize("argv", [["--scrub-sweep"], ["--scrub-sweep=x.tsv"], ["--scrub-classes", "c.classes"], ["--scrub-classes=c.classes"]])
def test_coverage_depth_either_flag_without_the_other(tmp_path, argv):
    (tmp_path / "c.classes").write_bytes(GOOD)
    before = sorted(os.listdir(tmp_path))
    p = _run(["-k", "missing.kmer_hits.gz"] + argv, str(tmp_path), exe=COV)
    _refused(p, before, tmp_path)
    assert b"go together" in p.stderr


@pytest.mark.parametrize("case", sorted(set(CLASS_FILES) - {"another_kmer", "one_more", "none", "twice"}))
def test_coverage_depth_refuses_a_bad_class_file_before_it_reads(tmp_path, case):
    if CLASS_FILES[case] is not None:
        (tmp_path / "c.classes").write_bytes(CLASS_FILES[case])
    before = sorted(os.listdir(tmp_path))
    p = _run(["-k", "missing.kmer_hits.gz", "--scrub-classes", "c.classes", "--scrub-sweep"], str(tmp_path), exe=COV)
    _refused(p, before, tmp_path)
    assert b"--scrub-classes c.classes" in p.stderr
    assert p.returncode == _run(["-k", "missing.kmer_hits.gz", "--spectrum", "--spectrum-max", "0"], str(tmp_path), exe=COV).returncode


# ---------------------------------------------------------------------------------------------------------------------------------
# the host side under ASan + UBSan, stand-alone
# ---------------------------------------------------------------------------------------------------------------------------------
def test_class_files_and_the_host_fold_under_sanitizers(tmp_path):
    exe = str(tmp_path / "sweep_sanitize")
    subprocess.run(["gcc", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                    os.path.join(REPO, "tests", "native", "sweep_sanitize.c"), os.path.join(REPO, "strainer2_amd", "csrc", "sk_host_cov.c"),
                    "-lz", "-o", exe], check=True)
    work = tmp_path / "files"
    work.mkdir()
    p = subprocess.run([exe, str(work)], env=ENV, capture_output=True, timeout=120)
    assert (p.returncode, p.stdout, p.stderr) == (0, b"sweep_sanitize: ok\n", b""), p.stderr.decode()[-3000:]
