"""Thresholds (strain_detect --coverage-thresholds, coverage_depth --thresholds; include/strainer_kmer.h has the rule), the parts
that need no device: the new ABI entries (header, export list, library symbols), the model's own arithmetic and its agreement with
the numbers the reference printed, the command lines refused before anything is opened -- each with one line on stderr, a non-zero
status and nothing written -- and the host fold (skc_report_thresholds) through strain_detect's host-only stand-alone build under
ASan + UBSan."""
import gzip
import json
import os
import re
import subprocess

import pytest

import strainer2_amd as sk
from _thresholds_model import DEFAULT, check_invariants, main_table, numbers, parse_table, table_from_hits
from strainer2_amd import native
from test_coverage_regions_host import ONE, _job, _refused, _run
from test_sanitizers import COV_CASES, prepare_cov_case

NEW = ["sk_covacc_set_thresholds", "sk_covacc_add_rows_hits", "sk_covacc_finish_target_thresholds", "sk_distinct_thresholds"]
COV = sk.cli_path("coverage_depth")
REFUSED_BY_THE_PROGRAM = {"general_text"}                      # non-ACGT k-mer text
FAILING = {"short_line", "zero_informative"}                   # cases in which the main table itself fails
BAD_LISTS = ["", ",", "1,,2", "1,", ",1", "1,1", "2,1", "0,1,2,1", "-1", "2147483647", "99999999999999999999", "1,x", "3 4",
             ",".join(str(i) for i in range(17))]


def test_new_entry_points_are_declared_listed_and_exported(repo):
    hdr = open(os.path.join(repo, "include", "strainer_kmer.h")).read()
    syms = subprocess.run(["nm", "-D", "--defined-only", sk.library_path()], capture_output=True, text=True).stdout
    for name in NEW:
        assert re.search(r"\b%s\(" % name, hdr), name
        assert name in native.ABI_SYMBOLS, name
        assert re.search(r"\bT %s$" % name, syms, re.M), name
    assert "#define SK_COVACC_THRESHOLDS_MAX 16u" in hdr and native.SK_COVACC_THRESHOLDS_MAX == 16
    assert tuple(native.DEFAULT_THRESHOLDS) == DEFAULT == (0, 1, 2, 3, 5, 10, 20, 50)
    assert ("strain_name<TAB>metagenome<TAB>min_kmer_hits<TAB>unique_observed_informative_kmers<TAB>"
            "total_observed_informative_kmers") in hdr
    for m in ("set_thresholds", "add_rows_hits", "finish_target_thresholds"):
        assert hasattr(sk.CoverageAcc, m), m
    assert hasattr(sk.KmerContext, "distinct_thresholds") and hasattr(native, "distinct_thresholds")


def test_the_model_on_a_few_lines():
    assert numbers([7, 7, 7], [1, 5, 9], [0, 4, 8, 12]) == ([1, 1, 1, 0], [3, 2, 1, 0])
    assert numbers([], [], [0, 1]) == ([0, 0], [0, 0])
    assert numbers([1, 2, 2], [4, 5, 0], [4]) == ([1], [1])                 # strictly above
    text = (b"d/m1\t1\t1\t1\t0\tAAAC\nm1\t1\t1\t1\t0\tAAAC\nm1\t2\t1\t3\t0\tAAAG\nm1\t1\t1\t0\t0\tAAAT\nm2\t0\t0\t1\t0\tAAAC\n"
            b"#m1\ttotal_kmer_evaluated\t9\n#m2\ttotal_kmer_evaluated\t9\n#m3\ttotal_kmer_evaluated\t9\n")
    assert table_from_hits(text, "x/a_b.kmer_hits.gz", (0, 1, 4), 1) == (
        b"strain_name\tmetagenome\tmin_kmer_hits\tunique_observed_informative_kmers\ttotal_observed_informative_kmers\n"
        b"a_b\tm1\t0\t3\t4\na_b\tm1\t1\t2\t3\na_b\tm1\t4\t1\t1\n"
        b"a_b\tm2\t0\t1\t1\na_b\tm2\t1\t0\t0\na_b\tm2\t4\t0\t0\n"           # below the run's filter, above t[0]: after m1, by its trailer
        b"a_b\tm3\t0\t0\t0\na_b\tm3\t1\t0\t0\na_b\tm3\t4\t0\t0\n")


def _case(name):
    d = os.path.join(COV_CASES, name)
    prepare_cov_case(name, d)
    meta = json.load(open(os.path.join(d, "case.json")))
    argv = meta["argv"]
    hits = argv[argv.index("-k") + 1]
    m = 1
    for flag in ("-m", "--min_kmer_hits"):
        if flag in argv:
            m = int(argv[argv.index(flag) + 1])
    return d, meta, hits, m


def test_the_model_reproduces_the_reference_numbers_at_the_cases_own_threshold():
    """the golden hit lists through the model alone, at t = the case's -m: the two columns the reference's script printed"""
    seen = 0
    for name in sorted(set(os.listdir(COV_CASES)) - REFUSED_BY_THE_PROGRAM - FAILING):
        d, meta, hits, m = _case(name)
        want = open(os.path.join(d, "expected.stdout"), "rb").read()
        lst = tuple(sorted({0, m, m + 1, 50}))
        got = table_from_hits(gzip.open(os.path.join(d, hits), "rb").read(), hits, lst, m)
        check_invariants(got, want, lst, m)
        at_m = {s: [(u, n) for t, u, n in rows if t == m][0] for s, rows in parse_table(got).items()}
        assert at_m == {s: (max(u, 0), n) for s, (u, n) in main_table(want).items()}, name
        seen += len(at_m)
    assert seen >= 5


# ---------------------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [["--coverage-thresholds"], ["--coverage-thresholds=t.tsv"],
                                   ["--coverage-thresholds", "--threshold-list", "1,2"]])
def test_the_flag_alone_is_refused(tmp_path, flags):
    before = _job(tmp_path)
    p = _run(ONE + flags, str(tmp_path))
    _refused(p, before, tmp_path)
    assert b"--coverage-thresholds goes with --coverage-depth or --coverage-only" in p.stderr


@pytest.mark.parametrize("table", ["--coverage-depth", "--coverage-only"])
def test_a_list_without_the_flag_is_refused(tmp_path, table):
    before = _job(tmp_path)
    p = _run(ONE + [table, "--threshold-list", "1,2"], str(tmp_path))
    _refused(p, before, tmp_path)
    assert b"--threshold-list goes with --coverage-thresholds" in p.stderr


@pytest.mark.parametrize("table", ["--coverage-depth", "--coverage-only"])
def test_a_file_name_with_several_strains_is_refused(tmp_path, table):
    before = _job(tmp_path)
    p = _run(["-S", "S.txt", "-B", "T.txt", table, "--coverage-thresholds=x"], str(tmp_path))
    _refused(p, before, tmp_path)
    assert b"--coverage-thresholds=FILE names one file" in p.stderr


@pytest.mark.parametrize("form", ["two", "one"])
@pytest.mark.parametrize("lst", BAD_LISTS)
def test_a_bad_list_is_refused(tmp_path, lst, form):
    before = _job(tmp_path)
    arg = ["--threshold-list", lst] if form == "two" else ["--threshold-list=" + lst]
    p = _run(ONE + ["--coverage-only", "--coverage-thresholds"] + arg, str(tmp_path))
    _refused(p, before, tmp_path)
    assert b"--threshold-list" in p.stderr
    assert p.returncode == _run(ONE + ["--coverage-only", "--coverage-spectrum", "--spectrum-max", "0"], str(tmp_path)).returncode


def test_behind_detect_with_several_strains(tmp_path):
    before = _job(tmp_path)
    (tmp_path / "A.txt").write_text("g.fa\n")
    before = sorted(before + ["A.txt"])
    front = ["-S", "S.txt", "-A", "A.txt", "-B", "A.txt", "--scrub", "0.01", "--detect", "-B", "T.txt"]
    p = _run(front + ["--coverage-only", "--coverage-thresholds=one.tsv"], str(tmp_path), exe=sk.cli_path())
    _refused(p, before, tmp_path)
    assert p.stderr.startswith(b"kmer_scrub_count: with -S, --coverage-thresholds takes no file name")
    p = _run(front + ["--coverage-thresholds", "--threshold-list", "7"], str(tmp_path), exe=sk.cli_path())
    _refused(p, before, tmp_path)
    assert p.stderr.startswith(b"kmer_scrub_count: --coverage-thresholds goes with --coverage-depth or --coverage-only")
    p = _run(front + ["--coverage-only", "--threshold-list", "7"], str(tmp_path), exe=sk.cli_path())
    _refused(p, before, tmp_path)
    assert p.stderr.startswith(b"kmer_scrub_count: --threshold-list goes with --coverage-thresholds")
    p = _run(front + ["--coverage-only", "--coverage-thresholds", "--threshold-list", "3,3"], str(tmp_path), exe=sk.cli_path())
    _refused(p, before, tmp_path)
    assert p.stderr.startswith(b"kmer_scrub_count: --threshold-list 3,3")


@pytest.mark.parametrize("argv", [["--thresholds", "--threshold-list", "1,1"], ["--thresholds", "--threshold-list=2,1"],
                                  ["--threshold-list", "5"], ["--thresholds=x.tsv", "--threshold-list", "abc"],
                                  ["--thresholds", "--threshold-list", ",".join(str(i) for i in range(17))],
                                  ["--thresholds", "--threshold-list", "1,,2"], ["--thresholds", "--threshold-list", "2147483647"]])
def test_coverage_depth_refuses_a_bad_list_before_it_reads(tmp_path, argv):
    before = sorted(os.listdir(tmp_path))
    p = _run(["-k", "missing.kmer_hits.gz"] + argv, str(tmp_path), exe=COV)
    _refused(p, before, tmp_path)
    assert b"--threshold" in p.stderr
    assert p.returncode == _run(["-k", "missing.kmer_hits.gz", "--spectrum", "--spectrum-max", "0"], str(tmp_path), exe=COV).returncode


# ---------------------------------------------------------------------------------------------------------------------------------
# the host fold, without a device: strain_detect's host layer over the CPU double of the device calls (the stand-alone program
# tests/test_sanitizers.py builds), under ASan + UBSan.  The double has no coverage accumulator, so --coverage-only counts on the
# host too: both flags go through skc_add_hit's kept lines and skc_report_thresholds.
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sd_host_exe(tmp_path_factory):
    from test_sanitizers import SD_SOURCES
    exe = str(tmp_path_factory.mktemp("sdth") / "sd_host")
    subprocess.run(["gcc", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer"] + SD_SOURCES +
                   ["-lz", "-lpthread", "-o", exe], check=True)
    return exe


@pytest.mark.parametrize("name,lst,m", [("batch", None, 1), ("batch", (0,), 1), ("batch", (3, 4, 5, 2147483646), 0), ("cli_pe", (0, 1, 2), 2),
                                        ("cli_pei", tuple(range(16)), 1), ("cli_se", (2, 40), 100)])
def test_the_host_fold_through_the_host_only_build(sd_host_exe, golden, tmp_path, name, lst, m):
    from test_sanitizers import ENV
    d = os.path.join(golden, "sd_cases", name)
    meta = json.load(open(os.path.join(d, "case.json")))
    tables = {}
    for flag in ("--coverage-depth", "--coverage-only"):
        argv = list(meta["argv"])
        hits = str(tmp_path / flag / "a_b_c.kmer_hits.gz")
        os.mkdir(tmp_path / flag)
        argv[argv.index("-o") + 1] = hits
        extra = ["--threshold-list", ",".join(map(str, lst))] if lst else []
        p = subprocess.run([sd_host_exe] + argv + [flag, "--coverage-thresholds", "--min-kmer-hits", str(m)] + extra, cwd=d,
                           env=dict(ENV, SK_THREADS="4"), capture_output=True)
        for bad in (b"runtime error", b"AddressSanitizer"):
            assert bad not in p.stderr, p.stderr.decode()[-3000:]
        assert p.returncode == 0, p.stderr.decode()[-1000:]
        tables[flag] = (open(hits[: -len(".kmer_hits.gz")] + ".coverage_thresholds", "rb").read(),
                        open(hits[: -len(".kmer_hits.gz")] + ".coverage_depth", "rb").read())
        q = subprocess.run([sd_host_exe] + argv + [flag, "--min-kmer-hits", str(m)], cwd=d, env=dict(ENV, SK_THREADS="4"), capture_output=True)
        assert q.returncode == 0 and (q.stdout, q.stderr) == (p.stdout, p.stderr)          # ... and nothing else changes
        assert open(hits[: -len(".kmer_hits.gz")] + ".coverage_depth", "rb").read() == tables[flag][1]
    want = table_from_hits(open(os.path.join(d, "expected.hits"), "rb").read(), "a_b_c.kmer_hits.gz", lst or DEFAULT, m)   # the REFERENCE's hit list
    assert tables["--coverage-depth"] == tables["--coverage-only"] and tables["--coverage-depth"][0] == want
    assert want.count(b"\n") >= 1 + len(lst or DEFAULT)
    check_invariants(want, tables["--coverage-depth"][1], lst or DEFAULT, m)
