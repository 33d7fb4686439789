"""The depth spectrum (strain_detect --coverage-spectrum, coverage_depth --spectrum; include/strainer_kmer.h has the rule), the parts
that need no device: the new ABI entries (header, export list, library symbols), the model's own arithmetic, and the command lines
refused before anything is opened -- each with one line on stderr, a non-zero status and nothing written.  coverage_depth itself
counts on the device, so its cases -- the hit lists under tests/golden/cov_cases against the model (tests/_spectrum_model.py) and
against the two numbers the reference printed for them -- carry the gpu mark, as the program's existing tests do."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

import strainer2_amd as sk
from _spectrum_model import check_invariants, parse_table, spectrum, table_from_hits
from strainer2_amd import native
from test_coverage_regions_host import ONE, _job, _refused, _run
from test_sanitizers import COV_CASES, prepare_cov_case

NEW = ["sk_covacc_set_spectrum", "sk_covacc_finish_target_spectrum", "sk_distinct_spectrum"]
COV = sk.cli_path("coverage_depth")
REFUSED_BY_THE_PROGRAM = {"general_text"}                      # non-ACGT k-mer text
FAILING = {"short_line", "zero_informative"}                   # cases in which the main table itself fails


def test_new_entry_points_are_declared_listed_and_exported(repo):
    hdr = open(os.path.join(repo, "include", "strainer_kmer.h")).read()
    syms = subprocess.run(["nm", "-D", "--defined-only", sk.library_path()], capture_output=True, text=True).stdout
    for name in NEW:
        assert re.search(r"\b%s\(" % name, hdr), name
        assert name in native.ABI_SYMBOLS, name
        assert re.search(r"\bT %s$" % name, syms, re.M), name
    assert "#define SK_COVACC_SPECTRUM_MAX 1023u" in hdr and native.SK_COVACC_SPECTRUM_MAX == 1023
    assert "strain_name<TAB>metagenome<TAB>depth<TAB>informative_kmers<TAB>observed_hits" in hdr
    assert hasattr(sk.CoverageAcc, "set_spectrum") and hasattr(sk.CoverageAcc, "finish_target_spectrum")
    assert hasattr(sk.KmerContext, "distinct_spectrum") and hasattr(native, "distinct_spectrum")


def test_the_model_on_a_depth_array():
    bins, deep = spectrum([0, 1, 1, 2, 3, 4, 70000, 0], 2)
    assert bins.tolist() == [2, 1, 3] and deep == 3 + 4 + 70000
    bins, deep = spectrum([], 5)
    assert bins.tolist() == [0] * 6 and deep == 0
    bins, deep = spectrum([1023, 1024], 1023)
    assert int(bins[1022]) == 1 and int(bins[1023]) == 1 and deep == 1024
    text = (b"d/m1\t1\t1\t1\t0\tAAAC\nm1\t1\t1\t1\t0\tAAAC\nm1\t2\t1\t0\t0\tAAAG\nm1\t1\t1\t0\t0\tAAAT\nm2\t3\t1\t0\t0\tAAAC\n"
            b"#m1\ttotal_kmer_evaluated\t9\n#m1\ttotal_genome_informative_kmers\t7\n#m3\ttotal_kmer_evaluated\t9\n"
            b"#m3\ttotal_genome_informative_kmers\t7  \n")
    assert table_from_hits(text, "x/a_b.kmer_hits.gz", 1) == (
        b"strain_name\tmetagenome\tdepth\tinformative_kmers\tobserved_hits\n"
        b"a_b\tm1\t0\t5\t0\na_b\tm1\t1\t1\t1\na_b\tm1\t>1\t1\t2\na_b\tm2\t1\t1\t1\na_b\tm3\t0\t7\t0\n")


# ---------------------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [["--coverage-spectrum"], ["--coverage-spectrum=s.tsv"], ["--coverage-spectrum", "--spectrum-max", "9"]])
def test_the_flag_alone_is_refused(tmp_path, flags):
    before = _job(tmp_path)
    p = _run(ONE + flags, str(tmp_path))
    _refused(p, before, tmp_path)
    assert b"--coverage-spectrum goes with --coverage-depth or --coverage-only" in p.stderr


@pytest.mark.parametrize("table", ["--coverage-depth", "--coverage-only"])
def test_a_maximum_without_the_flag_is_refused(tmp_path, table):
    before = _job(tmp_path)
    p = _run(ONE + [table, "--spectrum-max", "10"], str(tmp_path))
    _refused(p, before, tmp_path)
    assert b"--spectrum-max goes with --coverage-spectrum" in p.stderr


@pytest.mark.parametrize("table", ["--coverage-depth", "--coverage-only"])
def test_a_file_name_with_several_strains_is_refused(tmp_path, table):
    before = _job(tmp_path)
    p = _run(["-S", "S.txt", "-B", "T.txt", table, "--coverage-spectrum=x"], str(tmp_path))
    _refused(p, before, tmp_path)
    assert b"--coverage-spectrum=FILE names one file" in p.stderr


@pytest.mark.parametrize("d", [["--spectrum-max", "0"], ["--spectrum-max=0"], ["--spectrum-max", "1024"], ["--spectrum-max", "-3"],
                               ["--spectrum-max", "12x"], ["--spectrum-max", ""], ["--spectrum-max", "99999999999999999999"]])
def test_a_bad_maximum_is_refused(tmp_path, d):
    before = _job(tmp_path)
    p = _run(ONE + ["--coverage-only", "--coverage-spectrum"] + d, str(tmp_path))
    _refused(p, before, tmp_path)
    assert b"--spectrum-max" in p.stderr and b"from 1 to 1023" in p.stderr


def test_behind_detect_with_several_strains(tmp_path):
    before = _job(tmp_path)
    (tmp_path / "A.txt").write_text("g.fa\n")
    before = sorted(before + ["A.txt"])
    front = ["-S", "S.txt", "-A", "A.txt", "-B", "A.txt", "--scrub", "0.01", "--detect", "-B", "T.txt"]
    p = _run(front + ["--coverage-only", "--coverage-spectrum=one.tsv"], str(tmp_path), exe=sk.cli_path())
    _refused(p, before, tmp_path)
    assert p.stderr.startswith(b"kmer_scrub_count: with -S, --coverage-spectrum takes no file name")
    p = _run(front + ["--coverage-spectrum", "--spectrum-max", "7"], str(tmp_path), exe=sk.cli_path())
    _refused(p, before, tmp_path)
    assert p.stderr.startswith(b"kmer_scrub_count: --coverage-spectrum goes with --coverage-depth or --coverage-only")


@pytest.mark.parametrize("argv", [["--spectrum", "--spectrum-max", "0"], ["--spectrum", "--spectrum-max=1024"], ["--spectrum-max", "5"],
                                  ["--spectrum=x.tsv", "--spectrum-max", "abc"]])
def test_coverage_depth_refuses_a_bad_maximum_before_it_reads(tmp_path, argv):
    before = sorted(os.listdir(tmp_path))
    p = _run(["-k", "missing.kmer_hits.gz"] + argv, str(tmp_path), exe=COV)
    _refused(p, before, tmp_path)
    assert b"--spectrum" in p.stderr


# ---------------------------------------------------------------------------------------------------------------------------------
# coverage_depth --spectrum on the golden hit lists (the program counts on the device)
# ---------------------------------------------------------------------------------------------------------------------------------
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


@pytest.mark.gpu
@pytest.mark.parametrize("D", [1, 2, 255])
@pytest.mark.parametrize("name", sorted(set(os.listdir(COV_CASES)) - REFUSED_BY_THE_PROGRAM - FAILING))
def test_coverage_depth_spectrum_equals_the_model(tmp_path, name, D):
    import gzip
    d, meta, hits, m = _case(name)
    out = tmp_path / "sp.tsv"
    p = subprocess.run([COV] + meta["argv"] + ["--spectrum=" + str(out), "--spectrum-max", str(D)], cwd=d, capture_output=True)
    want_main = open(os.path.join(d, "expected.stdout"), "rb").read()
    assert (p.returncode, p.stdout) == (0, want_main), p.stderr.decode()[-500:]      # the main table's bytes are unchanged
    got = out.read_bytes()
    assert got == table_from_hits(gzip.open(os.path.join(d, hits), "rb").read(), hits, D, m)
    check_invariants(got, want_main)                                                # ... and the reference's two numbers
    if name == "no_stats":                                                           # no trailer: no 0 line
        assert all(lab != b"0" for rows in parse_table(got).values() for lab, _, _ in rows)
    if name == "oneword":                                                            # a sample without a hit line: its 0 line alone
        assert parse_table(got)[b"m0.fa"] == [(b"0", 3, 0)]
    if name == "basic" and D == 1:
        assert any(lab == b">1" for lab, _, _ in parse_table(got)[b"s1_PE1.fastq.gz"])


@pytest.mark.gpu
def test_coverage_depth_spectrum_default_path_and_default_maximum(tmp_path):
    import gzip
    import shutil
    d, meta, hits, m = _case("basic")
    shutil.copy(os.path.join(d, hits), tmp_path / hits)
    p = subprocess.run([COV, "-k", hits, "--spectrum"], cwd=tmp_path, capture_output=True)
    assert (p.returncode, p.stdout) == (0, open(os.path.join(d, "expected.stdout"), "rb").read())
    got = (tmp_path / (hits[: -len(".kmer_hits.gz")] + ".coverage_spectrum")).read_bytes()
    assert got == table_from_hits(gzip.open(tmp_path / hits, "rb").read(), hits, 255, 1)
    assert sorted(os.listdir(tmp_path)) == sorted([hits, hits[: -len(".kmer_hits.gz")] + ".coverage_spectrum"])


@pytest.mark.gpu
def test_coverage_depth_refuses_general_text(tmp_path):
    d, meta, hits, m = _case("general_text")
    out = tmp_path / "sp.tsv"
    p = subprocess.run([COV] + meta["argv"] + ["--spectrum=" + str(out)], cwd=d, capture_output=True)
    assert p.returncode != 0 and p.stdout == b"" and p.stderr.count(b"\n") == 1 and b"--spectrum" in p.stderr
    assert not out.exists()


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(FAILING))
def test_coverage_depth_failing_cases_fail_as_before(tmp_path, name):
    d, meta, hits, m = _case(name)
    out = tmp_path / "sp.tsv"
    p = subprocess.run([COV] + meta["argv"] + ["--spectrum=" + str(out)], cwd=d, capture_output=True)
    assert p.returncode == meta["returncode"] and p.stdout == open(os.path.join(d, "expected.stdout"), "rb").read()
    assert not out.exists()


def test_the_model_agrees_with_the_reference_numbers_without_a_device():
    """the golden hit lists through the model alone: its bins sum to the unique and total columns the reference printed"""
    import gzip
    for name in sorted(set(os.listdir(COV_CASES)) - REFUSED_BY_THE_PROGRAM - FAILING):
        d, meta, hits, m = _case(name)
        for D in (1, 255):
            check_invariants(table_from_hits(gzip.open(os.path.join(d, hits), "rb").read(), hits, D, m),
                             open(os.path.join(d, "expected.stdout"), "rb").read())
    assert np.array_equal(spectrum(np.array([5, 5, 1]), 4)[0], [1, 0, 0, 0, 2])


# ---------------------------------------------------------------------------------------------------------------------------------
# the host fold, without a device: strain_detect's host layer over the CPU double of the device calls (the stand-alone program
# tests/test_sanitizers.py builds), under ASan + UBSan.  The double has no coverage accumulator, so --coverage-only counts on the
# host too: both flags go through skc_report_spectrum.
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sd_host_exe(tmp_path_factory):
    from test_sanitizers import SD_SOURCES
    exe = str(tmp_path_factory.mktemp("sdsp") / "sd_host")
    subprocess.run(["gcc", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer"] + SD_SOURCES +
                   ["-lz", "-lpthread", "-o", exe], check=True)
    return exe


@pytest.mark.parametrize("name,D", [("batch", 1), ("batch", 255), ("cli_pe", 2), ("cli_pei", 1), ("cli_se", 1023)])
def test_the_host_fold_through_the_host_only_build(sd_host_exe, golden, tmp_path, name, D):
    import gzip
    from test_sanitizers import ENV
    d = os.path.join(golden, "sd_cases", name)
    meta = json.load(open(os.path.join(d, "case.json")))
    tables = {}
    for flag in ("--coverage-depth", "--coverage-only"):
        argv = list(meta["argv"])
        hits = str(tmp_path / flag / "a_b_c.kmer_hits.gz")
        os.mkdir(tmp_path / flag)
        argv[argv.index("-o") + 1] = hits
        p = subprocess.run([sd_host_exe] + argv + [flag, "--coverage-spectrum", "--spectrum-max", str(D)], cwd=d,
                           env=dict(ENV, SK_THREADS="4"), capture_output=True)
        for bad in (b"runtime error", b"AddressSanitizer"):
            assert bad not in p.stderr, p.stderr.decode()[-3000:]
        assert p.returncode == 0, p.stderr.decode()[-1000:]
        tables[flag] = (open(hits[: -len(".kmer_hits.gz")] + ".coverage_spectrum", "rb").read(),
                        open(hits[: -len(".kmer_hits.gz")] + ".coverage_depth", "rb").read())
    want = table_from_hits(open(os.path.join(d, "expected.hits"), "rb").read(), "a_b_c.kmer_hits.gz", D, 1)    # the REFERENCE's hit list
    assert tables["--coverage-depth"] == tables["--coverage-only"] and tables["--coverage-depth"][0] == want
    assert want.count(b"\n") >= 3
    check_invariants(want, tables["--coverage-depth"][1])
