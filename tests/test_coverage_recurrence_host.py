"""Recurrence (strain_detect --coverage-recurrence [--recurrence-pairs], coverage_depth --recurrence; include/strainer_kmer.h has
the rule), the parts that need no device: the new ABI entries (header, export list, library symbols), the model's own arithmetic
(tests/_recurrence_model.py), the command lines refused before anything is opened -- each with one line on stderr, a non-zero status
and nothing written -- and the host fold (skc_report_recurrence) on crafted lists against a brute-force loop, in a stand-alone C
program under AddressSanitizer + UBSan (tests/native/recur_sanitize.c)."""
import os
import re
import subprocess

import numpy as np
import pytest

import strainer2_amd as sk
from _recurrence_model import HIST_HEADER, PAIRS_HEADER, check_tables, recurrence, tables_from_hits
from strainer2_amd import native
from test_coverage_regions_host import ONE, _job, _refused, _run
from test_sanitizers import ENV, REPO

NEW = ["sk_recur_create", "sk_recur_destroy", "sk_recur_mark_bits", "sk_recur_finish", "sk_covacc_set_recurrence", "sk_covacc_mark_target",
       "sk_distinct_recurrence"]
COV = sk.cli_path("coverage_depth")


def test_new_entry_points_are_declared_listed_and_exported(repo):
    hdr = open(os.path.join(repo, "include", "strainer_kmer.h")).read()
    syms = subprocess.run(["nm", "-D", "--defined-only", sk.library_path()], capture_output=True, text=True).stdout
    for name in NEW:
        assert re.search(r"\b%s\(" % name, hdr), name
        assert name in native.ABI_SYMBOLS, name
        assert re.search(r"\bT %s$" % name, syms, re.M), name
    assert "#define SK_RECUR_SAMPLES_MAX 4096u" in hdr and native.SK_RECUR_SAMPLES_MAX == sk.SK_RECUR_SAMPLES_MAX == 4096
    assert "#define SK_RECUR_PAIRS_MAX    256u" in hdr and native.SK_RECUR_PAIRS_MAX == sk.SK_RECUR_PAIRS_MAX == 256
    assert HIST_HEADER.decode().rstrip("\n").replace("\t", "<TAB>") in hdr
    assert PAIRS_HEADER.decode().rstrip("\n").replace("\t", "<TAB>") in hdr
    for attr in ("mark_bits", "finish"):
        assert hasattr(sk.Recurrence, attr)
    assert hasattr(sk.CoverageAcc, "set_recurrence") and hasattr(sk.CoverageAcc, "mark_target")
    assert hasattr(sk.KmerContext, "distinct_recurrence")


def test_the_model_on_a_hand_written_case():
    planes = np.array([[1, 1, 0, 0, 1, 0],
                       [1, 0, 0, 1, 1, 0],
                       [1, 0, 0, 0, 0, 0]], dtype=bool)
    hist, shared = recurrence(planes)
    assert hist.tolist() == [2, 2, 1, 1]
    assert shared.tolist() == [[3, 2, 1], [2, 3, 1], [1, 1, 1]]
    check_tables(hist, shared, 6)
    hist, shared = recurrence(np.zeros((2, 0), dtype=bool))
    assert hist.tolist() == [0, 0, 0] and shared.tolist() == [[0, 0], [0, 0]]
    assert recurrence(planes, pairs=False)[1] is None
    text = (b"d/m1\t1\t1\t1\t0\tAAAC\nm1\t1\t1\t1\t0\tAAAC\nm1\t2\t1\t0\t0\tAAAG\nm1\t1\t1\t0\t0\tAAAT\nm2\t3\t1\t0\t0\tAAAC\n"
            b"m2\t3\t1\t0\t0\tAAAT\n#m1\ttotal_kmer_evaluated\t9\n#m1\ttotal_genome_informative_kmers\t7\n#m3\ttotal_kmer_evaluated\t9\n"
            b"#m3\ttotal_genome_informative_kmers\t7  \n")
    h, p = tables_from_hits(text, "x/a_b.kmer_hits.gz", 1)      # m1 sees AAAC, AAAG (AAAT fails the filter); m2 AAAC, AAAT; m3 nothing
    assert h == HIST_HEADER + b"a_b\t3\t0\t4\na_b\t3\t1\t2\na_b\t3\t2\t1\n"
    assert p == PAIRS_HEADER + (b"a_b\tm1\tm1\t2\t2\na_b\tm1\tm2\t1\t3\na_b\tm1\tm3\t0\t2\na_b\tm2\tm2\t2\t2\na_b\tm2\tm3\t0\t2\n"
                                b"a_b\tm3\tm3\t0\t0\n")


# ---------------------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [["--coverage-recurrence"], ["--coverage-recurrence=r.tsv"], ["--coverage-recurrence", "--recurrence-pairs"],
                                   ["--coverage-recurrence", "--recurrence-pairs=p.tsv"]])
def test_the_flags_alone_are_refused(tmp_path, flags):
    before = _job(tmp_path)
    p = _run(ONE + flags, str(tmp_path))
    _refused(p, before, tmp_path)
    assert b"--coverage-recurrence goes with --coverage-depth or --coverage-only" in p.stderr


@pytest.mark.parametrize("table", ["--coverage-depth", "--coverage-only"])
@pytest.mark.parametrize("pairs", [["--recurrence-pairs"], ["--recurrence-pairs=p.tsv"]])
def test_pairs_without_the_histogram_are_refused(tmp_path, table, pairs):
    before = _job(tmp_path)
    p = _run(ONE + [table] + pairs, str(tmp_path))
    _refused(p, before, tmp_path)
    assert b"--recurrence-pairs goes with --coverage-recurrence" in p.stderr


@pytest.mark.parametrize("table", ["--coverage-depth", "--coverage-only"])
@pytest.mark.parametrize("flags", [["--coverage-recurrence=x"], ["--coverage-recurrence", "--recurrence-pairs=y"]])
def test_a_file_name_with_several_strains_is_refused(tmp_path, table, flags):
    before = _job(tmp_path)
    p = _run(["-S", "S.txt", "-B", "T.txt", table] + flags, str(tmp_path))
    _refused(p, before, tmp_path)
    assert b"--coverage-recurrence=FILE names one file" in p.stderr


@pytest.mark.parametrize("table", ["--coverage-depth", "--coverage-only"])
@pytest.mark.parametrize("lines,flags,word", [(4097, ["--coverage-recurrence"], b"at most 4096"),
                                              (257, ["--coverage-recurrence", "--recurrence-pairs"], b"at most 256")])
def test_too_many_target_lines_are_refused(tmp_path, table, lines, flags, word):
    _job(tmp_path)
    (tmp_path / "T.txt").write_text("".join("SE\tt%d.fa\n" % i for i in range(lines)))      # (no such files: no target is opened)
    before = sorted(os.listdir(tmp_path))
    p = _run(ONE + [table] + flags, str(tmp_path))
    _refused(p, before, tmp_path)
    assert word in p.stderr and b"targets" in p.stderr


def test_behind_detect_with_several_strains(tmp_path):
    before = _job(tmp_path)
    (tmp_path / "A.txt").write_text("g.fa\n")
    before = sorted(before + ["A.txt"])
    front = ["-S", "S.txt", "-A", "A.txt", "-B", "A.txt", "--scrub", "0.01", "--detect", "-B", "T.txt"]
    p = _run(front + ["--coverage-only", "--coverage-recurrence=one.tsv"], str(tmp_path), exe=sk.cli_path())
    _refused(p, before, tmp_path)
    assert p.stderr.startswith(b"kmer_scrub_count: with -S, --coverage-recurrence takes no file name")
    p = _run(front + ["--coverage-only", "--coverage-recurrence", "--recurrence-pairs=two.tsv"], str(tmp_path), exe=sk.cli_path())
    _refused(p, before, tmp_path)
    assert p.stderr.startswith(b"kmer_scrub_count: with -S, --recurrence-pairs takes no file name")
    p = _run(front + ["--coverage-recurrence"], str(tmp_path), exe=sk.cli_path())
    _refused(p, before, tmp_path)
    assert p.stderr.startswith(b"kmer_scrub_count: --coverage-recurrence goes with --coverage-depth or --coverage-only")
    p = _run(front + ["--coverage-depth", "--recurrence-pairs"], str(tmp_path), exe=sk.cli_path())
    _refused(p, before, tmp_path)
    assert p.stderr.startswith(b"kmer_scrub_count: --recurrence-pairs goes with --coverage-recurrence")


def test_coverage_depth_refuses_pairs_alone_before_it_reads(tmp_path):
    before = sorted(os.listdir(tmp_path))
    p = _run(["-k", "missing.kmer_hits.gz", "--recurrence-pairs"], str(tmp_path), exe=COV)
    _refused(p, before, tmp_path)
    assert b"--recurrence-pairs goes with --recurrence" in p.stderr


def test_a_build_without_the_entry_points_refuses_the_flag(tmp_path):
    """strain_detect's host layer over the CPU double of the device calls has no recurrence engine: one line, nothing written"""
    from test_sanitizers import SD_SOURCES
    exe = str(tmp_path / "sd_host")
    subprocess.run(["gcc", "-O1", "-g"] + SD_SOURCES + ["-lz", "-lpthread", "-o", exe], check=True)
    job = tmp_path / "job"
    job.mkdir()
    before = _job(job)
    for table in ("--coverage-depth", "--coverage-only"):
        p = _run(ONE + [table, "--coverage-recurrence"], str(job), exe=exe)
        _refused(p, before, job)
        assert b"--coverage-recurrence: this build has no recurrence engine" in p.stderr


# ---------------------------------------------------------------------------------------------------------------------------------
# the host fold under ASan + UBSan, as a process
# ---------------------------------------------------------------------------------------------------------------------------------
def test_the_host_fold_against_a_brute_force_loop_under_sanitizers(tmp_path):
    exe = str(tmp_path / "recur_sanitize")
    subprocess.run(["gcc", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                    os.path.join(REPO, "tests", "native", "recur_sanitize.c"), os.path.join(REPO, "strainer2_amd", "csrc", "sk_host_cov.c"),
                    "-lz", "-o", exe], check=True)
    p = subprocess.run([exe], env=ENV, capture_output=True, timeout=120)
    assert (p.returncode, p.stdout, p.stderr) == (0, b"recur_sanitize: ok\n", b""), p.stderr.decode()[-3000:]
