"""strain_detect --coverage-only, the parts that need no device: the new ABI entries (header, export list, library symbols) and
the command lines the flag refuses before anything is opened -- each with one line on stderr, a non-zero status and nothing
written."""
import os
import re
import subprocess

import pytest

import strainer2_amd as sk
from strainer2_amd import native

EXE = sk.cli_path("strain_detect")
NEW = ["sk_covacc_create", "sk_covacc_destroy", "sk_covacc_hold", "sk_covacc_add", "sk_covacc_add_rows", "sk_covacc_finish_target",
       "sk_covacc_rows", "sk_covacc_pick", "sk_covacc_fetch_hold", "sk_tally_collect_counts", "sk_tally_fetch_held",
       "sk_union_tally_launch_ex", "sk_union_tally_collect_counts", "sk_union_tally_fetch_held", "skh_coverage_only_stats"]


def _job(d):
    (d / "g.fa").write_bytes(b">g\n" + b"ACGTTGCAAGGCTTAACCGGTTAACCGTAGCTAGCTAGGCTA" * 20 + b"\n")
    (d / "inf.txt").write_bytes(b"#informative\nACGTTGCAAGGCTTAACCGGTTAACCGTAGC\n")
    (d / "T.txt").write_text("SE\tg.fa\n")
    (d / "S.txt").write_text("g.fa\tinf.txt\tGenus_species_a.kmer_hits.gz\ng.fa\tinf.txt\tGenus_species_b.kmer_hits.gz\n")
    return sorted(os.listdir(d))


def _run(argv, cwd, exe=EXE):
    return subprocess.run([exe] + argv, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)


def _refused(p, before, d):
    assert p.returncode != 0
    assert p.stdout == b""
    assert p.stderr.count(b"\n") == 1 and p.stderr.endswith(b"\n"), p.stderr
    assert sorted(os.listdir(d)) == before


def test_new_entry_points_are_declared_listed_and_exported(repo):
    hdr = open(os.path.join(repo, "include", "strainer_kmer.h")).read()
    syms = subprocess.run(["nm", "-D", "--defined-only", sk.library_path()], capture_output=True, text=True).stdout
    for name in NEW:
        assert re.search(r"\b%s\(" % name, hdr), name
        assert name in native.ABI_SYMBOLS, name
        assert re.search(r"\bT %s$" % name, syms, re.M), name
    assert native.coverage_only_stats() == (0, 0, 0)


@pytest.mark.parametrize("order", [["--coverage-only", "--coverage-depth"], ["--coverage-depth=x.tsv", "--coverage-only"],
                                   ["--coverage-only=y.tsv", "--coverage-depth"]])
def test_both_tables_flags_are_refused(tmp_path, order):
    before = _job(tmp_path)
    p = _run(["-r", "g.fa", "-a", "inf.txt", "-B", "T.txt", "-o", "Genus_species_a.kmer_hits.gz"] + order, str(tmp_path))
    _refused(p, before, tmp_path)
    assert b"--coverage-only and --coverage-depth" in p.stderr


def test_a_file_name_with_several_strains_is_refused(tmp_path):
    before = _job(tmp_path)
    p = _run(["-S", "S.txt", "-B", "T.txt", "--coverage-only=one.tsv"], str(tmp_path))
    _refused(p, before, tmp_path)
    assert b"--coverage-only=FILE names one file" in p.stderr


def test_a_file_name_behind_detect_with_several_strains_is_refused(tmp_path):
    before = _job(tmp_path)
    (tmp_path / "A.txt").write_text("g.fa\n")
    before = sorted(before + ["A.txt"])
    p = _run(["-S", "S.txt", "-A", "A.txt", "-B", "A.txt", "--scrub", "0.01", "--detect", "-B", "T.txt", "--coverage-only=one.tsv"],
             str(tmp_path), exe=sk.cli_path())
    _refused(p, before, tmp_path)
    assert p.stderr.startswith(b"kmer_scrub_count: with -S, --coverage-only takes no file name")


def test_a_missing_o_is_refused(tmp_path):
    before = _job(tmp_path)
    p = _run(["-r", "g.fa", "-a", "inf.txt", "-B", "T.txt", "--coverage-only"], str(tmp_path))
    _refused(p, before, tmp_path)
    assert b"--coverage-only needs -o" in p.stderr


def test_both_flags_behind_detect_with_several_strains_are_refused(tmp_path):
    before = _job(tmp_path)
    (tmp_path / "A.txt").write_text("g.fa\n")
    before = sorted(before + ["A.txt"])
    for order in (["--coverage-only", "--coverage-depth"], ["--coverage-depth", "--coverage-only"]):
        p = _run(["-S", "S.txt", "-A", "A.txt", "-B", "A.txt", "--scrub", "0.01", "--detect", "-B", "T.txt"] + order, str(tmp_path),
                 exe=sk.cli_path())
        _refused(p, before, tmp_path)
        assert p.stderr.startswith(b"kmer_scrub_count: --coverage-only and --coverage-depth exclude each other")
