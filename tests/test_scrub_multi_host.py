"""kmer_scrub_count -S, the parts that need no device: the command line's dispatch, the strains file, the outfiles checked
before anything is opened on the device, and the ABI (header, export list, library symbols)."""
import os
import re
import subprocess

import pytest

import strainer2_amd as sk
from strainer2_amd import native

EXE = sk.cli_path()
NEW = ["sk_union_count_enable", "sk_union_context", "sk_union_counts_fold", "skh_kmer_scrub_count_multi_main"]


def _run(argv, cwd):
    return subprocess.run([EXE] + argv, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)


def _job(d):
    (d / "g.fa").write_bytes(b">g\n" + b"ACGTTGCAAGGCTTAACCGGTTAACCGTAGCTAGCTAGGCTA" * 20 + b"\n")
    (d / "A.txt").write_text("g.fa\n")
    (d / "B.txt").write_text("g.fa\n")


def test_new_entry_points_are_declared_listed_and_exported(repo):
    hdr = open(os.path.join(repo, "include", "strainer_kmer.h")).read()
    syms = subprocess.run(["nm", "-D", "--defined-only", sk.library_path()], capture_output=True, text=True).stdout
    for name in NEW:
        assert re.search(r"\b%s\(" % name, hdr), name
        assert name in native.ABI_SYMBOLS, name
        assert re.search(r"\bT %s$" % name, syms, re.M), name


def test_with_r_the_S_flag_is_what_it_was(tmp_path):
    """-S next to -r: usage for the unknown letter, then the single program's own check (no -A/-B here)"""
    _job(tmp_path)
    p = _run(["-S", "x.txt", "-r", "g.fa"], str(tmp_path))
    q = _run(["-Q", "x.txt", "-r", "g.fa"], str(tmp_path))
    assert p.returncode == q.returncode == 1
    assert p.stderr == q.stderr.replace(b"'Q'", b"'S'")
    assert b"-S <strains file" not in p.stderr


def test_S_with_scrub_is_refused(tmp_path):
    _job(tmp_path)
    (tmp_path / "S.txt").write_text("g.fa\tout.tsv\n")
    p = _run(["-S", "S.txt", "-A", "A.txt", "-B", "B.txt", "--scrub", "0.1"], str(tmp_path))
    assert p.returncode == 1
    assert p.stderr == b"kmer_scrub_count: -S does not go with --scrub/--detect (run the strains one by one for those)\n"
    assert not (tmp_path / "out.tsv").exists()


@pytest.mark.parametrize("line", ["g.fa", "g.fa\tout.tsv\textra"])
def test_bad_strains_line(tmp_path, line):
    _job(tmp_path)
    (tmp_path / "S.txt").write_text("# comment\n\ng.fa\tok.tsv\n" + line + "\n")
    p = _run(["-S", "S.txt", "-A", "A.txt", "-B", "B.txt"], str(tmp_path))
    assert p.returncode == 1
    assert p.stderr == b"kmer_scrub_count: S.txt: a line needs <reference genome> TAB <outfile>\n"
    assert not (tmp_path / "ok.tsv").exists() and not (tmp_path / "out.tsv").exists()


def test_S_without_lists_prints_usage(tmp_path):
    _job(tmp_path)
    (tmp_path / "S.txt").write_text("g.fa\tout.tsv\n")
    p = _run(["-S", "S.txt", "-A", "A.txt"], str(tmp_path))
    assert p.returncode == 1 and p.stderr.startswith(b"Usage: kmer_scrub_count -S <strains file")


def test_unwritable_outfile_is_refused_before_any_scan(tmp_path):
    _job(tmp_path)
    (tmp_path / "S.txt").write_text("g.fa\tfirst.tsv\ng.fa\tno_such_dir/out.tsv.gz\n")
    p = _run(["-S", "S.txt", "-A", "A.txt", "-B", "B.txt", "-p", "prog"], str(tmp_path))
    assert p.returncode == 1
    assert p.stderr == b"kmer_scrub_count: cannot write no_such_dir/out.tsv.gz\n"
    assert not (tmp_path / "first.tsv").exists() and not (tmp_path / "prog").exists()


def test_unreadable_genome_has_the_single_programs_text(tmp_path):
    """the key set is built (and fails) before any device context is asked for"""
    _job(tmp_path)
    (tmp_path / "S.txt").write_text("missing.fa\tm.tsv\n")
    p = _run(["-S", "S.txt", "-A", "A.txt", "-B", "B.txt"], str(tmp_path))
    q = _run(["-r", "missing.fa", "-A", "A.txt", "-B", "B.txt"], str(tmp_path))
    assert p.returncode == q.returncode == 1
    assert p.stderr == q.stderr == b"could not read file missing.fa GEN_hash_sequences_set_count_vec()\n"
    assert not (tmp_path / "m.tsv").exists()
