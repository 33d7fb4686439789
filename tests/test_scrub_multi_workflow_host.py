"""kmer_scrub_count -S --scrub .. --detect, the parts that need no device: the new ABI entry (header, export list, library
symbols), and every argument the fused many-strain workflow refuses before anything is opened on the device."""
import os
import re
import subprocess

import pytest

import strainer2_amd as sk
from strainer2_amd import native

EXE = sk.cli_path()
NEW = ["skh_strain_detect_resident_many"]
NO_DEVICE = b"kmer_scrub_count: cannot use HIP device"


def _run(argv, cwd, env=None):
    e = dict(os.environ)
    e.update(env or {})
    return subprocess.run([EXE] + argv, cwd=cwd, env=e, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)


def _job(d, strains):
    (d / "g.fa").write_bytes(b">g\n" + b"ACGTTGCAAGGCTTAACCGGTTAACCGTAGCTAGCTAGGCTA" * 20 + b"\n")
    (d / "A.txt").write_text("g.fa\n")
    (d / "B.txt").write_text("g.fa\n")
    (d / "T.txt").write_text("SE\tg.fa\n")
    (d / "S.txt").write_text("# genome\tinformative\thits\n\n" + "".join("\t".join(l) + "\n" for l in strains))


LISTS = ["-S", "S.txt", "-A", "A.txt", "-B", "B.txt"]
FUSED = LISTS + ["--scrub", "0.01", "--detect", "-B", "T.txt"]


def _nothing_written(d):
    assert sorted(os.listdir(d)) == ["A.txt", "B.txt", "S.txt", "T.txt", "g.fa"]


def test_new_entry_point_is_declared_listed_and_exported(repo):
    hdr = open(os.path.join(repo, "include", "strainer_kmer.h")).read()
    syms = subprocess.run(["nm", "-D", "--defined-only", sk.library_path()], capture_output=True, text=True).stdout
    for name in NEW:
        assert re.search(r"\b%s\(" % name, hdr), name
        assert name in native.ABI_SYMBOLS, name
        assert re.search(r"\bT %s$" % name, syms, re.M), name


@pytest.mark.parametrize("flag", ["-r", "-a", "-o", "-S", "-g"])
def test_strain_flags_after_detect_are_refused(tmp_path, flag):
    """each strain's line gives -r/-a/-o/-g; -S belongs to kmer_scrub_count -- the dispatch must not take -r as the single form"""
    _job(tmp_path, [("g.fa", "i.txt", "h.gz")])
    p = _run(FUSED + [flag, "x"], str(tmp_path))
    assert p.returncode == 1
    assert p.stderr == b"kmer_scrub_count: with -S, each strain's line gives strain_detect's %s (not after --detect)\n" % flag.encode()
    _nothing_written(tmp_path)


def test_flag_in_a_cluster_after_detect_is_refused(tmp_path):
    _job(tmp_path, [("g.fa", "i.txt", "h.gz")])
    p = _run(LISTS + ["--scrub", "0.01", "--detect", "-BT.txt", "-og.gz"], str(tmp_path))
    assert p.returncode == 1 and p.stderr.endswith(b"strain_detect's -o (not after --detect)\n")
    _nothing_written(tmp_path)


def test_coverage_depth_file_is_refused(tmp_path):
    _job(tmp_path, [("g.fa", "i.txt", "h.gz")])
    p = _run(FUSED + ["--coverage-depth=cov.txt"], str(tmp_path))
    assert p.returncode == 1
    assert p.stderr == b"kmer_scrub_count: with -S, --coverage-depth takes no file name (each strain's table goes next to its hit list)\n"
    _nothing_written(tmp_path)


def test_detect_without_scrub_has_the_single_strain_wording(tmp_path):
    _job(tmp_path, [("g.fa", "i.txt", "h.gz")])
    p = _run(LISTS + ["--detect", "-B", "T.txt"], str(tmp_path))
    q = _run(["-r", "g.fa", "-A", "A.txt", "-B", "B.txt", "--detect", "-B", "T.txt", "-o", "h.gz"], str(tmp_path))
    assert p.returncode == q.returncode == 1
    assert p.stderr == q.stderr == b"kmer_scrub_count: --detect needs --scrub <min_fraction> and a single process\n"
    _nothing_written(tmp_path)


def test_sk_devices_is_refused(tmp_path):
    _job(tmp_path, [("g.fa", "i.txt", "h.gz")])
    p = _run(FUSED, str(tmp_path), env={"SK_DEVICES": "2"})
    assert p.returncode == 1
    assert p.stderr == b"kmer_scrub_count: -S --detect keeps every strain on the device that counted it (SK_DEVICES is not for this run)\n"
    _nothing_written(tmp_path)


def test_scrub_out_is_refused(tmp_path):
    _job(tmp_path, [("g.fa", "i.txt", "h.gz")])
    p = _run(LISTS + ["--scrub", "0.01", "--scrub-out", "x.txt", "--detect", "-B", "T.txt"], str(tmp_path))
    assert p.returncode == 1
    assert p.stderr == b"kmer_scrub_count: with -S the strains file names each informative outfile (no --scrub-out)\n"
    _nothing_written(tmp_path)


def test_bad_fraction_is_refused(tmp_path):
    _job(tmp_path, [("g.fa", "i.txt", "h.gz")])
    p = _run(LISTS + ["--scrub", "1.5", "--detect", "-B", "T.txt"], str(tmp_path))
    assert p.returncode == 1 and p.stderr == b"kmer_scrub_count: --scrub needs a fraction between 0.0 and 1.0\n"
    _nothing_written(tmp_path)


@pytest.mark.parametrize("lines", [
    [("g.fa", "ok.txt", "ok.gz"), ("g.fa", "i.txt")],
    [("g.fa", "i.txt", "h.gz", "g.txt", "extra")],
    [("g.fa",)],
])
def test_strain_lines_need_three_or_four_columns(tmp_path, lines):
    _job(tmp_path, lines)
    p = _run(FUSED, str(tmp_path))
    assert p.returncode == 1
    assert p.stderr == (b"kmer_scrub_count: S.txt: a line needs <reference genome> TAB <informative outfile> TAB <hits outfile> "
                        b"[TAB <-g list>]\n")
    _nothing_written(tmp_path)


@pytest.mark.parametrize("words", [["--scrub", "0.01"], ["--scrub=0.01", "--independent"], ["--independent"]])
def test_scrub_without_detect_keeps_its_refusal(tmp_path, words):
    """the informative lists alone are not a -S job: the refusal -S always had, before any strain line is read"""
    _job(tmp_path, [("g.fa", "i.txt", "h.gz")])
    p = _run(LISTS + words, str(tmp_path))
    assert p.returncode == 1
    assert p.stderr == b"kmer_scrub_count: -S does not go with --scrub/--detect (run the strains one by one for those)\n"
    _nothing_written(tmp_path)


def test_unwritable_hits_outfile_is_refused_before_any_scan(tmp_path):
    _job(tmp_path, [("g.fa", "i.txt", "h.gz"), ("g.fa", "i2.txt.gz", "no_such_dir/h2.kmer_hits.gz")])
    p = _run(FUSED + ["--coverage-depth"], str(tmp_path))
    assert p.returncode == 1
    assert p.stderr == b"kmer_scrub_count: cannot write no_such_dir/h2.kmer_hits.gz\n"
    _nothing_written(tmp_path)


def _past_the_arguments(p):
    """a run that got past every argument check: on a machine without a device it stops at the context, with a device it
    succeeds"""
    if p.returncode == 0:
        return True
    return p.returncode == 1 and p.stderr.startswith(NO_DEVICE)


def test_plain_S_still_gets_past_the_arguments(tmp_path):
    """no --scrub: the strain lines are still <genome> TAB <counts outfile>, and the run goes on to the device"""
    _job(tmp_path, [("g.fa", "counts.tsv")])
    p = _run(LISTS, str(tmp_path))
    assert _past_the_arguments(p), p.stderr
    if p.returncode:
        _nothing_written(tmp_path)
    else:
        assert (tmp_path / "counts.tsv").read_bytes().startswith(b"#kmer\treference_count")


def test_fused_forms_get_past_the_arguments(tmp_path):
    _job(tmp_path, [("g.fa", "i.txt", "h.kmer_hits.gz")])
    assert _past_the_arguments(_run(LISTS + ["--scrub", "0.01", "--independent", "--detect", "-B", "T.txt"], str(tmp_path)))
    (tmp_path / "G.txt").write_text("g.fa\n")                  # (a -g list: one genome or metagenome file per line)
    (tmp_path / "S.txt").write_text("g.fa\ti.txt.gz\th.kmer_hits.gz\tG.txt\n")
    p = _run(FUSED + ["--coverage-depth", "--min-kmer-hits", "2"], str(tmp_path))
    assert _past_the_arguments(p), p.stderr
