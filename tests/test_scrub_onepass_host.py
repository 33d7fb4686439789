"""kmer_scrub_count -S over one decode of the lists for every resident union: the parts that need no device -- the new ABI
(header, export list, library symbols) and the two settings, which change nothing a run shows before it reaches the device."""
import os
import re
import subprocess

import pytest

import strainer2_amd as sk
from strainer2_amd import native

EXE = sk.cli_path()
NEW = ["sk_scan_pinned_many", "sk_scan_pinned_packed_many", "sk_device_memory", "skh_scan_list_many"]
JUNK = [{"SK_SCRUB_UNIONS": "0"}, {"SK_SCRUB_UNIONS": "-3", "SK_SCRUB_HBM_MB": "0"}, {"SK_SCRUB_UNIONS": "many", "SK_SCRUB_HBM_MB": "x"},
        {"SK_SCRUB_HBM_MB": "-1"}, {"SK_SCRUB_UNIONS": "", "SK_SCRUB_HBM_MB": ""}]


def _run(argv, cwd, env=None):
    e = {k: v for k, v in os.environ.items() if not k.startswith("SK_SCRUB_")}
    e.update(env or {})
    return subprocess.run([EXE] + argv, cwd=cwd, env=e, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)


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


@pytest.mark.parametrize("case", ["bad_line", "usage", "unwritable", "missing_genome", "detect_without_scrub"])
def test_settings_set_to_garbage_change_nothing_before_device_work(tmp_path, case):
    _job(tmp_path)
    argv = ["-S", "S.txt", "-A", "A.txt", "-B", "B.txt", "-p", "prog"]
    if case == "bad_line":
        (tmp_path / "S.txt").write_text("g.fa\tok.tsv\ng.fa\n")
    elif case == "usage":
        (tmp_path / "S.txt").write_text("g.fa\tok.tsv\n")
        argv = argv[:4]
    elif case == "unwritable":
        (tmp_path / "S.txt").write_text("g.fa\tok.tsv\ng.fa\tno_such_dir/o.tsv.gz\n")
    elif case == "missing_genome":
        (tmp_path / "S.txt").write_text("g.fa\tok.tsv\nmissing.fa\tm.tsv\n")
    else:
        (tmp_path / "S.txt").write_text("g.fa\tok.tsv\th.kmer_hits.gz\n")
        argv = argv + ["--detect", "-B", "B.txt"]
    want = _run(argv, str(tmp_path))
    assert want.returncode == 1
    for env in JUNK:
        got = _run(argv, str(tmp_path), env)
        assert (got.returncode, got.stdout, got.stderr) == (want.returncode, want.stdout, want.stderr), env
        assert not (tmp_path / "ok.tsv").exists()


def test_settings_set_to_garbage_reach_the_device_as_before(tmp_path):
    """a valid job: here (no device) it fails where the device is first asked for, with or without the settings; on a GPU
    machine it runs either way"""
    _job(tmp_path)
    (tmp_path / "S.txt").write_text("g.fa\tok.tsv\n")
    argv = ["-S", "S.txt", "-A", "A.txt", "-B", "B.txt"]
    want = _run(argv, str(tmp_path))
    for env in JUNK:
        got = _run(argv, str(tmp_path), env)
        assert got.returncode == want.returncode, env
        if want.returncode:
            assert got.stderr == want.stderr, env
