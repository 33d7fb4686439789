"""strain_detect --coverage-regions, the parts that need no device: the new ABI entries (header, export list, library symbols), the
command lines the flag refuses before anything is opened -- each with one line on stderr, a non-zero status and nothing written --
the region table of a strain file (native.regions_from_file) against a model (tests/_regions_model.py), and the record parser with and without
its name sink compiled in."""
import gzip
import os
import random
import re
import subprocess

import pytest

import _synth
from _regions_model import model_records, model_regions
import strainer2_amd as sk
from strainer2_amd import native

EXE = sk.cli_path("strain_detect")
NEW = ["skh_regions_from_file", "skh_regions_free", "sk_table_first_pos", "sk_covacc_set_regions", "sk_covacc_region_rows",
       "sk_covacc_finish_target_regions"]


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


ONE = ["-r", "g.fa", "-a", "inf.txt", "-B", "T.txt", "-o", "Genus_species_a.kmer_hits.gz"]


def test_new_entry_points_are_declared_listed_and_exported(repo):
    hdr = open(os.path.join(repo, "include", "strainer_kmer.h")).read()
    syms = subprocess.run(["nm", "-D", "--defined-only", sk.library_path()], capture_output=True, text=True).stdout
    for name in NEW:
        assert re.search(r"\b%s\(" % name, hdr), name
        assert name in native.ABI_SYMBOLS, name
        assert re.search(r"\bT %s$" % name, syms, re.M), name
    assert "a row's region is the one that holds the FIRST base of the row's first occurrence" in hdr
    assert hasattr(sk.CoverageAcc, "set_regions") and hasattr(sk.CoverageAcc, "region_rows") and hasattr(sk.CoverageAcc, "finish_target_regions")
    assert hasattr(sk.KmerContext, "first_pos")


@pytest.mark.parametrize("flags", [["--coverage-regions"], ["--coverage-regions=r.tsv"], ["--coverage-regions", "--region-window", "50"]])
def test_the_flag_alone_is_refused(tmp_path, flags):
    before = _job(tmp_path)
    p = _run(ONE + flags, str(tmp_path))
    _refused(p, before, tmp_path)
    assert b"--coverage-regions goes with --coverage-depth or --coverage-only" in p.stderr


@pytest.mark.parametrize("table", ["--coverage-depth", "--coverage-only"])
def test_a_file_name_with_several_strains_is_refused(tmp_path, table):
    before = _job(tmp_path)
    p = _run(["-S", "S.txt", "-B", "T.txt", table, "--coverage-regions=x"], str(tmp_path))
    _refused(p, before, tmp_path)
    assert b"--coverage-regions=FILE names one file" in p.stderr


@pytest.mark.parametrize("w", [["--region-window", "-1"], ["--region-window=-1"], ["--region-window", "12x"], ["--region-window", ""]])
def test_a_bad_window_is_refused(tmp_path, w):
    before = _job(tmp_path)
    p = _run(ONE + ["--coverage-only", "--coverage-regions"] + w, str(tmp_path))
    _refused(p, before, tmp_path)
    assert b"--region-window" in p.stderr and b"0 or more" in p.stderr


def test_a_window_without_the_flag_is_refused(tmp_path):
    before = _job(tmp_path)
    p = _run(ONE + ["--coverage-only", "--region-window", "10"], str(tmp_path))
    _refused(p, before, tmp_path)


@pytest.mark.parametrize("many", [False, True])
@pytest.mark.parametrize("table", ["--coverage-depth", "--coverage-only"])
def test_more_than_2_to_the_20_regions_are_refused(tmp_path, table, many):
    """2^20 + 1 bases at one base per region; one base fewer is not refused here (it goes on and fails for want of a device or
    succeeds: either way not with this line)"""
    rng = random.Random(5)
    big = _synth.rand_dna(rng, (1 << 20) + 1)
    before = _job(tmp_path)
    (tmp_path / "big.fa").write_bytes(b">a\n" + big[:600000] + b"\n>short\nACGT\n>b\n" + big[600000:] + b"\n")
    (tmp_path / "S2.txt").write_text("g.fa\tinf.txt\tGenus_species_a.kmer_hits.gz\nbig.fa\tinf.txt\tGenus_species_b.kmer_hits.gz\n")
    before = sorted(before + ["big.fa", "S2.txt"])
    argv = ["-S", "S2.txt", "-B", "T.txt"] if many else ["-r", "big.fa"] + ONE[2:]
    p = _run(argv + [table, "--coverage-regions", "--region-window", "1"], str(tmp_path))
    _refused(p, before, tmp_path)
    assert b"more than 1048576 regions" in p.stderr and b"big.fa" in p.stderr
    with pytest.raises(sk.SKError):
        native.regions_from_file(str(tmp_path / "big.fa"), 1)
    regs, n = native.regions_from_file(str(tmp_path / "big.fa"), 2)
    assert n == (1 << 20) + 1 and len(regs) == 300000 + (448577 + 1) // 2 and regs[-1][1] == 3


# ---------------------------------------------------------------------------------------------------------------------------------
# the region table against a model
# ---------------------------------------------------------------------------------------------------------------------------------
def _wrap(seq, n):
    return b"\n".join(seq[i:i + n] for i in range(0, len(seq), n))


@pytest.fixture(scope="module")
def crafted():
    rng = random.Random(77)
    d = _synth.rand_dna
    W = 64
    lens = [29, 30, 31, W - 1, W, W + 1, 2 * W + 5, 5, 200]
    fa = b"".join(b">rec%d some comment %d\tmore\n%s\n" % (i, i, d(rng, n)) for i, n in enumerate(lens))
    multi = b"".join(b">m%d\n%s\n" % (i, _wrap(d(rng, n), 17)) for i, n in enumerate([2 * W + 5, 29, W, 31, 3 * W]))
    fq = b""
    for i, n in enumerate([W + 1, 29, 30, 2 * W + 5, W - 1]):
        s = d(rng, n)
        fq += b"@q%d/1 lane=3\n%s\n+q%d\n@%s\n" % (i, s, i, bytes(rng.choice(b"@>+IF#") for _ in range(n - 1)))
    odd = b"> spaced name\n" + d(rng, 40) + b"\n>\n" + d(rng, 33) + b"\n>crlf x\r\n" + d(rng, 70) + b"\r\n"
    return {"fa": fa, "multi": multi, "fq": fq, "odd": odd}, W


@pytest.mark.parametrize("name", ["fa", "multi", "fq", "odd"])
@pytest.mark.parametrize("gz", [False, True])
@pytest.mark.parametrize("w", ["0", "W", "1", "100000"])
def test_regions_from_file_against_the_model(tmp_path, crafted, name, gz, w):
    texts, W = crafted
    w = W if w == "W" else int(w)
    p = tmp_path / (name + (".gz" if gz else ".txt"))
    p.write_bytes(gzip.compress(texts[name]) if gz else texts[name])
    recs = model_records(texts[name])
    if name == "fq":
        assert all(not n.startswith(b"I") for n, _ in recs) and len(recs) == 5         # (no quality line was taken for a header)
    want, n = model_regions(recs, w)
    got, gn = native.regions_from_file(str(p), w)
    assert (got, gn) == (want, n)
    assert len(want) > 0 and (w != W or name == "odd" or any(r[3] == 5 for r in want))  # (the 2W + 5 record's last window)


def test_regions_of_a_file_without_a_kept_record(tmp_path):
    (tmp_path / "s.fa").write_bytes(b">a\nACGT\n>b\n" + b"A" * 29 + b"\n")
    assert native.regions_from_file(str(tmp_path / "s.fa"), 10) == ([], 0)
    with pytest.raises(sk.SKError):
        native.regions_from_file(str(tmp_path / "missing.fa"), 10)


def test_the_parser_with_and_without_the_name_sink(tmp_path, repo, crafted):
    """three builds of tests/native/parser_names_main.c on a reads file (FASTQ whose quality lines begin with @, wrapped FASTA,
    headers with comments, a truncated last record) and on the crafted strains, fed in blocks of 7 bytes and of 64 KiB: the same
    records and the same ending; the sink's names are the model's"""
    texts, _ = crafted
    rng = random.Random(3)
    reads = b""
    for i in range(300):
        s = _synth.rand_dna(rng, rng.choice([20, 31, 75, 150]))
        reads += b"@r%d x=%d\n%s\n+\n%s\n" % (i, i, s, bytes(rng.choice(b"@+>IF#") for _ in s))
    inputs = dict(texts, reads=reads, cut=reads[:-40], fa_reads=b"".join(b">f%d\n%s\n" % (i, _synth.rand_dna(rng, 60)) for i in range(200)))
    src = os.path.join(repo, "tests", "native", "parser_names_main.c")
    exes = {}
    for tag, defs in (("plain", []), ("compiled", ["-DSKP_NAME_SINK"]), ("sink", ["-DSKP_NAME_SINK", "-DUSE_SINK"])):
        exes[tag] = str(tmp_path / tag)
        subprocess.run(["gcc", "-O1", "-Wall", "-Wextra", "-Werror", "-Wno-unused-function"] + defs + [src, "-o", exes[tag]], check=True)
    for name, text in inputs.items():
        f = tmp_path / (name + ".in")
        f.write_bytes(text)
        outs = {}
        for tag, exe in exes.items():
            for bs in ("7", "65536"):
                p = subprocess.run([exe, str(f), bs], capture_output=True)
                assert p.returncode == 0
                outs[tag, bs] = p
        first = outs["plain", "65536"].stdout
        assert first.count(b"\n") > 3
        assert all(p.stdout == first for p in outs.values()), name
        assert all(outs[tag, bs].stderr == b"" for tag in ("plain", "compiled") for bs in ("7", "65536"))
        if name != "cut":
            names = b"".join(n + b"\n" for n, _ in model_records(text))
            assert outs["sink", "7"].stderr == names and outs["sink", "65536"].stderr == names, name
