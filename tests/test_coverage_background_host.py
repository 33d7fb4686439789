"""The background of step 4's numbers without a GPU (include/strainer_kmer.h has the rule): the pure-Python model
(tests/_background_model.py) against the project's CPU oracle for COUNT, the invariants of a block, the host's table writer
(strainer2_amd/csrc/sk_host_background.c) driven by tests/native/background_check.c under AddressSanitizer + UBSan against the model's
two tables, the declarations, and the refusals strain_detect makes before it needs a device."""
import os
import random
import re
import subprocess

import numpy as np
import pytest

import _background_model as model
import _oracle
import _synth
import strainer2_amd as sk
from strainer2_amd import native

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = sk.cli_path("strain_detect")
SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")


def _world(seed):
    """a strain of two records (one partly lower case, an N, an IUPAC letter) and reads over it: lower case, an N, an R, the other
    strand, a read of 30 bases, one of exactly 31, unrelated reads"""
    rng = random.Random(seed)
    g = bytearray(_synth.rand_dna(rng, 700))
    g[100] = ord("N")
    g[300] = ord("R")
    strain = [bytes(g[:400]), bytes(g[400:]).lower()]
    reads = []
    for _ in range(120):
        ln = rng.choice([30, 31, 32, 47, 100, 150])
        a = rng.randrange(len(g) - ln)
        r = bytes(g[a:a + ln])
        pick = rng.random()
        if pick < 0.2:
            r = r.lower()
        elif pick < 0.4:
            r = r.translate(bytes.maketrans(b"ACGTRN", b"TGCAYN"))[::-1]
        elif pick < 0.5:
            r = r[:ln // 2] + b"N" + r[ln // 2 + 1:]
        elif pick < 0.6:
            r = _synth.rand_dna(rng, ln)
        reads.append(r)
    reads.append(bytes(g[290:320]))          # 30 bases around the R: no window
    reads.append(bytes(g[285:316]))          # 31 bases with the R: one window, a byte-string key
    return strain, reads


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_the_models_row_counts_are_the_oracles(seed):
    strain, reads = _world(seed)
    keys = model.strain_keys(strain)
    counts = model.row_counts(keys, reads)
    t = _oracle.OracleTable()
    assert t.build_stream(b"\n".join(strain) + b"\n", default=1, incr=0) == 0
    t.scan_stream(b"\n".join(reads) + b"\n", 2)
    okeys, ocounts = t.rows()
    t.close()
    assert sorted(okeys) == sorted(keys) and len(set(keys)) == len(keys)
    want = dict(zip(okeys, (int(x) for x in ocounts[:, 2])))
    assert {k: int(c) for k, c in zip(keys, counts)} == want
    assert any(b"R" in k or b"Y" in k for k in keys) and int(counts.sum()) > 500
    assert all(b"N" not in k for k in keys)
    with_r = [int(c) for k, c in zip(keys, counts) if b"R" in k or b"Y" in k]
    assert max(with_r) >= 1, "the read of 31 bases over the R counts on a byte-string key"


def test_a_read_shorter_than_k_has_no_window():
    strain, _ = _world(5)
    keys = model.strain_keys(strain)
    assert int(model.row_counts(keys, [strain[0][:30], strain[0][5:35].lower(), b""]).sum()) == 0
    assert int(model.row_counts(keys, [strain[0][:31]]).sum()) == 1


@pytest.mark.parametrize("D", [1, 2, 63, 255])
def test_block_invariants_and_edges(D):
    rng = np.random.default_rng(D)
    n = 5000
    counts = rng.poisson(3.0, n).astype(np.uint64)
    counts[:7] = [D - 1, D, D + 1, 70000, 2**32 - 1, 0, 1]
    inf = rng.random(n) < 0.02
    inf[:7] = [True, False, True, False, True, True, False]
    b = model.block(counts, inf, D)
    model.check_block(b)
    assert int(b[0, 0]) + int(b[1, 0]) == n, "informative + background kmers == table rows"
    assert int(b[0, 0]) == int(inf.sum())
    assert int(b[0, 2]) + int(b[1, 2]) == sum(int(x) for x in counts)
    assert int(b[0, 4]) >= 2**32 - 1 and int(b[1, 4]) >= 70000
    for flags in (np.zeros(n, bool), np.ones(n, bool)):
        e = model.block(counts, flags, D)
        model.check_block(e)
        assert int(e[0 if flags.all() else 1, 0]) == n and not e[1 if flags.all() else 0].any()
    z = model.block(np.zeros(n, np.uint64), inf, D)
    assert int(z[0, model.HEAD]) == int(inf.sum()) and not z[:, 1:model.HEAD].any()


def test_entry_points_are_declared():
    hdr = open(os.path.join(REPO, "include", "strainer_kmer.h")).read()
    syms = subprocess.run(["nm", "-D", "--defined-only", sk.library_path()], capture_output=True, text=True).stdout
    for name in ("sk_scan_batch", "sk_background_finish", "sk_union_background_finish"):
        assert re.search(r"\b%s\(" % name, hdr), name
        assert name in native.ABI_SYMBOLS, name
        assert re.search(r"\b%s\b" % name, syms), name
    assert "may be refilled only after the scan is done" in hdr
    assert native.SK_BACKGROUND_MAX_DEPTH == 255 and native.SK_BACKGROUND_HEAD == model.HEAD
    for m in ("scan_batch", "background_finish"):
        assert hasattr(sk.KmerContext, m) and hasattr(sk.KmerUnion, m)


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("bg") / "background_check")
    subprocess.run(["gcc"] + SAN + [os.path.join(REPO, "tests", "native", "background_check.c"), "-o", exe], check=True)
    return exe


@pytest.mark.parametrize("D,ntargets", [(1, 1), (63, 9), (255, 3), (7, 0)])
def test_the_table_writer_under_sanitizers_against_the_model(checker, tmp_path, D, ntargets):
    rng = np.random.default_rng(100 + D)
    blocks, script = [], ["D %d strainA" % D]
    for t in range(ntargets):
        counts = rng.poisson(2.0, 3000).astype(np.uint64)
        counts[:3] = [D + 1, 2**32 - 1, 2**32 - 1]
        b = model.block(counts, rng.random(3000) < 0.05, D)
        name = "meta_%d.fq.gz" % t
        blocks.append((name, b))
        script.append("T /some/dir/%s %s" % (name, " ".join(str(int(x)) for x in b.ravel())))
    (tmp_path / "script").write_text("\n".join(script) + "\n")
    p = subprocess.run([checker, str(tmp_path / "script"), str(tmp_path / "t"), str(tmp_path / "s")], env=ENV, capture_output=True)
    assert b"runtime error" not in p.stderr and b"AddressSanitizer" not in p.stderr and b"LeakSanitizer" not in p.stderr, p.stderr.decode()[-2000:]
    assert p.returncode == 0 and p.stdout == b"%d\n" % ntargets, (p.returncode, p.stderr.decode()[-1000:])
    traw, sraw = (tmp_path / "t").read_bytes(), (tmp_path / "s").read_bytes()
    assert traw == model.table("strainA", blocks)
    assert sraw == model.spectrum("strainA", blocks)
    t, order = model.blocks_of_tables(traw, sraw)
    assert [m for _, m, c in order if c == "informative"] == [m for m, _ in blocks], "targets in run order"
    sp = model.parse_spectrum(sraw)
    for name, b in blocks:
        for c, cls in enumerate(model.CLASSES):
            assert sp[("strainA", name, cls)] == [int(x) for x in b[c]]
            assert t[("strainA", name, cls)] == tuple(int(x) for x in b[c, :3])


def _job(d):
    rng = random.Random(9)
    g = _synth.rand_dna(rng, 600)
    (d / "g.fna").write_bytes(b">g\n" + g + b"\n")
    (d / "a.txt").write_bytes(g[10:41] + b"\n")
    os.makedirs(d / "x", exist_ok=True)
    os.makedirs(d / "y", exist_ok=True)
    for sub in ("x", "y"):
        (d / sub / "same.fa").write_bytes(b">r\n" + g[:100] + b"\n")
    (d / "B.txt").write_text("SE\tx/same.fa\nSE\ty/same.fa\n")
    (d / "S.txt").write_text("g.fna\ta.txt\ts1.kmer_hits.gz\ng.fna\ta.txt\ts2.kmer_hits.gz\n")
    return sorted(os.listdir(d))


BASE = ["-r", "g.fna", "-a", "a.txt", "-o", "o.kmer_hits.gz", "-n", "-b", "x/same.fa"]
REFUSALS = [
    ("max_256", BASE + ["--coverage-only", "--coverage-background", "--background-max", "256"], b"--background-max 256: a depth from 1 to 255"),
    ("max_0", BASE + ["--coverage-only", "--coverage-background", "--background-max=0"], b"--background-max 0: a depth from 1 to 255"),
    ("spectrum_alone", BASE + ["--coverage-only", "--background-spectrum"], b"--background-spectrum goes with --coverage-background"),
    ("max_alone", BASE + ["--coverage-depth", "--background-max", "9"], b"--background-max goes with --coverage-background"),
    ("no_table", BASE + ["--coverage-background"], b"--coverage-background goes with --coverage-depth or --coverage-only"),
    ("file_several", ["-S", "S.txt", "-n", "-b", "x/same.fa", "--coverage-only", "--coverage-background=one.tsv"],
     b"--coverage-background=FILE names one file"),
    ("same_basename", ["-r", "g.fna", "-a", "a.txt", "-o", "o.kmer_hits.gz", "-B", "B.txt", "--coverage-depth", "--coverage-background"],
     b"two targets of B.txt share a file name"),
]


@pytest.mark.parametrize("case", REFUSALS, ids=[c[0] for c in REFUSALS])
def test_refusals_come_before_anything_is_read_or_written(tmp_path, case):
    """each gives its one line and a non-zero exit and leaves the directory as it was; none needs a device"""
    _, argv, words = case
    before = _job(tmp_path)
    clean = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "SK_WORLD_SIZE", "SK_SD_NO_UNION", "RANK")}
    p = subprocess.run([EXE] + argv, cwd=tmp_path, capture_output=True, timeout=120, env=clean)
    assert p.returncode != 0 and p.stdout == b""
    assert p.stderr.count(b"\n") == 1 and p.stderr.endswith(b"\n") and words in p.stderr, p.stderr
    assert sorted(os.listdir(tmp_path)) == before


DETECT = ["--scrub", "0.5", "--detect", "-B", "B.txt", "--coverage-depth", "--coverage-background"]


@pytest.mark.parametrize("front", [["-r", "g.fna", "-A", "S.txt", "-B", "S.txt"], ["-S", "S.txt", "-A", "B.txt", "-B", "B.txt"]], ids=["one_strain", "many_strains"])
def test_the_flag_behind_detect_is_refused_before_anything_is_read(tmp_path, front):
    """kmer_scrub_count ... --detect, with -r and with -S (two checks in two files): one line, a non-zero exit, nothing read or written"""
    before = _job(tmp_path)
    clean = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "SK_WORLD_SIZE", "RANK")}
    p = subprocess.run([sk.cli_path("kmer_scrub_count")] + front + DETECT, cwd=tmp_path, capture_output=True, timeout=120, env=clean)
    assert p.returncode != 0 and p.stdout == b""
    assert p.stderr.count(b"\n") == 1 and b"--coverage-background does not go behind --detect" in p.stderr, p.stderr
    assert sorted(os.listdir(tmp_path)) == before
