"""kmer_scrub_count -S <strains> ... --scrub f [--independent] --detect <strain_detect args>: steps 1 to 4 of the workflow for
many strains in one job, the tables of step 1 kept on the device for steps 2 and 3 (skh_scrub_filter_resident per strain,
then skh_strain_detect_resident_many over all of them).  Every strain's informative list, hit list and coverage table must be
what the single-strain fused run (`-r <genome> ... --scrub f --detect ...`) writes, and for the bundled pair and a few random
worlds what the reference's chain of programs writes."""
import gzip
import hashlib
import json
import os
import random
import re
import shutil
import subprocess

import pytest

import _oracle
import _synth
import strainer2_amd as sk
from test_scrub_multi_gpu import _fasta, _mutate, _world      # the worlds of related strains that -S (step 1) is tested on

pytestmark = pytest.mark.gpu

EXE = sk.cli_path()
ORACLE_DIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle")


def _read(path):
    opener = gzip.open if str(path).endswith(".gz") else open
    with opener(path, "rb") as f:
        return f.read()


def _md5(path):
    return hashlib.md5(_read(path)).hexdigest()


def _run(argv, cwd=None, env=None, timeout=300):
    e = dict(os.environ)
    e.update(env or {})
    return subprocess.run([EXE] + argv, cwd=cwd, env=e, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout)


def _said(stderr):
    """stderr lines without the ones SK_TIMING=1 adds"""
    return sorted(l for l in stderr.decode().splitlines() if "timing" not in l and not l.startswith("key set of "))


def _cov_path(hits):
    return hits[: -len(".kmer_hits.gz")] + ".coverage_depth"


def _cov_rows(path=None, data=None):
    """a coverage table without its first three columns (strain, species and genus name: made from the hit list's name)"""
    return [l.split(b"\t", 3)[-1] for l in (_read(path) if data is None else data).split(b"\n")]


def _drug_list(d, genomes, seed):
    """-C: the genomes of _world's strains that are a random prefix + half of the base (pick 4), each named twice -- every
    strain keeps enough of its own k-mers for the filter's drug check, and those strains skip their own lines"""
    mine = [g for s, g in enumerate(genomes) if (s + seed) % 5 == 4]
    assert mine, "this world has no pick-4 strain"
    with open(os.path.join(d, "C.txt"), "w") as f:
        f.write("".join(g + "\n" for g in mine + mine[:1]))


def _write_strains(path, lines):
    with open(path, "w") as f:
        f.write("# genome\tinformative\thits\n\n")
        for l in lines:
            f.write("\t".join(l) + "\n")


# ---------------------------------------------------------------------------------------------------------------------
# 1. the bundled pair against the reference's chain (tests/golden/pair_workflow_facts.json)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def facts(golden):
    return json.load(open(os.path.join(golden, "pair_workflow_facts.json")))


def _bundled_copy(golden, facts, tmp_path):
    b = tmp_path / "bundled"
    b.mkdir()
    src = os.path.join(golden, "bundled")
    for n in ("strains", "metagenomes"):
        os.symlink(os.path.join(src, n), b / n)
    for n in ("genomes_to_scrub.txt", "metagenomes_to_scrub.txt", "target_metagenomes.txt"):
        shutil.copy(os.path.join(src, n), b / n)
    (b / facts["c_name"]).write_text("".join(l + "\n" for l in facts["c_list"]))
    return b


@pytest.mark.parametrize("case", ["plain", "drug", "independent"])
def test_bundled_pair_in_one_job_matches_the_reference_chain(golden, facts, tmp_path, case):
    b = _bundled_copy(golden, facts, tmp_path)
    c = facts["cases"][case]
    base = {n: str(tmp_path / os.path.basename(g)[: -len(".fna.gz")]) for n, g in facts["strains"].items()}   # (as test/example.sh
    out = {n: (base[n] + ".scrubbed_kmers" + (".gz" if n == "D4" else ""), base[n] + ".kmer_hits.gz") for n in base}  # names them)
    _write_strains(tmp_path / "S.txt", [(facts["strains"][n], out[n][0], out[n][1]) for n in facts["strains"]])
    argv = (["-S", str(tmp_path / "S.txt"), "-A", "genomes_to_scrub.txt", "-B", "metagenomes_to_scrub.txt"] + c["kmer_scrub_count"] +
            ["--scrub", facts["min_fraction"]] + (["--independent"] if c["kmer_scrub_filter"] else []) +
            ["--detect"] + facts["detect_args"] + ["--coverage-depth"])
    p = _run(argv, cwd=str(b))
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    assert p.stdout == b""
    with open(out["D4"][0], "rb") as f:
        assert f.read(2) == b"\x1f\x8b"                 # (a name ending in .gz is written gzip)
    for n, want in c["strains"].items():
        inf, hits = out[n]
        assert _md5(inf) == want["informative_md5"], (case, n)
        assert _md5(hits) == want["hits_md5"], (case, n)
        assert hashlib.md5(open(_cov_path(hits), "rb").read()).hexdigest() == want["coverage_md5"], (case, n)
    if case == "plain":                                 # the pins of the single-strain fused path's test
        assert _md5(out["B8"][0]) == "fe981fa571be70e602875ac3463ecdac"
        f3 = json.load(open(os.path.join(golden, "bundled", "step3_facts.json")))
        assert _md5(out["B8"][1]) == f3["hits_md5"]
        assert open(_cov_path(out["B8"][1]), "rb").read() == open(os.path.join(golden, "cov_cases", "bundled_step4", "expected.stdout"), "rb").read()


# ---------------------------------------------------------------------------------------------------------------------
# 2. random worlds against the single-strain fused run (and, for a few, the CPU oracle chain)
# ---------------------------------------------------------------------------------------------------------------------
def _genome_seq(path):
    return b"".join(l for l in _read(path).split(b"\n") if not l.startswith(b">"))


def _targets(d, genomes, seed):
    """target metagenomes: reads of the strains (SE, FASTQ, gzip) and a pair of mate files; T.txt lists them for -B"""
    rng = random.Random(seed * 7 + 1)
    seqs = [_genome_seq(os.path.join(d, g)) for g in genomes]
    lines = []
    for t in range(2):
        recs = b"".join(_synth.fuzz_stream(rng, rng.choice(seqs), 300, p_junk=0.01, min_len=0, max_len=200) for _ in range(2)).split(b"\n")[:-1]
        name = f"t{t}.fq" + (".gz" if t else "")
        body = b"".join(b"@r%d\n" % i + r.replace(b"\r", b"A") + b"\n+\n" + b"I" * len(r) + b"\n" for i, r in enumerate(recs))
        with (gzip.open if name.endswith(".gz") else open)(os.path.join(d, name), "wb") as f:
            f.write(body)
        lines.append(f"SE\t{name}")
    recs = _synth.fuzz_stream(rng, rng.choice(seqs), 400, p_junk=0.01, min_len=40, max_len=150).split(b"\n")[:-1]
    for m in (1, 2):
        with open(os.path.join(d, f"pe_{m}.fa"), "wb") as f:
            f.write(b"".join(b">p%d/%d\n" % (i, m) + (r if m == 1 else _synth.revcomp(r)).replace(b"\r", b"A") + b"\n" for i, r in enumerate(recs)))
    lines.append("PE\tpe_1.fa\tpe_2.fa")
    with open(os.path.join(d, "T.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


def _oracle_bin(name):
    p = os.path.join(ORACLE_DIR, name)
    if not os.path.exists(p):
        subprocess.run(["make", "-C", ORACLE_DIR, name], check=True, stdout=subprocess.DEVNULL)
    return p


def _oracle_chain(d, g, tail, fraction, scrub_extra, detect, i, cov=True):
    """kso -> ksf -> ksd -> kcd for one strain: (informative list, hits (decompressed), coverage table or None)"""
    t = _oracle.run_oracle_cli(["-r", g] + tail, cwd=d)
    assert t.returncode == 0, t.stderr
    with gzip.open(os.path.join(d, f"orc{i}.counts.gz"), "wb") as f:
        f.write(t.stdout)
    flt = subprocess.run([_oracle_bin("ksf_oracle"), "-s", f"orc{i}.counts.gz", "-m", fraction] + (["-i"] if scrub_extra else []),
                         cwd=d, capture_output=True)
    assert flt.returncode == 0, flt.stderr
    with open(os.path.join(d, f"orc{i}.inf"), "wb") as f:
        f.write(flt.stdout)
    hits = f"orc{i}.kmer_hits.gz"
    s = _oracle.run_sd_oracle_cli(["-r", g, "-a", f"orc{i}.inf"] + detect + ["-o", hits], cwd=d)
    assert s.returncode == 0, s.stderr
    if not cov:
        return flt.stdout, _read(os.path.join(d, hits)), None
    cov = subprocess.run([_oracle_bin("kcd_oracle"), "-k", hits], cwd=d, capture_output=True)
    assert cov.returncode == 0, cov.stderr
    return flt.stdout, _read(os.path.join(d, hits)), cov.stdout


def _fused(d, genomes, tail, detect, env=None, fraction="0.01", scrub_extra=(), strains_file="S.txt", prefix="f", cov=True):
    lines = [(g, f"{prefix}{i}.inf" + (".gz" if i % 3 == 1 else ""), f"{prefix}{i}.kmer_hits.gz") for i, g in enumerate(genomes)]
    _write_strains(os.path.join(d, strains_file), lines)
    argv = ["-S", strains_file] + tail + ["--scrub", fraction] + list(scrub_extra) + ["--detect"] + detect + (["--coverage-depth"] if cov else [])
    return _run(argv, cwd=d, env=env), lines


def _check_fused(d, genomes, tail, detect, env=None, fraction="0.01", scrub_extra=(), oracle=False, singles=None, cov=True):
    """the fused -S job against one single-strain fused run per strain (those of `singles`, default all): same files, and the
    same stderr lines as a multiset.  (strain_detect -S prints no line once per run that a single run prints per strain, for
    these worlds: the multisets are compared whole.)"""
    env = env or {}
    p, lines = _fused(d, genomes, tail, detect, env, fraction, scrub_extra, cov=cov)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    assert p.stdout == b""
    single_env = {k: v for k, v in env.items() if k not in ("SK_TIMING", "SK_SCRUB_GROUP", "SK_SD_GROUP")}
    want_err = []
    for i, g in enumerate(genomes):
        if singles is not None and i not in singles:
            continue
        inf, hits = f"one{i}.inf", f"one{i}.kmer_hits.gz"
        one = _run(["-r", g] + tail + ["--scrub", fraction] + list(scrub_extra) + ["--scrub-out", inf, "--detect"] + detect +
                   ["-o", hits] + (["--coverage-depth"] if cov else []), cwd=d, env=single_env)
        assert one.returncode == 0, one.stderr.decode()[-3000:]
        assert one.stdout == b""
        got = (_read(os.path.join(d, lines[i][1])), _read(os.path.join(d, lines[i][2])), _cov_rows(os.path.join(d, _cov_path(lines[i][2]))) if cov else None)
        want = (_read(os.path.join(d, inf)), _read(os.path.join(d, hits)), _cov_rows(os.path.join(d, _cov_path(hits))) if cov else None)
        assert got[0] == want[0], (i, g, "informative")
        assert got[1] == want[1], (i, g, "hits")
        assert got[2] == want[2], (i, g, "coverage")
        want_err += one.stderr.decode().splitlines()
        if oracle:
            o = _oracle_chain(d, g, tail, fraction, scrub_extra, detect, i, cov)
            assert o[:2] == want[:2], (i, g)
            assert o[2] is None or _cov_rows(data=o[2]) == want[2], (i, g)
    if singles is None:
        assert _said(p.stderr) == sorted(want_err)
    return p, lines


@pytest.mark.parametrize("seed", [1, 2, 3, 4])
def test_random_world_equals_single_fused_runs(seed, tmp_path):
    d = str(tmp_path)
    genomes, tail = _world(seed, d, nstrains=5)
    _drug_list(d, genomes, seed)
    genomes = genomes + [genomes[0]]                    # a line twice
    _targets(d, genomes, seed)
    _check_fused(d, genomes, tail, ["-B", "T.txt"], oracle=seed <= 2)


def test_groups_in_both_steps(tmp_path):
    d = str(tmp_path)
    genomes, tail = _world(21, d, nstrains=5)
    _drug_list(d, genomes, 21)
    _targets(d, genomes, 21)
    p, _ = _check_fused(d, genomes, tail, ["-B", "T.txt"], env={"SK_SCRUB_GROUP": "2", "SK_SD_GROUP": "2", "SK_TIMING": "1"})
    assert re.search(rb"5 strain\(s\) opened .* 3 union pass\(es\) \+ 0 single pass\(es\)", p.stderr)


def test_34_strains_make_two_unions(tmp_path):
    """two unions of default size in step 1 (and in step 3): every strain as the member-by-member way gives it; the strains
    at the unions' edges as their single fused runs give them"""
    d = str(tmp_path)
    rng = random.Random(34)
    base = _synth.rand_dna(rng, 3000)
    genomes = []
    for s in range(34):
        g = _mutate(rng, base, 0.01) if s % 2 else _synth.rand_dna(rng, 800) + base[:1500]
        (tmp_path / f"g{s}.fa").write_bytes(_fasta(g))
        genomes.append(f"g{s}.fa")
    (tmp_path / "m.fa").write_bytes(b"".join(b">r\n" + r + b"\n" for r in _synth.fuzz_stream(rng, base, 3000, p_junk=0.01).split(b"\n")[:-1]))
    (tmp_path / "A.txt").write_text("g0.fa\n")
    (tmp_path / "B.txt").write_text("m.fa\n")
    (tmp_path / "C.txt").write_text("g3.fa\nm.fa\ng20.fa\n")
    tail = ["-A", "A.txt", "-B", "B.txt", "-C", "C.txt"]
    _targets(d, genomes[:4], 34)
    p, lines = _check_fused(d, genomes, tail, ["-B", "T.txt"], env={"SK_TIMING": "1"}, singles={0, 31, 32, 33})
    assert re.search(rb"34 strain\(s\) opened .* 2 union pass\(es\) \+ 0 single pass\(es\)", p.stderr)
    q, qlines = _fused(d, genomes, tail, ["-B", "T.txt"], env={"SK_SCRUB_NO_UNION": "1", "SK_SD_NO_UNION": "1"}, strains_file="S2.txt", prefix="n")
    assert q.returncode == 0, q.stderr.decode()[-2000:]
    assert _said(q.stderr) == _said(p.stderr)
    for a, b in zip(lines, qlines):
        assert _read(os.path.join(d, a[1])) == _read(os.path.join(d, b[1])), a
        assert _read(os.path.join(d, a[2])) == _read(os.path.join(d, b[2])), a
        assert _cov_rows(os.path.join(d, _cov_path(a[2]))) == _cov_rows(os.path.join(d, _cov_path(b[2]))), a


def test_iupac_strain_among_union_members(tmp_path):
    d = str(tmp_path)
    genomes, tail = _world(33, d, nstrains=4, iupac=True)
    _drug_list(d, genomes, 33)
    _targets(d, genomes, 33)
    p, _ = _check_fused(d, genomes, tail, ["-B", "T.txt"], env={"SK_TIMING": "1"})
    assert re.search(rb"1 union pass\(es\) \+ 1 single pass\(es\)", p.stderr)


def test_paired_end_targets(tmp_path):
    d = str(tmp_path)
    genomes, tail = _world(7, d, nstrains=3)
    _drug_list(d, genomes, 7)
    _targets(d, genomes, 7)
    _check_fused(d, genomes, tail, ["-b", "pe_1.fa", "-c", "pe_2.fa", "-t", "PE"])


def test_independent(tmp_path):
    d = str(tmp_path)
    genomes, tail = _world(8, d, nstrains=4)
    _drug_list(d, genomes, 8)
    _targets(d, genomes, 8)
    _check_fused(d, genomes, tail, ["-B", "T.txt"], scrub_extra=["--independent"], oracle=True)


def test_a_strain_with_no_informative_kmers_left(tmp_path):
    """a copy of strain 0's genome under another name, and -C naming strain 0: every k-mer of the copy is a drug k-mer (strain 0
    skips its own line), so with --scrub 0 (no drug check) the copy's list holds its comment lines only.  (No --coverage-depth:
    coverage_depth.py divides by the number of informative k-mers.)"""
    d = str(tmp_path)
    genomes, tail = _world(7, d, nstrains=3)
    shutil.copy(os.path.join(d, genomes[0]), os.path.join(d, "copy_" + genomes[0]))
    genomes.append("copy_" + genomes[0])
    with open(os.path.join(d, "C.txt"), "w") as f:
        f.write(genomes[0] + "\n")
    _targets(d, genomes, 7)
    _, lines = _check_fused(d, genomes, tail, ["-B", "T.txt"], fraction="0", oracle=True, cov=False)
    empty = _read(os.path.join(d, lines[-1][1]))
    assert empty.startswith(b"#") and all(l.startswith(b"#") for l in empty.splitlines()), empty[-300:]
    assert any(not l.startswith(b"#") for l in _read(os.path.join(d, lines[0][1])).splitlines())


# ---------------------------------------------------------------------------------------------------------------------
# 3. ranks, failure
# ---------------------------------------------------------------------------------------------------------------------
def test_two_ranks_deal_the_strains(tmp_path):
    d = str(tmp_path)
    genomes, tail = _world(50, d, nstrains=5)
    _drug_list(d, genomes, 50)
    _targets(d, genomes, 50)
    p, lines = _fused(d, genomes, tail, ["-B", "T.txt"], strains_file="S1.txt", prefix="one")
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    two = [(g, f"two{i}.inf", f"two{i}.kmer_hits.gz") for i, g in enumerate(genomes)]
    _write_strains(os.path.join(d, "S2.txt"), two)
    argv = ["-S", "S2.txt"] + tail + ["--scrub", "0.01", "--detect", "-B", "T.txt", "--coverage-depth"]
    procs = [subprocess.Popen([EXE] + argv, cwd=d, env={**os.environ, "WORLD_SIZE": "2", "RANK": str(r)},
                              stdout=subprocess.PIPE, stderr=subprocess.PIPE) for r in range(2)]
    outs = [q.communicate(timeout=240) for q in procs]
    assert [q.returncode for q in procs] == [0, 0], outs
    for a, b in zip(lines, two):
        assert _read(os.path.join(d, a[1])) == _read(os.path.join(d, b[1])), b
        assert _read(os.path.join(d, a[2])) == _read(os.path.join(d, b[2])), b
        assert _cov_rows(os.path.join(d, _cov_path(a[2]))) == _cov_rows(os.path.join(d, _cov_path(b[2]))), b


def test_unreadable_target_fails_and_leaves_no_outfiles(tmp_path):
    d = str(tmp_path)
    genomes, tail = _world(42, d, nstrains=3)
    _drug_list(d, genomes, 42)
    _targets(d, genomes, 42)
    with open(os.path.join(d, "T.txt"), "a") as f:
        f.write("SE\tno_such_target.fq\n")
    before = set(os.listdir(d))
    p, lines = _fused(d, genomes, tail, ["-B", "T.txt"])
    assert p.returncode != 0
    assert set(os.listdir(d)) == before | {"S.txt"}, sorted(set(os.listdir(d)) - before)
