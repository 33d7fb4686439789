"""kmer_scrub_count -S: many strains over ONE pass of the -A/-B/-C lists through a union table (sk_union_count_enable /
sk_union_counts_fold).  Every outfile must hold exactly the bytes `kmer_scrub_count -r <that strain>` prints: the bundled pair
against the unmodified reference's facts (tests/golden/step1_pair_facts.json), random worlds of related strains against the
single-strain program (and, for a few, the CPU oracle), the fallback for strains the union cannot hold, groups, ranks, errors."""
import gzip
import hashlib
import json
import os
import random
import re
import shutil
import subprocess

import numpy as np
import pytest

import _oracle
import _synth
import strainer2_amd as sk

pytestmark = pytest.mark.gpu

EXE = sk.cli_path()


def _md5_file(path):
    h, n = hashlib.md5(), 0
    opener = gzip.open if str(path).endswith(".gz") else open
    with opener(path, "rb") as f:
        for blk in iter(lambda: f.read(1 << 24), b""):
            h.update(blk)
            n += len(blk)
    return h.hexdigest(), n


def _read(path):
    opener = gzip.open if str(path).endswith(".gz") else open
    with opener(path, "rb") as f:
        return f.read()


def _run(argv, cwd=None, env=None, timeout=600):
    e = dict(os.environ)
    e.update(env or {})
    return subprocess.run([EXE] + argv, cwd=cwd, env=e, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout)


def _write_strains(path, pairs):
    with open(path, "w") as f:
        f.write("# genome\toutfile\n\n")
        for g, o in pairs:
            f.write(f"{g}\t{o}\n")


# ---------------------------------------------------------------------------------------------------------------------
# 1. the bundled pair against the reference
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pair_facts(golden):
    return json.load(open(os.path.join(golden, "step1_pair_facts.json")))


def test_bundled_pair_matches_reference(golden, pair_facts, tmp_path):
    b = os.path.join(golden, "bundled")
    st = tmp_path / "strains.txt"
    _write_strains(st, [(pair_facts["strains"]["B8"], tmp_path / "B8.tsv"), (pair_facts["strains"]["D4"], tmp_path / "D4.tsv")])
    p = _run(["-S", str(st), "-A", "genomes_to_scrub.txt", "-B", "metagenomes_to_scrub.txt", "-p", str(tmp_path / "prog")], cwd=b)
    assert p.returncode == 0, p.stderr
    assert p.stderr == b"" and p.stdout == b""
    for name in ("B8", "D4"):
        want = pair_facts["runs"][name]
        assert _md5_file(tmp_path / f"{name}.tsv") == (want["stdout_md5"], want["stdout_bytes"]), name
    assert _md5_file(tmp_path / "B8.tsv")[0] == "75989a9bc31ef0b6f53a5112a60920bd"
    prog = (tmp_path / "prog").read_text().splitlines()
    assert prog[0] == "adding kmer counts for:"
    assert [l.split("\t")[0] for l in prog[1:]] == [pair_facts["strains"]["D4"], "metagenomes/1001099B_150804_B6_s09_tiny_PE1.fasta.gz"]


def test_bundled_pair_with_drug_list_skips_each_strain_itself(golden, pair_facts, tmp_path):
    """-C names both strains (B8 twice): each strain skips only its own lines; one outfile is gzip"""
    b = tmp_path / "bundled"
    b.mkdir()
    src = os.path.join(golden, "bundled")
    for n in ("strains", "metagenomes"):
        os.symlink(os.path.join(src, n), b / n)
    for n in ("genomes_to_scrub.txt", "metagenomes_to_scrub.txt"):
        shutil.copy(os.path.join(src, n), b / n)
    (b / pair_facts["c_name"]).write_text("".join(l + "\n" for l in pair_facts["c_list"]))
    st = tmp_path / "strains.txt"
    _write_strains(st, [(pair_facts["strains"]["B8"], tmp_path / "B8.tsv"), (pair_facts["strains"]["D4"], tmp_path / "D4.tsv.gz")])
    p = _run(["-S", str(st), "-A", "genomes_to_scrub.txt", "-B", "metagenomes_to_scrub.txt", "-C", pair_facts["c_name"]], cwd=str(b))
    assert p.returncode == 0, p.stderr
    want_b8, want_d4 = pair_facts["runs"]["B8+C"], pair_facts["runs"]["D4+C"]
    assert _md5_file(tmp_path / "B8.tsv") == (want_b8["stdout_md5"], want_b8["stdout_bytes"])
    with open(tmp_path / "D4.tsv.gz", "rb") as f:
        assert f.read(2) == b"\x1f\x8b"
    assert _md5_file(tmp_path / "D4.tsv.gz") == (want_d4["stdout_md5"], want_d4["stdout_bytes"])
    # one line per (list line, strain) pair, in list order
    c = pair_facts["c_list"]
    assert p.stderr.decode() == "".join(f"skipping {l} (identical match)\n" for l in c)
    assert sorted(p.stderr.decode().splitlines()) == sorted((want_b8["stderr"] + want_d4["stderr"]).splitlines())


# ---------------------------------------------------------------------------------------------------------------------
# 2. random worlds of related strains against the single-strain program
# ---------------------------------------------------------------------------------------------------------------------
def _mutate(rng, seq, rate):
    b = bytearray(seq)
    for i in range(len(b)):
        if rng.random() < rate:
            b[i] = rng.choice(b"ACGT")
    return bytes(b)


def _fasta(seq, name=b"s", width=70):
    return b">" + name + b"\n" + b"".join(seq[i:i + width] + b"\n" for i in range(0, len(seq), width))


def _world(seed, d, nstrains=None, iupac=False):
    """2-7 related strains (copies, diverged copies, the other strand of a part, a repeated segment), -A/-B lists of fuzzed
    reads as FASTA/FASTQ, plain and gzip, and a -C list naming some strains' own genomes.  Returns (genome paths, argv tail)."""
    rng = random.Random(seed)
    base = _synth.rand_dna(rng, rng.choice([3000, 12000, 30000]))
    n = nstrains or rng.randint(2, 7)
    genomes, seqs = [], []
    for s in range(n):
        pick = (s + seed) % 5
        if pick == 0:
            g = base
        elif pick == 1:
            g = _mutate(rng, base, rng.choice([0.002, 0.01, 0.05]))
        elif pick == 2:
            g = _synth.revcomp(base[len(base) // 3:]) + _synth.rand_dna(rng, 500)
        elif pick == 3:
            cut = len(base) // 2
            g = base[:cut] + base[cut // 2:cut] + base[cut:]
        else:
            g = _synth.rand_dna(rng, 4000) + base[: len(base) // 2]
        if iupac and s == n - 1:
            g = bytearray(g)
            for i in range(5, len(g), 97):
                g[i] = rng.choice(b"RYKM")
            g = bytes(g)
        path = f"g{s}.fa" + (".gz" if s % 3 == 2 else "")
        data = _fasta(g, b"g%d" % s)
        with (gzip.open if path.endswith(".gz") else open)(os.path.join(d, path), "wb") as f:
            f.write(data)
        genomes.append(path)
        seqs.append(g)
    files = []
    for fi in range(4):
        src = rng.choice([base] + seqs)
        recs = _synth.fuzz_stream(rng, src, 400, p_junk=0.01, min_len=0, max_len=220).split(b"\n")[:-1]
        fastq = fi % 2 == 1
        body = bytearray()
        for i, r in enumerate(recs):
            r = r.replace(b"\r", b"A")
            if fastq:
                body += b"@r%d\n" % i + r + b"\n+\n" + b"I" * len(r) + b"\n"
            else:
                body += b">r%d\n" % i + r + b"\n"
        name = f"m{fi}.f" + ("q" if fastq else "a") + (".gz" if fi >= 2 else "")
        with (gzip.open if name.endswith(".gz") else open)(os.path.join(d, name), "wb") as f:
            f.write(bytes(body))
        files.append(name)
    with open(os.path.join(d, "A.txt"), "w") as f:
        f.write(files[0] + "\n" + genomes[0] + "\n")
    with open(os.path.join(d, "B.txt"), "w") as f:
        f.write("\n".join(files[1:]) + "\n")
    c_lines = [files[3]] + [genomes[i] for i in range(n) if i % 2 == 0] + [genomes[0]]
    with open(os.path.join(d, "C.txt"), "w") as f:
        f.write("\n".join(c_lines) + "\n")
    return genomes, ["-A", "A.txt", "-B", "B.txt", "-C", "C.txt"]


def _check_world(d, genomes, tail, env, gz_every=2, oracle=False):
    outs = [f"o{i}.tsv" + (".gz" if i % gz_every == 1 else "") for i in range(len(genomes))]
    _write_strains(os.path.join(d, "S.txt"), zip(genomes, outs))
    p = _run(["-S", "S.txt", "-p", "prog"] + tail, cwd=d, env=env)
    assert p.returncode == 0, p.stderr
    single_env = {k: v for k, v in env.items() if k != "SK_TIMING"}
    want_err = []
    for i, g in enumerate(genomes):
        one = _run(["-r", g] + tail, cwd=d, env=single_env)
        assert one.returncode == 0, one.stderr
        assert _read(os.path.join(d, outs[i])) == one.stdout, (g, env)
        want_err += one.stderr.decode().splitlines()
        if oracle:
            o = _oracle.run_oracle_cli(["-r", g] + tail, cwd=d)
            assert o.returncode == 0 and o.stdout == one.stdout, g
    said = [l for l in p.stderr.decode().splitlines() if "timing" not in l and not l.startswith("key set of ")]   # (SK_TIMING=1)
    assert sorted(said) == sorted(want_err)
    return p


@pytest.mark.parametrize("seed", list(range(1, 17)))
def test_random_world_equals_single_runs(seed, tmp_path):
    genomes, tail = _world(seed, str(tmp_path))
    for pack in ("0", "2"):
        _check_world(str(tmp_path), genomes, tail, {"SK_LIST_PACK": pack}, oracle=(seed <= 3 and pack == "0"))


def test_random_world_member_by_member_and_small_groups(tmp_path):
    genomes, tail = _world(21, str(tmp_path), nstrains=5)
    _check_world(str(tmp_path), genomes, tail, {"SK_SCRUB_NO_UNION": "1"})
    p = _check_world(str(tmp_path), genomes, tail, {"SK_SCRUB_GROUP": "2", "SK_TIMING": "1"})
    assert re.search(rb"3 union pass\(es\) \+ 0 single pass\(es\)", p.stderr)


# ---------------------------------------------------------------------------------------------------------------------
# 3. fallback and group size
# ---------------------------------------------------------------------------------------------------------------------
def test_iupac_strain_goes_through_its_own_pass(tmp_path):
    genomes, tail = _world(33, str(tmp_path), nstrains=4, iupac=True)
    p = _check_world(str(tmp_path), genomes, tail, {"SK_TIMING": "1"})
    assert re.search(rb"1 union pass\(es\) \+ 1 single pass\(es\)", p.stderr)


def test_34_strains_make_two_unions(tmp_path):
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
    p = _check_world(str(tmp_path), genomes, ["-A", "A.txt", "-B", "B.txt", "-C", "C.txt"], {"SK_TIMING": "1"}, gz_every=5)
    assert re.search(rb"34 strain\(s\) opened .* 2 union pass\(es\) \+ 0 single pass\(es\)", p.stderr)


# ---------------------------------------------------------------------------------------------------------------------
# 4. the device API: union COUNT scan + fold == each member's own scan
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [5, 6, 7])
def test_union_count_fold_equals_member_scans(seed):
    rng = random.Random(seed)
    base = _synth.rand_dna(rng, 20000)
    strains = [base, _mutate(rng, base, 0.01), _synth.revcomp(base[5000:]) + _synth.rand_dna(rng, 300), base[:9000] + base[4000:9000] + base[9000:]]
    batches = [_synth.fuzz_stream(rng, base, 3000, p_junk=0.01, min_len=0, max_len=250) for _ in range(3)]
    sets = [sk.Keyset.from_stream(g + b"\n") for g in strains]
    ctxs = [sk.KmerContext(0) for _ in strains]
    own = [sk.KmerContext(0) for _ in strains]
    try:
        for c, o, ks in zip(ctxs, own, sets):
            c.load_keyset(ks, 4)
            o.load_keyset(ks, 4)
        near = [np.full(ks.nrows, 2**32 - 3, dtype=np.uint32) for ks in sets]
        for c, o, v in zip(ctxs, own, near):
            c.set_counts(2, v)
            o.set_counts(2, v)
        with sk.KmerUnion(ctxs) as u:
            with pytest.raises(sk.SKError) as e:
                u.scan_stream(batches[0], 0)                  # no count columns yet: refused, never launched
            assert e.value.code == -7                     # SK_E_STATE
            u.count_enable(1)
            for bt in batches:
                u.scan_stream(bt, 0)
            u.fold_counts(0, 2)
            ms, launches = u.scan_timing()
            assert launches >= len(batches) and ms > 0
            for bt in batches:
                for o in own:
                    o.scan_stream(bt, 2)
            for i, (c, o) in enumerate(zip(ctxs, own)):
                got, want = c.counts(2), o.counts(2)
                assert np.array_equal(got, want), i
                assert (got < 2**32 - 3).any()                # some counters wrapped
            # a batch taken back from members 1 and 3 only
            u.scan_stream(batches[1], 0)
            u.fold_counts(0, 2, member_mask=0b1010, subtract=True)
            for i, c in enumerate(ctxs):
                if i in (1, 3):
                    o2 = sk.KmerContext(0)
                    try:
                        o2.load_keyset(sets[i], 4)
                        o2.set_counts(2, near[i])
                        for bt in (batches[0], batches[2]):
                            o2.scan_stream(bt, 2)
                        assert np.array_equal(c.counts(2), o2.counts(2)), i
                    finally:
                        o2.close()
                else:
                    assert np.array_equal(c.counts(2), own[i].counts(2)), i
    finally:
        for c in ctxs + own:
            c.close()


# ---------------------------------------------------------------------------------------------------------------------
# 5. errors (the ones that need the device; the others are in test_scrub_multi_host.py)
# ---------------------------------------------------------------------------------------------------------------------
def test_missing_list_item_fails_like_the_single_program(tmp_path):
    genomes, tail = _world(40, str(tmp_path), nstrains=3)
    with open(tmp_path / "B.txt", "a") as f:
        f.write("no_such_file.fq\n")
    _write_strains(tmp_path / "S.txt", [(g, f"o{i}.tsv") for i, g in enumerate(genomes)])
    p = _run(["-S", "S.txt"] + tail, cwd=str(tmp_path))
    one = _run(["-r", genomes[0]] + tail, cwd=str(tmp_path))
    assert p.returncode == 1 and one.returncode == 1
    assert b"could not read file no_such_file.fq in GEN_calculate_kmer_count()\n" in one.stderr
    assert p.stderr == one.stderr
    assert not any((tmp_path / f"o{i}.tsv").exists() for i in range(3))


# ---------------------------------------------------------------------------------------------------------------------
# 6. two ranks on the one card: disjoint outfiles, identical to one process
# ---------------------------------------------------------------------------------------------------------------------
def test_two_ranks_deal_the_strains(tmp_path):
    d = str(tmp_path)
    genomes, tail = _world(50, d, nstrains=5)
    _write_strains(os.path.join(d, "S1.txt"), [(g, f"one{i}.tsv") for i, g in enumerate(genomes)])
    assert _run(["-S", "S1.txt", "-p", "prog1"] + tail, cwd=d).returncode == 0
    _write_strains(os.path.join(d, "S2.txt"), [(g, f"two{i}.tsv") for i, g in enumerate(genomes)])
    env = {"WORLD_SIZE": "2"}
    procs = [subprocess.Popen([EXE, "-S", "S2.txt", "-p", f"prog2_{r}"] + tail, cwd=d, env={**os.environ, **env, "RANK": str(r)},
                              stdout=subprocess.PIPE, stderr=subprocess.PIPE) for r in range(2)]
    outs = [p.communicate(timeout=600) for p in procs]
    assert [p.returncode for p in procs] == [0, 0], outs
    for i in range(len(genomes)):
        assert _read(os.path.join(d, f"two{i}.tsv")) == _read(os.path.join(d, f"one{i}.tsv")), i
    assert os.path.exists(os.path.join(d, "prog2_0")) and not os.path.exists(os.path.join(d, "prog2_1"))
    strip = lambda t: [l.split("\t")[0] for l in t.splitlines()]
    assert strip(open(os.path.join(d, "prog2_0")).read()) == strip(open(os.path.join(d, "prog1")).read())
