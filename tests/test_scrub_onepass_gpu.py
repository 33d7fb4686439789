"""kmer_scrub_count -S with every resident union fed by ONE decode of the -A/-B/-C lists (skh_scan_list_many over
sk_scan_pinned[_packed]_many).  The device API against each context scanned alone; then whole runs against SK_SCRUB_UNIONS=1 (one
union per decode, what -S did before): outfiles, stderr and progress file the same, only the number of decodes in SK_TIMING differs."""
import ctypes as C
import gzip
import os
import random
import re
import subprocess

import numpy as np
import pytest

import _oracle
import _synth
import strainer2_amd as sk
from strainer2_amd.native import lib
from test_scrub_multi_gpu import _fasta, _mutate, _read, _run, _world, _write_strains
from test_scrub_multi_workflow_gpu import _cov_path, _cov_rows, _fused, _said, _targets

pytestmark = pytest.mark.gpu

EXE = sk.cli_path()
SK_E_ARG, SK_E_STATE = -3, -7


# ---------------------------------------------------------------------------------------------------------------------
# 1. the device API: one upload, n scans == n scans alone
# ---------------------------------------------------------------------------------------------------------------------
def _chunks(rng, base, n):
    """n record streams of different contents; every third one holds U, IUPAC and other bytes for the byte-string kernel (the
    others only A/C/G/T in either case and N: they can go up packed)"""
    out = []
    for i in range(n):
        odd = i % 3 == 2
        s = bytearray(_synth.fuzz_stream(rng, base, 2500 + 300 * i, junk=b"NnRYKMUu-. acgt\rX*" if odd else b"Nnacgt", p_junk=0.01,
                                         min_len=0, max_len=250))
        if odd:
            for j in range(7, len(s), 301):
                if s[j] != 0x0A:
                    s[j] = rng.choice(b"URYU")
        out.append(bytes(s))
    return out


def test_scan_pinned_many_equals_each_context_alone():
    rng = random.Random(71)
    base = _synth.rand_dna(rng, 30000)
    strains = [base, _mutate(rng, base, 0.01), _synth.revcomp(base[8000:]) + _synth.rand_dna(rng, 400),
               base[:12000] + base[3000:12000] + base[12000:], _mutate(rng, base, 0.03)]
    sets = [sk.Keyset.from_stream(g + b"\n") for g in strains]
    ctxs = []
    try:
        for ks in sets + sets:                            # members of the unions fed together, then of the ones fed alone
            c = sk.KmerContext(0)
            ctxs.append(c)
            c.load_keyset(ks, 4)
        feed, alone = ctxs[:5], ctxs[5:]
        u1, u2 = sk.KmerUnion(feed[0:2]), sk.KmerUnion(feed[2:4])
        r1, r2 = sk.KmerUnion(alone[0:2]), sk.KmerUnion(alone[2:4])
        for u in (u1, u2, r1, r2):
            u.count_enable(1)
        plain, plain_alone = feed[4], alone[4]
        chunks = _chunks(rng, base, 7)                    # more chunks than the staging ring holds, all in flight at once
        for packed in (False, True):
            bufs, tickets = [], []
            for s in chunks:
                pk, odd = sk.pack_stream(s)
                if packed and odd:
                    continue                              # (a chunk with an odd byte goes up as bytes)
                src = pk if packed else np.frombuffer(s, dtype=np.uint8)
                buf = plain.pinned_alloc(max(src.size, 1))
                buf[: src.size] = src
                bufs.append((buf, len(s)))
                fn = plain.scan_pinned_packed_many if packed else plain.scan_pinned_many
                tickets.append(fn([u1, u2], buf, len(s), 0))
            assert len(bufs) == (5 if packed else 7)
            for t in tickets:
                plain.ticket_wait(t)
            for buf, _ in bufs:
                plain.pinned_free(buf)                    # (waits for the whole group's scans)
            for s in chunks:                              # the same chunks, each context alone (sk_scan_pinned[_packed])
                pk, odd = sk.pack_stream(s)
                if packed and odd:
                    continue
                src = pk if packed else np.frombuffer(s, dtype=np.uint8)
                buf = plain_alone.pinned_alloc(max(src.size, 1))
                buf[: src.size] = src
                for h in (plain_alone._h, r1.context_handle, r2.context_handle):
                    t = C.c_uint64(0)
                    fn = lib.sk_scan_pinned_packed if packed else lib.sk_scan_pinned
                    assert fn(h, buf.ctypes.data, len(s), 0, C.byref(t)) == 0
                    assert lib.sk_ticket_wait(h, t.value) == 0 and lib.sk_sync(h) == 0
                plain_alone.pinned_free(buf)
            assert np.array_equal(plain.counts(0), plain_alone.counts(0)), packed
            for got, want in ((u1, r1), (u2, r2)):
                assert np.array_equal(got.counts(0), want.counts(0)), packed
                assert int(got.counts(0).sum()) > 0
        # refused: a column one context lacks, a union without count columns, another device (where there is one)
        buf = plain.pinned_alloc(len(chunks[0]))
        buf[:] = np.frombuffer(chunks[0], dtype=np.uint8)
        with pytest.raises(sk.SKError) as e:
            plain.scan_pinned_many([u1], buf, len(chunks[0]), 2)
        assert e.value.code == SK_E_ARG
        with sk.KmerUnion(feed[0:2]) as bare:
            with pytest.raises(sk.SKError) as e:
                plain.scan_pinned_many([u1, bare], buf, len(chunks[0]), 0)
            assert e.value.code == SK_E_STATE
        try:
            other = sk.KmerContext(1)
        except sk.SKError:
            other = None
        if other is not None:
            try:
                other.load_keyset(sets[0], 4)
                with pytest.raises(sk.SKError) as e:
                    plain.scan_pinned_many([other], buf, len(chunks[0]), 0)
                assert e.value.code == SK_E_ARG
            finally:
                other.close()
        plain.pinned_free(buf)
        for u in (u1, u2, r1, r2):
            u.close()
    finally:
        for c in ctxs:
            c.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. many unions, one decode
# ---------------------------------------------------------------------------------------------------------------------
def _many_world(d, n, seed, iupac_last=False):
    """n strains around one base (diverged copies, a random prefix + part of the base), reads of them as FASTA / FASTQ, plain and
    gzip; -C names strains 3 (twice) and n - 4 and a metagenome.  Returns (genome paths, argv tail)."""
    rng = random.Random(seed)
    base = _synth.rand_dna(rng, 4000)
    genomes = []
    for s in range(n):
        g = _mutate(rng, base, 0.01) if s % 2 else _synth.rand_dna(rng, 500) + base[: 1200 + 30 * s]
        if iupac_last and s == n - 1:
            g = bytearray(g)
            for i in range(5, len(g), 97):
                g[i] = rng.choice(b"RYKM")
            g = bytes(g)
        name = f"g{s}.fa"
        with open(os.path.join(d, name), "wb") as f:
            f.write(_fasta(g, b"g%d" % s))
        genomes.append(name)
    for fi, name in enumerate(("m0.fa", "m1.fq.gz", "m2.fq")):
        recs = _synth.fuzz_stream(rng, base, 1500, p_junk=0.01, min_len=0, max_len=220).split(b"\n")[:-1]
        if name.startswith("m0"):
            body = b"".join(b">r%d\n" % i + r.replace(b"\r", b"A") + b"\n" for i, r in enumerate(recs))
        else:
            body = b"".join(b"@r%d\n" % i + r.replace(b"\r", b"A") + b"\n+\n" + b"I" * len(r) + b"\n" for i, r in enumerate(recs))
        with (gzip.open if name.endswith(".gz") else open)(os.path.join(d, name), "wb") as f:
            f.write(body)
    with open(os.path.join(d, "A.txt"), "w") as f:
        f.write("m0.fa\ng0.fa\n")
    with open(os.path.join(d, "B.txt"), "w") as f:
        f.write("m1.fq.gz\nm2.fq\n")
    with open(os.path.join(d, "C.txt"), "w") as f:
        f.write("".join(l + "\n" for l in (genomes[3], "m2.fq", genomes[n - 4], genomes[3])))
    return genomes, ["-A", "A.txt", "-B", "B.txt", "-C", "C.txt"]


def _S(d, genomes, tail, tag, env=None, gz_every=5, progress=True):
    outs = [f"{tag}{i}.tsv" + (".gz" if i % gz_every == gz_every - 1 else "") for i in range(len(genomes))]
    _write_strains(os.path.join(d, f"S_{tag}.txt"), zip(genomes, outs))
    p = _run(["-S", f"S_{tag}.txt"] + (["-p", f"prog_{tag}"] if progress else []) + tail, cwd=d, env={"SK_TIMING": "1", **(env or {})})
    return p, outs


def _decodes(stderr):
    m = re.search(rb"(\d+) union pass\(es\) \+ (\d+) single pass\(es\).*lists decoded (\d+) time\(s\) \((\d+) bases\)", stderr)
    assert m, stderr.decode()[-2000:]
    return tuple(int(x) for x in m.groups())


def _same_runs(d, a, b, outs_a, outs_b, progress=True):
    assert a.returncode == 0, a.stderr.decode()[-2000:]
    assert b.returncode == 0, b.stderr.decode()[-2000:]
    for x, y in zip(outs_a, outs_b):
        assert _read(os.path.join(d, x)) == _read(os.path.join(d, y)), x
    assert _said(a.stderr) == _said(b.stderr)
    assert _in_order(a.stderr) == _in_order(b.stderr)


def _in_order(stderr):
    """stderr without what SK_TIMING=1 adds, in its order"""
    return [l for l in stderr.decode().splitlines() if "timing" not in l and not l.startswith("key set of ")]


def _progress_col1(d, tag):
    return [l.split("\t")[0] for l in open(os.path.join(d, f"prog_{tag}")).read().splitlines()]


def test_70_strains_three_unions_one_decode(tmp_path):
    d = str(tmp_path)
    genomes, tail = _many_world(d, 70, 70)
    p, outs = _S(d, genomes, tail, "one")
    q, outs_q = _S(d, genomes, tail, "per", env={"SK_SCRUB_UNIONS": "1"})
    _same_runs(d, p, q, outs, outs_q)
    assert _progress_col1(d, "one") == _progress_col1(d, "per")
    assert _decodes(p.stderr)[:3] == (3, 0, 1)
    assert _decodes(q.stderr)[:3] == (3, 0, 3)
    # the -C lines' skip messages: union by union, in -C line order inside each
    assert [l for l in _in_order(p.stderr) if l.startswith("skipping")] == \
        [f"skipping {genomes[3]} (identical match)"] * 2 + [f"skipping {genomes[66]} (identical match)"]
    for i in (0, 31, 32, 63, 64, 69):                    # the first and last strain of every union
        one = _run(["-r", genomes[i]] + tail, cwd=d)
        assert one.returncode == 0, one.stderr
        assert _read(os.path.join(d, outs[i])) == one.stdout, i
    for i in (3, 66):                                     # two that skip -C lines, against the CPU oracle
        o = _oracle.run_oracle_cli(["-r", genomes[i]] + tail, cwd=d)
        assert o.returncode == 0, o.stderr
        assert _read(os.path.join(d, outs[i])) == o.stdout, i


# ---------------------------------------------------------------------------------------------------------------------
# 3. residency planning: SK_SCRUB_UNIONS and SK_SCRUB_HBM_MB
# ---------------------------------------------------------------------------------------------------------------------
def test_residency_planning_decides_the_number_of_decodes(tmp_path):
    d = str(tmp_path)
    genomes, tail = _world(21, d, nstrains=5)
    runs = {}
    for tag, env, want in (("all", {}, 1), ("two", {"SK_SCRUB_UNIONS": "2"}, 2), ("tiny", {"SK_SCRUB_HBM_MB": "1"}, 3),
                           ("junk", {"SK_SCRUB_UNIONS": "0", "SK_SCRUB_HBM_MB": "-5"}, 1)):
        p, outs = _S(d, genomes, tail, tag, env={"SK_SCRUB_GROUP": "2", **env}, gz_every=2)
        assert p.returncode == 0, p.stderr.decode()[-2000:]
        assert _decodes(p.stderr)[:3] == (3, 0, want), tag
        runs[tag] = (p, outs)
    for tag in ("two", "tiny", "junk"):
        _same_runs(d, runs["all"][0], runs[tag][0], runs["all"][1], runs[tag][1])
        assert _progress_col1(d, tag) == _progress_col1(d, "all")
    bases = {tag: _decodes(runs[tag][0].stderr)[3] for tag in runs}
    assert bases["two"] == 2 * bases["all"] and bases["tiny"] == 3 * bases["all"]


# ---------------------------------------------------------------------------------------------------------------------
# 4. cut big plain files: a cut that does not hold puts every union's column back
# ---------------------------------------------------------------------------------------------------------------------
def _cut_files(d, strain, rng):
    def fastq(n):
        out = []
        for i in range(n):
            a = rng.randrange(0, len(strain) - 150)
            out.append(b"@r%d\n%s\n+\n%s\n" % (i, strain[a:a + 150] if rng.random() < 0.6 else _synth.rand_dna(rng, 150), b"I" * 150))
        return b"".join(out)
    recs = []
    for i in range(400):
        a = rng.randrange(0, len(strain) - 150)
        s = strain[a:a + 150]
        q = b"@" + b"I" * 49 + b"\n" + b"I" * 50 + b"\n" + b"+" + b"I" * 49
        recs.append(b"@r%d\n%s\n%s\n%s\n+\n%s\n" % (i, s[:50], s[50:100], s[100:], q))
    with open(os.path.join(d, "wrapped.fq"), "wb") as f:
        f.write(b"".join(recs))
    bad = b"@bad\n" + strain[100:250] + b"\n+\n" + b"I" * 170 + b"\n"
    with open(os.path.join(d, "whole.fq"), "wb") as f:
        f.write(fastq(300) + bad + fastq(300))
    with open(os.path.join(d, "ok.fq"), "wb") as f:
        f.write(fastq(2000))


@pytest.mark.parametrize("pack", ["0", "2"])
def test_cuts_that_hold_and_one_that_does_not(tmp_path, pack):
    d = str(tmp_path)
    rng = random.Random(23)
    base = _synth.rand_dna(rng, 30000)
    genomes = []
    for s in range(5):
        g = _mutate(rng, base, 0.01 * s) if s % 2 == 0 else base[3000 * s:] + _synth.rand_dna(rng, 300)
        with open(os.path.join(d, f"g{s}.fa"), "wb") as f:
            f.write(_fasta(g, b"g%d" % s))
        genomes.append(f"g{s}.fa")
    _cut_files(d, base, rng)
    with open(os.path.join(d, "A.txt"), "w") as f:
        f.write("g1.fa\n")
    with open(os.path.join(d, "good.txt"), "w") as f:
        f.write("ok.fq\ng0.fa\nok.fq\n")
    with open(os.path.join(d, "bad.txt"), "w") as f:
        f.write("ok.fq\nwrapped.fq\nwhole.fq\nok.fq\n")
    env = {"SK_SPLIT_BYTES": "5000", "SK_THREADS": "4", "SK_LIST_PACK": pack, "SK_SCRUB_GROUP": "2"}
    for lst, fails in (("good.txt", False), ("bad.txt", True)):
        tail = ["-A", "A.txt", "-B", lst]
        p, outs = _S(d, genomes, tail, "one" + lst[:3], env=env, gz_every=3)
        q, outs_q = _S(d, genomes, tail, "per" + lst[:3], env={**env, "SK_SCRUB_UNIONS": "1"}, gz_every=3)
        _same_runs(d, p, q, outs, outs_q)
        assert _decodes(p.stderr)[:3] == (3, 0, 1)
        assert (b"did not hold; the list is scanned again uncut" in p.stderr) == fails, lst
        assert _progress_col1(d, "one" + lst[:3]) == _progress_col1(d, "per" + lst[:3])
        nocut, outs_n = _S(d, genomes, tail, "nocut" + lst[:3], env={**env, "SK_NO_SPLIT": "1"}, gz_every=3, progress=False)
        assert nocut.returncode == 0
        for x, y in zip(outs, outs_n):
            assert _read(os.path.join(d, x)) == _read(os.path.join(d, y)), x


# ---------------------------------------------------------------------------------------------------------------------
# 5. the fused workflow (steps 1-4) over one decode
# ---------------------------------------------------------------------------------------------------------------------
def test_fused_workflow_40_strains_one_decode(tmp_path):
    d = str(tmp_path)
    genomes, tail = _many_world(d, 40, 40)
    tail = tail[:4]                                       # (no -C: a drug list that takes most of some strains' k-mers leaves the
    _targets(d, genomes[:4], 40)                          #  filter nothing to keep; tests/test_scrub_multi_workflow_gpu.py has -C)
    p, lines = _fused(d, genomes, tail, ["-B", "T.txt"], env={"SK_TIMING": "1"}, strains_file="S1.txt", prefix="a")
    q, qlines = _fused(d, genomes, tail, ["-B", "T.txt"], env={"SK_TIMING": "1", "SK_SCRUB_UNIONS": "1"}, strains_file="S2.txt", prefix="b")
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    assert q.returncode == 0, q.stderr.decode()[-3000:]
    assert _decodes(p.stderr)[:3] == (2, 0, 1) and _decodes(q.stderr)[:3] == (2, 0, 2)
    assert _said(p.stderr) == _said(q.stderr)
    for a, b in zip(lines, qlines):
        assert _read(os.path.join(d, a[1])) == _read(os.path.join(d, b[1])), a
        assert _read(os.path.join(d, a[2])) == _read(os.path.join(d, b[2])), a
        assert _cov_rows(os.path.join(d, _cov_path(a[2]))) == _cov_rows(os.path.join(d, _cov_path(b[2]))), a


# ---------------------------------------------------------------------------------------------------------------------
# 6. failures and the paths that keep a pass of their own
# ---------------------------------------------------------------------------------------------------------------------
def test_missing_list_item_with_70_strains(tmp_path):
    d = str(tmp_path)
    genomes, tail = _many_world(d, 70, 71)
    with open(os.path.join(d, "B.txt"), "a") as f:
        f.write("no_such_file.fq\n")
    p, outs = _S(d, genomes, tail, "one", progress=False)
    q, outs_q = _S(d, genomes, tail, "per", env={"SK_SCRUB_UNIONS": "1"}, progress=False)
    assert p.returncode == q.returncode == 1
    assert b"could not read file no_such_file.fq in GEN_calculate_kmer_count()\n" in p.stderr
    assert _in_order(p.stderr) == _in_order(q.stderr)
    assert not any(os.path.exists(os.path.join(d, o)) for o in outs + outs_q)


def test_iupac_strain_among_34_keeps_its_own_pass(tmp_path):
    d = str(tmp_path)
    genomes, tail = _many_world(d, 34, 34, iupac_last=True)
    p, outs = _S(d, genomes, tail, "one")
    q, outs_q = _S(d, genomes, tail, "per", env={"SK_SCRUB_UNIONS": "1"})
    _same_runs(d, p, q, outs, outs_q)
    assert _decodes(p.stderr)[:3] == (2, 1, 2)            # 33 strains in two unions over one decode, the IUPAC one alone
    assert _decodes(q.stderr)[:3] == (2, 1, 3)
    one = _run(["-r", genomes[33]] + tail, cwd=d)
    assert one.returncode == 0 and _read(os.path.join(d, outs[33])) == one.stdout


def test_two_ranks_each_decode_once(tmp_path):
    d = str(tmp_path)
    genomes, tail = _many_world(d, 40, 41)
    files = {}
    for tag, env in (("one", {}), ("per", {"SK_SCRUB_UNIONS": "1"})):
        outs = [f"{tag}{i}.tsv" for i in range(len(genomes))]
        _write_strains(os.path.join(d, f"S_{tag}.txt"), zip(genomes, outs))
        procs = [subprocess.Popen([EXE, "-S", f"S_{tag}.txt"] + tail, cwd=d,
                                  env={**os.environ, "WORLD_SIZE": "2", "RANK": str(r), "SK_SCRUB_GROUP": "8", "SK_TIMING": "1", **env},
                                  stdout=subprocess.PIPE, stderr=subprocess.PIPE) for r in range(2)]
        res = [p.communicate(timeout=600) for p in procs]
        assert [p.returncode for p in procs] == [0, 0], res
        files[tag] = outs
        for _, err in res:                                # 20 strains per rank: 3 unions of up to 8
            assert _decodes(err)[:3] == ((3, 0, 1) if tag == "one" else (3, 0, 3))
    for a, b in zip(files["one"], files["per"]):
        assert _read(os.path.join(d, a)) == _read(os.path.join(d, b)), a
