"""strain_detect's target cache on the device (opt-in: --target-cache DIR / SK_TARGET_CACHE=DIR).

1. sk_batch_pack_home against sk_pack_stream, byte for byte, the odd flag included: lengths around the 16-byte chunk and the pair of
   chunks a lane takes, every byte value at every position of a chunk, a batch refilled shorter over bytes of an earlier fill, the
   output buffer behind the packed form, SK_E_STATE on a packed batch.
2. Round trip: a batch filled with bytes and packed home, a second batch filled with that packed form and the same starts -- the same
   tallies and hit logs, on one table and on a 2-member union, also with a tally launched before the pack was waited for.
3. bin/strain_detect off, filling and served: the golden cases at 64- and 4096-byte chunks; plain and .gz targets; IUPAC, U and CR;
   short and empty records; a truncated FASTQ; a PE2 that ends before PE1; -S in two unions, SK_DEVICES=0,0, the fused
   kmer_scrub_count job (they reach the cache through sd_run, which every one of these paths ends in); random worlds.
4. Validity: a touched source, ro, a flipped payload byte, a changed length under a sum that holds."""
import gzip
import json
import os
import random
import shutil
import subprocess

import numpy as np
import pytest

import _skt
import _synth
import _tally_ref as tr
import strainer2_amd as sk
from strainer2_amd.native import TallyBatch, pack_stream

pytestmark = pytest.mark.gpu
K = 31
SD_CASES = ["batch", "cli_se", "cli_pe", "cli_pei", "cli_default", "background", "err_missing", "err_type",
            "err_pe_one_file", "err_b_and_B", "err_no_inf", "err_no_read1"]


# =====================================================================================================================
# 1. pack_home against pack_stream
# =====================================================================================================================
@pytest.fixture(scope="module")
def world():
    """two strains that share keys (a 2-member union), a third of their rows informative"""
    rng = random.Random(41)
    g = _synth.rand_dna(rng, 120_000)
    ctxs, sets = [], []
    for s in (g[:80_000], g[50_000:]):
        ks = sk.Keyset.from_stream(s + b"\n", default_val=1, incr=0)
        c = sk.KmerContext(0)
        c.load_keyset(ks, 6)
        t = np.ones(ks.nrows, dtype=np.uint32)
        t[rng.sample(range(ks.nrows), ks.nrows // 3)] = 2
        c.set_counts(0, t)
        ctxs.append(c)
        sets.append(ks)
    u = sk.KmerUnion(ctxs, 0, 2)
    ba, bb = TallyBatch(ctxs[0]), TallyBatch(ctxs[0])
    yield dict(g=g, ctxs=ctxs, u=u, ba=ba, bb=bb)
    ba.close()
    bb.close()
    u.close()
    for c in ctxs:
        c.close()
    for k in sets:
        k.close()


def _check_pack(b, stream, guard=64):
    b.fill(stream, np.zeros(1, dtype=np.uint32))
    got, odd = b.pack_home(guard=guard)
    want, want_odd = pack_stream(stream)
    n = len(want)
    assert odd == want_odd, len(stream)
    assert np.array_equal(got[:n], want), len(stream)
    assert (got[n:] == 0xA5).all(), (len(stream), "bytes behind the packed form were written")


@pytest.mark.parametrize("n", [1, 15, 16, 17, 31, 32, 33, 47, 4095, 4097, 32767, 32768, 32769, 100_003])
def test_pack_home_lengths(world, n):
    rng = random.Random(n)
    s = bytearray(_synth.rand_dna(rng, n))
    for i in range(0, n, 151):
        s[i] = ord("\n")
    for i in range(7, n, 977):
        s[i] = ord("Nn"[i & 1])
    _check_pack(world["ba"], bytes(s))
    if n > 20:                                             # ... and with a byte for the byte-string kernel in the last, cut chunk
        s[n - 1] = ord("R")
        _check_pack(world["ba"], bytes(s))


def test_pack_home_every_byte_value_at_every_position(world):
    for pos in range(16):
        s = bytearray(b"ACGT" * 4 * 256)
        for v in range(256):
            s[16 * v + pos] = v
        _check_pack(world["ba"], bytes(s))
    for v in (0, ord("R"), ord("U"), 13, ord("a"), ord("n"), 255):     # one value alone: the flag is this byte's
        s = bytearray(b"ACGTACGTACGTACGTACGTACGTACGTACGTACG")
        s[33] = v
        _check_pack(world["ba"], bytes(s))


def test_pack_home_ignores_what_an_earlier_longer_fill_left(world):
    b = TallyBatch(world["ctxs"][0])
    try:
        rng = random.Random(3)
        long = bytearray(_synth.rand_dna(rng, 5000))
        long[4990] = ord("R")
        b.fill(bytes(long), np.zeros(1, dtype=np.uint32))
        _, odd = b.pack_home()
        assert odd
        for n in (4985, 4989, 4990, 3001):                 # (the R lies behind nbytes: in the cut chunk's own 16 bytes, in the next chunk, far behind)
            short = bytes(long[:n])
            b.fill(short, np.zeros(1, dtype=np.uint32))
            got, odd = b.pack_home(guard=32)
            want, want_odd = pack_stream(short)
            assert not odd and not want_odd and np.array_equal(got[:len(want)], want) and (got[len(want):] == 0xA5).all(), n
    finally:
        b.close()


def test_pack_home_state_errors(world):
    b = TallyBatch(world["ctxs"][0])
    try:
        with pytest.raises(sk.SKError) as e:               # empty
            b.pack_home()
        assert e.value.code == sk.native.SK_E_STATE
        s = _synth.rand_dna(random.Random(4), 500) + b"\n"
        b.fill(s, np.zeros(1, dtype=np.uint32), packed=True)
        with pytest.raises(sk.SKError) as e:
            b.pack_home()
        assert e.value.code == sk.native.SK_E_STATE
        text = b">a\n" + s
        info, _ = b.fill_text(text)
        assert info.status == 0
        with pytest.raises(sk.SKError) as e:               # parsed from text
            b.pack_home()
        assert e.value.code == sk.native.SK_E_STATE
        b.fill(s, np.zeros(1, dtype=np.uint32))
        got, odd = b.pack_home()
        assert not odd and np.array_equal(got, pack_stream(s)[0])
    finally:
        b.close()


# =====================================================================================================================
# 2. round trip: bytes -> pack_home -> fill_packed
# =====================================================================================================================
def _sorted_hits(h):
    h = np.asarray(h, dtype=np.int64).reshape(-1, h.shape[1] if len(h) else 2)
    return h[np.lexsort(tuple(h[:, i] for i in range(h.shape[1] - 1, -1, -1)))] if len(h) else h


def _records(rng, g, n):
    out = []
    for _ in range(n):
        a = rng.randrange(len(g) - 300)
        r = g[a:a + rng.randint(31, 250)]
        out.append(_synth.revcomp(r) if rng.random() < 0.5 else (r[:40] + b"N" + r[41:] if rng.random() < 0.1 and len(r) > 45 else r))
    return out


@pytest.mark.parametrize("n", [1, 700, 1500])
def test_round_trip_tallies_and_hit_logs(world, n):
    """700 records: more than one 32 KiB tile, 1500: several; the first tally of the byte batch is launched BEFORE the pack is waited for"""
    rng = random.Random(50 + n)
    recs = _records(rng, world["g"], n)
    stream = b"".join(r + b"\n" for r in recs)
    starts = tr.starts_of(recs)
    ba, bb, c0 = world["ba"], world["bb"], world["ctxs"][0]
    ba.fill(stream, starts)
    nb = int(sk.native.lib.sk_packed_bytes(len(stream)))
    buf = c0.pinned_alloc(nb + 16)
    try:
        flag = buf[(nb + 7) // 8 * 8:][:4].view(np.uint32)
        flag[0] = 7
        ba.pack_home_begin(buf, flag)
        c0.tally_launch(ba, 0, 2)                          # (beside the pack: it waits for the upload's event only)
        ba.pack_home_wait()
        t0, h0, _ = c0.tally_collect()
        assert flag[0] == 0
        packed = buf[:nb].copy()
    finally:
        c0.pinned_free(buf)
    assert np.array_equal(packed, pack_stream(stream)[0])
    rc = sk.native.lib.sk_batch_fill_packed(bb._h, packed.ctypes.data, len(stream), starts.ctypes.data, len(starts))
    assert rc == 0
    c0._ck(sk.native.lib.sk_batch_sync(bb._h))
    bb.nbytes, bb.nrec = len(stream), len(starts)
    inf = 0
    for s, c in enumerate(world["ctxs"]):
        c.tally_launch(ba, 0, 2)
        t1, h1, _ = c.tally_collect()
        c.tally_launch(bb, 0, 2)
        t2, h2, _ = c.tally_collect()
        assert np.array_equal(t1, t2) and np.array_equal(_sorted_hits(h1), _sorted_hits(h2)), s
        if s == 0:
            assert np.array_equal(t0, t1) and np.array_equal(_sorted_hits(h0), _sorted_hits(h1))
            inf = int(t1[:, 1].sum())
    ut1, uh1 = world["u"].tally_filled(ba)
    ut2, uh2 = world["u"].tally_filled(bb)
    assert np.array_equal(ut1, ut2) and np.array_equal(uh1, uh2)
    assert inf > 0 or n == 1, "no informative hit: the comparison would be of zeros"


# =====================================================================================================================
# 3. the program: off, filling, served
# =====================================================================================================================
def _exe():
    return sk.cli_path("strain_detect")


@pytest.mark.parametrize("chunk", ["64", "4096"])
@pytest.mark.parametrize("name", SD_CASES)
def test_golden_cases_off_filling_served(golden, name, chunk, tmp_path):
    fill, served = _skt.off_filling_served([_exe()], os.path.join(golden, "sd_cases", name), tmp_path, env={"SK_SD_CHUNK_BYTES": chunk})
    if name == "cli_se":
        assert fill == (0, 1, 0, 0) and served == (1, 0, 0, 0)
    if name == "cli_pe":
        assert fill == (0, 2, 0, 0) and served == (2, 0, 0, 0)
    if name == "batch":
        assert fill[1] >= 4 and fill[0] >= 1


@pytest.fixture(scope="module")
def strain(tmp_path_factory):
    """two strains with their informative lists"""
    d = tmp_path_factory.mktemp("tcache")
    rng = random.Random(99)
    g = _synth.rand_dna(rng, 30_000)
    (d / "s.fa").write_bytes(b">s\n" + g + b"\n")
    kms = sorted({max(g[i:i + K], _synth.revcomp(g[i:i + K])) for i in range(0, len(g) - K, 5)})
    (d / "s.inf").write_bytes(b"#informative\n" + b"\n".join(kms) + b"\n")
    other = _synth.rand_dna(rng, 30_000)
    (d / "t.fa").write_bytes(b">t\n" + g[:10_000] + other[:20_000] + b"\n")
    kms = sorted({max(other[i:i + K], _synth.revcomp(other[i:i + K])) for i in range(0, 19_000, 7)})
    (d / "t.inf").write_bytes(b"#informative\n" + b"\n".join(kms) + b"\n")
    return dict(d=d, g=g, other=other)


def _piece(rng, g, n):
    a = rng.randrange(len(g) - n)
    s = g[a:a + n]
    return _synth.revcomp(s) if rng.random() < 0.5 else s


def _reads(rng, g, n, lo=20, hi=200):
    return [_piece(rng, g, rng.randint(lo, hi)) if rng.random() < 0.8 else _synth.rand_dna(rng, rng.randint(lo, hi)) for _ in range(n)]


def _fasta(recs):
    return b"".join(b">r%d\n%s\n" % (i, r) if r else b">r%d\n" % i for i, r in enumerate(recs))


def _fastq(recs):
    return b"".join(b"@q%d\n%s\n+\n%s\n" % (i, r, b"I" * len(r)) for i, r in enumerate(recs))


def _three(strain, tmp_path, files, mode, chunk="64", rc=0, env=None):
    """strain_detect over `files` off, filling and served: exit code, stdout, stderr less the timing lines and hits are equal; returns
    (the counters of the filling run, of the served run, the hits, the cache directory)"""
    d = strain["d"]
    argv = ["-r", str(d / "s.fa"), "-a", str(d / "s.inf"), "-b", str(files[0])] + (["-c", str(files[1])] if len(files) > 1 else []) + ["-t", mode]
    cache = tmp_path / "tc"
    cache.mkdir(exist_ok=True)
    e = dict(os.environ, SK_SD_TIMING="1", **(env or {}))
    for k in ("SK_TARGET_CACHE", "SK_TARGET_CACHE_MODE"):
        e.pop(k, None)
    if chunk:
        e["SK_SD_CHUNK_BYTES"] = str(chunk)
    runs = []
    for k in range(3):
        out = tmp_path / ("o%d.gz" % k)
        p = subprocess.run([_exe()] + argv + ["-o", str(out)] + (["--target-cache", str(cache)] if k else []), cwd=str(tmp_path), env=e, capture_output=True)
        assert p.returncode == rc, p.stderr.decode()[-2000:]
        runs.append((p.stdout, _skt.quiet(p.stderr), gzip.open(out, "rb").read() if rc == 0 else None, _skt.stats(p.stderr)))
        _skt.no_temporaries(cache)
    assert runs[0][:3] == runs[1][:3] == runs[2][:3]
    assert runs[0][3] is None
    for f in os.listdir(cache):
        _skt.segments(os.path.join(cache, f))
    return runs[1][3], runs[2][3], runs[0][2], cache


@pytest.mark.parametrize("gz", [False, True])
@pytest.mark.parametrize("chunk", ["64", "5000", None])
def test_plain_and_gz_targets(strain, tmp_path, gz, chunk):
    rng = random.Random(20)
    text = _fastq(_reads(rng, strain["g"], 400, 31, 200))
    f = tmp_path / ("r.fq.gz" if gz else "r.fq")
    f.write_bytes(gzip.compress(text) if gz else text)
    fill, served, hits, cache = _three(strain, tmp_path, [f], "SE", chunk=chunk)
    assert fill == (0, 1, 0, 0) and served == (1, 0, 0, 0) and hits.count(b"\n") > 50
    _, segs = _skt.segments(os.path.join(cache, os.listdir(cache)[0]))
    assert all(s["kind"] == 1 for s in segs) and (len(segs) > 1) == (chunk is not None)


def test_odd_bytes_short_and_empty_records(strain, tmp_path):
    """IUPAC letters, U and a CR: their segments are kept as bytes (the device's odd flag), the others packed; records shorter than k
    and empty ones have no place in a stream, and a segment of nothing else has an empty one"""
    rng = random.Random(21)
    recs = _reads(rng, strain["g"], 300, 40, 150)
    recs[5] = recs[5][:20] + b"R" + recs[5][21:]
    recs[100] = recs[100].replace(b"T", b"U")
    recs[200] = recs[200][:30] + b"Y" + recs[200][31:]
    for i in range(10, 300, 17):
        recs[i] = b"" if i % 2 else recs[i][:12]
    recs[150:150] = [b"ACGT", b"", b"A" * 30, b"", b"AC"]         # (64-byte chunks: a whole chunk of records without a window)
    text = _fasta(recs) + b">cr\r\n" + recs[0] + b"\r\n"
    for name, data in (("odd.fa", text), ("odd.fa.gz", gzip.compress(text))):
        w = tmp_path / name.replace(".", "_")
        w.mkdir()
        (w / name).write_bytes(data)
        fill, served, hits, cache = _three(strain, w, [w / name], "SE", chunk="400")
        assert fill == (0, 1, 0, 0) and served == (1, 0, 0, 0) and hits.count(b"\n") > 20
        _, segs = _skt.segments(os.path.join(cache, os.listdir(cache)[0]))
        assert sum(s["kind"] == 2 for s in segs) >= 3 and sum(s["kind"] == 1 and s["np"] > 0 for s in segs) > 10
    (tmp_path / "short.fa").write_bytes(_fasta([b"ACGT", b"", b"A" * 30]))
    fill, served, _, cache = _three(strain, tmp_path, [tmp_path / "short.fa"], "SE")
    assert fill == (0, 1, 0, 0) and served == (1, 0, 0, 0)
    _, segs = _skt.segments(os.path.join(cache, os.listdir(cache)[0]))
    assert all(s["stream_len"] == 0 for s in segs)


def test_truncated_fastq_is_written_with_its_ending(strain, tmp_path):
    rng = random.Random(22)
    recs = _reads(rng, strain["g"], 60, 40, 150)
    (tmp_path / "t.fq").write_bytes(_fastq(recs) + b"@last\n" + recs[0] + b"\n+\nII")
    fill, served, hits, _ = _three(strain, tmp_path, [tmp_path / "t.fq"], "SE")
    assert fill == (0, 1, 0, 0) and served == (1, 0, 0, 0) and hits.count(b"\n") > 10


def test_pe2_ends_before_pe1(strain, tmp_path):
    """the reference's message, exit code 1 in all three runs; PE2 was read to its end and is written, PE1 was abandoned: nothing"""
    rng = random.Random(23)
    r1 = _reads(rng, strain["g"], 80, 40, 150)
    (tmp_path / "a_1.fq").write_bytes(_fastq(r1))
    (tmp_path / "a_2.fq").write_bytes(_fastq([_synth.revcomp(r) for r in r1[:30]]))
    d = strain["d"]
    cache = tmp_path / "tc"
    cache.mkdir()
    runs = []
    for k in range(3):
        p = subprocess.run([_exe(), "-r", str(d / "s.fa"), "-a", str(d / "s.inf"), "-t", "PE", "-b", str(tmp_path / "a_1.fq"), "-c", str(tmp_path / "a_2.fq"),
                            "-o", str(tmp_path / f"o{k}.gz")] + (["--target-cache", str(cache)] if k else []),
                           env=dict(os.environ, SK_SD_TIMING="1", SK_SD_CHUNK_BYTES="64"), capture_output=True)
        runs.append((p.returncode, p.stdout, _skt.quiet(p.stderr), _skt.stats(p.stderr)))
        _skt.no_temporaries(cache)
    assert runs[0][:3] == runs[1][:3] == runs[2][:3] and runs[0][0] == 1 and b"reached end of PE2" in runs[0][2]
    assert runs[1][3] == (0, 1, 0, 1) and runs[2][3] == (1, 0, 0, 1)
    assert [f.split(".")[0] for f in os.listdir(cache)] == ["a_2"]


def _two_strains(strain, tmp_path, env):
    """-S with two strains: the files off, filling and served"""
    d = strain["d"]
    rng = random.Random(18)
    recs = _reads(rng, strain["g"], 400) + _reads(rng, strain["other"], 400)
    rng.shuffle(recs)
    (tmp_path / "r.fa").write_bytes(_fasta(recs))
    (tmp_path / "r.fq.gz").write_bytes(gzip.compress(_fastq([r for r in recs if r])))
    (tmp_path / "B.txt").write_text(f"SE\t{tmp_path}/r.fa\nPEI\t{tmp_path}/r.fq.gz\n")
    cache = tmp_path / "tc"
    cache.mkdir()
    res = []
    for k in range(3):
        (tmp_path / "S.txt").write_text(f"{d}/s.fa\t{d}/s.inf\t{tmp_path}/a{k}.gz\n{d}/t.fa\t{d}/t.inf\t{tmp_path}/b{k}.gz\n")
        e = dict(os.environ, SK_SD_TIMING="1", SK_SD_CHUNK_BYTES="20000", **env)
        if k:
            e["SK_TARGET_CACHE"] = str(cache)
        p = subprocess.run([_exe(), "-S", str(tmp_path / "S.txt"), "-B", str(tmp_path / "B.txt")], cwd=str(tmp_path), env=e, capture_output=True)
        assert p.returncode == 0, p.stderr.decode()[-2000:]
        res.append((p.stdout, gzip.open(tmp_path / f"a{k}.gz").read(), gzip.open(tmp_path / f"b{k}.gz").read(), _skt.stats(p.stderr)))
        _skt.no_temporaries(cache)
    assert res[0][:3] == res[1][:3] == res[2][:3] and res[0][3] is None
    assert res[1][3] == (0, 2, 0, 0) and res[2][3] == (2, 0, 0, 0)
    assert res[2][1].count(b"\n") > 50 and res[2][2].count(b"\n") > 50


def test_two_strains_in_two_unions(strain, tmp_path):
    """-S, like SK_DEVICES and the fused job below, ends in sd_run and its streams: the cache needs nothing of its own there"""
    _two_strains(strain, tmp_path, {"SK_SD_GROUP": "1"})


def test_two_logical_devices(strain, tmp_path):
    _two_strains(strain, tmp_path, {"SK_DEVICES": "0,0", "SK_SD_GROUP": "1"})


def test_the_fused_scrub_and_detect_job(tmp_path):
    import test_scrub_multi_workflow_gpu as wf
    d = str(tmp_path)
    genomes, tail = wf._world(1, d, nstrains=5)
    wf._drug_list(d, genomes, 1)
    wf._targets(d, genomes, 1)
    cache = tmp_path / "tc"
    cache.mkdir()
    outs, st = [], []
    for k in range(3):
        p, lines = wf._fused(d, genomes, tail, ["-B", "T.txt"] + (["--target-cache", str(cache)] if k else []), env={"SK_SD_TIMING": "1"}, prefix=f"f{k}_")
        assert p.returncode == 0, p.stderr.decode()[-2000:]
        outs.append([(wf._read(os.path.join(d, l[1])), wf._read(os.path.join(d, l[2]))) for l in lines])
        st.append(_skt.stats(p.stderr))
        _skt.no_temporaries(cache)
    assert outs[0] == outs[1] == outs[2] and sum(len(h) for _, h in outs[2]) > 1000
    assert st == [None, (0, 4, 0, 0), (4, 0, 0, 0)]


@pytest.fixture(scope="module")
def strain_ref(strain):
    """tests/_tally_ref.py's table of the strain, and which of its rows the -a list makes informative"""
    g, d = strain["g"], strain["d"]
    o = tr.OracleStrain(g + b"\n", capacity=1 << 17)
    kms = {l for l in (d / "s.inf").read_bytes().split(b"\n")[1:] if l}
    return o, np.array([max(k, _synth.revcomp(k)) in kms for k in o.keys], dtype=bool)


@pytest.mark.parametrize("seed", range(6))
def test_random_worlds_served_against_off_and_the_tally_reference(strain, strain_ref, tmp_path, seed):
    """six random worlds, plain and .gz, FASTA and FASTQ, SE and PEI: served against off (and filling), and the k-mers of the hit lines
    against tests/_tally_ref.py"""
    g = strain["g"]
    o, informative = strain_ref
    rng = random.Random(2000 + seed)
    recs = _reads(rng, g, 200 + 50 * seed, 1, 260)
    for i in range(3, len(recs), 23):
        recs[i] = recs[i][:rng.randint(1, 30)]
    if seed % 2 and len(recs) % 2:
        recs.pop()
    text = _fastq(recs) if seed % 3 == 0 else _fasta(recs)
    gz = seed >= 3
    f = tmp_path / ("w.txt.gz" if gz else "w.txt")
    f.write_bytes(gzip.compress(text) if gz else text)
    fill, served, hits, _ = _three(strain, tmp_path, [f], "PEI" if seed % 2 else "SE", chunk=str((64, 700, 3000)[seed % 3]))
    assert fill == (0, 1, 0, 0) and served == (1, 0, 0, 0)
    stream = b"".join(r + b"\n" for r in recs)
    want, log = o.tally(stream, tr.starts_of(recs), informative)
    lines = [l.split(b"\t") for l in hits.split(b"\n") if l]
    got_keys = {max(l[5], _synth.revcomp(l[5])) for l in lines if not l[0].startswith(b"#")}
    want_keys = {max(o.keys[row], _synth.revcomp(o.keys[row])) for (_r, row) in log}
    assert got_keys == want_keys and len(want_keys) > 10, seed


# =====================================================================================================================
# 4. validity
# =====================================================================================================================
def test_validity_stale_ro_and_damage(golden, tmp_path):
    work = tmp_path / "case"
    shutil.copytree(os.path.join(golden, "sd_cases", "cli_se"), work)
    cache = tmp_path / "tc"
    cache.mkdir()
    env = {"SK_SD_CHUNK_BYTES": "64"}
    run = lambda **kw: _skt.run_case([_exe()], str(work), tmp_path, cache=cache, env=env, **kw)
    assert run(mode="ro")[4] == (0, 0, 0, 0) and os.listdir(cache) == []          # ro on an empty directory writes nothing
    assert run()[4] == (0, 1, 0, 0)
    (f,) = os.listdir(cache)
    path = os.path.join(cache, f)
    good = open(path, "rb").read()
    _, segs = _skt.segments(path)
    assert len(segs) > 3
    target = work / "se.fq.gz"
    st = os.stat(target)
    os.utime(target, ns=(st.st_atime_ns, st.st_mtime_ns + 1_000_000_000))
    assert run(mode="ro")[4] == (0, 0, 1, 0) and open(path, "rb").read() == good   # stale: left alone in ro
    assert run()[4] == (0, 1, 1, 0) and open(path, "rb").read() != good            # ... re-parsed and rewritten in rw
    assert run()[4] == (1, 0, 0, 0)
    good = open(path, "rb").read()
    _skt.flip_payload_byte(path, [i for i, s in enumerate(segs) if s["payload_len"]][1])
    rc, _, err, _, _ = run(check=False)
    assert rc != 0 and path.encode() in err
    open(path, "wb").write(good)
    i = [k for k, s in enumerate(segs) if s["np"]][0]
    r = [k for k, l in enumerate(segs[i]["lens"]) if l >= 31][0]
    _skt.change_length(path, i, r, segs[i]["lens"][r] - 1)
    rc, _, err, hits, _ = run(check=False)
    assert rc != 0 and path.encode() in err
    rc, _, err, hits, st = _skt.run_case([_exe()], str(work), tmp_path, cache=tmp_path / "nowhere", env=env, check=False)
    assert rc == 0 and err.count(b"cannot be used") == 1 and st is None and hits == open(work / "expected.hits", "rb").read()
