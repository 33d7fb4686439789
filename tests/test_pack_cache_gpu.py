"""The list scan's packed input cache on the device: the pack kernel (sk_pack_device) against the host's sk_pack_stream, byte for
byte; sk_scan_pinned_pack_many against sk_scan_pinned_many; and the programs -- golden cases, random worlds against the oracle,
-S with two unions -- printing the same bytes with the cache off, being filled and served from."""
import gzip
import json
import os
import random
import re
import shutil
import subprocess

import numpy as np
import pytest

import _synth
import strainer2_amd as sk
from strainer2_amd import native

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = sk.cli_path()
ORACLE = os.path.join(REPO, "oracle", "kso_oracle")
CASES = ["mixed", "truncated_fastq", "iupac_strain", "drug", "missing_in_list", "skip_after_missing"]
LENGTHS = [1, 15, 16, 17, 31, 32, 33, 47, 4095, 4097]
STAT = re.compile(rb"pack cache: .*?: (\d+) items served, (\d+) written, (\d+) stale, (\d+) not cached")


@pytest.fixture(scope="module")
def world():
    """a strain resident in a context, and reads of it"""
    rng = random.Random(4711)
    strain = _synth.rand_dna(rng, 20000)
    ks = sk.Keyset.from_stream(strain + b"\n")
    ctx = sk.KmerContext(0)
    ctx.load_keyset(ks, 4)
    yield ctx, ks, strain
    ctx.close()


def device_pack(ctx, data, nbytes=None, poison=b"A"):
    """-> (packed bytes the device wrote for data[:nbytes], odd); the device bytes beyond nbytes hold `poison`, the packed buffer is
    longer than needed and must be left alone behind sk_packed_bytes(nbytes)"""
    buf = np.frombuffer(bytes(data), dtype=np.uint8)
    n = buf.size if nbytes is None else nbytes
    room = (n + 15) // 16 * 16 + 64
    up = np.full(room, poison[0], dtype=np.uint8)
    up[:n] = buf[:n]
    d_in = ctx.dev_alloc(room)
    pb = int(native.lib.sk_packed_bytes(n))
    d_out = ctx.dev_alloc(pb + 64)
    ctx.dev_upload(d_in, up)
    ctx.dev_upload(d_out, np.full(pb + 64, 0xEE, dtype=np.uint8))
    odd = ctx.pack_device(d_in, n, d_out)
    got = ctx.dev_download(d_out, pb + 64)
    ctx.dev_free(d_in)
    ctx.dev_free(d_out)
    assert (got[pb:] == 0xEE).all()
    return got[:pb], odd


def check_pack(ctx, data, nbytes=None):
    n = len(data) if nbytes is None else nbytes
    want, want_odd = native.pack_stream(bytes(data[:n]))
    got, odd = device_pack(ctx, data, nbytes)
    assert odd == bool(want_odd)
    assert np.array_equal(got, want[:got.size])
    return odd


def test_pack_device_every_byte_value_at_every_position(world):
    ctx = world[0]
    base = np.frombuffer(b"ACGTTGCAGTCAACGT", dtype=np.uint8)
    allv = np.tile(base, 256 * 16).reshape(256, 16, 16).copy()
    for pos in range(16):
        allv[:, pos, pos] = np.arange(256, dtype=np.uint8)
    assert allv.size == 65536
    assert check_pack(ctx, allv.tobytes()) is True
    odd_values = 0
    for v in range(256):                                   # the flag, value by value: 16 chunks, the byte at each position once
        odd_values += check_pack(ctx, allv[v].tobytes())
    assert odd_values == 256 - len(b"ACGTNacgtn\n")


@pytest.mark.parametrize("n", LENGTHS)
def test_pack_device_lengths_with_poison_behind_the_end(world, n):
    ctx = world[0]
    rng = random.Random(n)
    data = bytes(rng.choice(b"ACGTACGTACGTNn\n") for _ in range(n + 40))
    assert check_pack(ctx, data, n) is False
    got_a, _ = device_pack(ctx, data, n, poison=b"A")
    got_r, odd_r = device_pack(ctx, data, n, poison=b"R")      # an odd byte behind the end is not the stream's
    assert np.array_equal(got_a, got_r) and odd_r is False
    if n % 16:                                             # the last chunk's bytes beyond n are "no A/C/G/T"
        nch = (n + 15) // 16
        mask = int(got_a[nch * 4 + 2 * (nch - 1)]) | int(got_a[nch * 4 + 2 * (nch - 1) + 1]) << 8
        assert mask >> (n % 16) == 0xFFFF >> (n % 16)


@pytest.mark.parametrize("n,foreign", [(100_003, 0), (100_003, 5), (1 << 20, 3), (17 * (1 << 20) + 5, 0), (17 * (1 << 20) + 5, 1)])
def test_pack_device_random_streams(world, n, foreign):
    ctx = world[0]
    rng = np.random.default_rng(n + foreign)
    data = np.frombuffer(b"ACGTacgtACGTACGTNn\n\nACGT", dtype=np.uint8)[rng.integers(0, 24, n)].copy()
    for at in rng.integers(0, n, foreign):
        data[at] = rng.choice(np.frombuffer(b"RYKMUu\r-.*X\x00\xff", dtype=np.uint8))
    if foreign:
        data[n - 1] = ord("R")                             # (the very last byte too)
    assert check_pack(ctx, data.tobytes()) is bool(foreign)


@pytest.mark.parametrize("nctx", [1, 2])
def test_scan_pinned_pack_many_counts_and_packed_form(world, nctx):
    ctx, ks, strain = world
    rng = random.Random(100 + nctx)
    others = []
    if nctx == 2:
        o = sk.KmerContext(0)
        o.load_keyset(ks, 4)
        others.append(o)
    try:
        # three batches in a row (the two device buffers take turns, the second is longer: they grow), the last with odd bytes
        batches = [_synth.fuzz_stream(rng, strain, 800, junk=b"Nn", p_junk=0.01, min_len=20, max_len=300),
                   _synth.fuzz_stream(rng, strain, 4000, junk=b"Nn", p_junk=0.01, min_len=20, max_len=300),
                   _synth.fuzz_stream(rng, strain, 900, p_junk=0.01, min_len=20, max_len=300)]
        cap = max(len(b) for b in batches)
        pin = ctx.pinned_alloc(cap)
        outs = [ctx.pinned_alloc(int(native.lib.sk_packed_bytes(cap))) for _ in batches]
        odds = [ctx.pinned_alloc(4096) for _ in batches]
        for c in [ctx] + others:
            c.zero_counts(2)
            c.zero_counts(3)
        for b in batches:                                  # what sk_scan_pinned_many counts: column 2
            pin[:len(b)] = np.frombuffer(b, dtype=np.uint8)
            ctx.ticket_wait(ctx.scan_pinned_many(others, pin, len(b), 2))
        tickets = []
        for b, out, odd in zip(batches, outs, odds):       # the new entry: column 3 (on return `pin` has been read)
            pin[:len(b)] = np.frombuffer(b, dtype=np.uint8)
            out[:] = 0xEE
            odd[:4] = 0xEE
            tickets.append(ctx.scan_pinned_pack_many(others, pin, len(b), 3, out, odd))
        for t in tickets:
            ctx.pack_ticket_wait(t)
        for c in [ctx] + others:
            assert np.array_equal(c.counts(3), c.counts(2)) and int(c.counts(2).sum()) > 1000
        for i, (b, out, odd) in enumerate(zip(batches, outs, odds)):
            want, want_odd = native.pack_stream(b)
            assert bool(odd[:4].view(np.uint32)[0]) == bool(want_odd) == (i == 2)
            assert np.array_equal(out[:want.size], want)
            assert (out[want.size:] == 0xEE).all()
        for a in [pin] + outs + odds:
            ctx.pinned_free(a)
    finally:
        for o in others:
            o.close()


# ---- the programs ----------------------------------------------------------------------------------------------------------------
def _env(**kw):
    e = {k: v for k, v in os.environ.items() if not k.startswith("SK_")}
    e.update(SK_CHUNK_BYTES="4096", SK_THREADS="4")
    e.update(kw)
    return e


def _run(argv, cwd, exe=EXE, **env):
    return subprocess.run([exe] + argv, cwd=str(cwd), env=_env(**env), capture_output=True, timeout=300)


def _stats(p):
    rows = STAT.findall(p.stderr)
    return tuple(sum(int(r[i]) for r in rows) for i in range(4))


def _quiet(stderr):
    return b"".join(l for l in stderr.splitlines(True) if not l.startswith((b"kmer_scrub_count timing:", b"key set of ")))


@pytest.mark.parametrize("name", CASES)
def test_program_on_the_golden_cases(golden, name, tmp_path):
    d = os.path.join(golden, "cases", name)
    meta = json.load(open(os.path.join(d, "case.json")))
    want_out = open(os.path.join(d, "expected.stdout"), "rb").read()
    want_err = open(os.path.join(d, "expected.stderr"), "rb").read()
    # (a job that stops at a missing file: with several decode threads, which later items were taken meanwhile differs from run to
    # run -- one thread, the reference's strict sequence, makes what the first run wrote a fact)
    threads = "4" if meta["returncode"] == 0 else "1"
    for pack in ("0", "2"):
        cache = tmp_path / ("cache" + pack)
        seen = []
        for tag in ("fill", "serve"):
            prog = str(tmp_path / ("progress_" + pack + tag))
            argv = [a if a not in ("progress.txt", "prog.txt") else prog for a in meta["argv"]]
            p = _run(argv, d, SK_PACK_CACHE=str(cache), SK_LIST_PACK=pack, SK_TIMING="1", SK_THREADS=threads)
            assert p.returncode == meta["returncode"], p.stderr.decode()[-2000:]
            assert p.stdout == want_out and _quiet(p.stderr) == want_err
            if meta["progress_col1"] is not None:
                assert [l.split("\t")[0] for l in open(prog).read().splitlines()] == meta["progress_col1"]
            seen.append(_stats(p))
        (s0, w0, st0, n0), (s1, w1, st1, n1) = seen
        assert (st0, n0, st1, n1, w1) == (0, 0, 0, 0, 0) and s1 == s0 + w0
        if meta["returncode"] == 0:
            assert w0 >= 1
        assert all(f.endswith(".skp") for f in os.listdir(cache)) if os.path.isdir(cache) else w0 == 0


@pytest.fixture(scope="module")
def fuzz_worlds(tmp_path_factory):
    """three random worlds, each with its lists in plain and in .gz form, and what the oracle prints for them"""
    out = []
    for seed in (11, 12, 13):
        d = tmp_path_factory.mktemp("pcw%d" % seed)
        argv = _synth.oracle_fuzz_world(seed, str(d))
        for lst in ("A.txt", "B.txt"):
            names = open(d / lst).read().split()
            for n in names:
                with open(d / n, "rb") as f, gzip.open(d / (n + ".gz"), "wb") as g:
                    g.write(f.read())
            (d / ("gz_" + lst)).write_text("".join(n + ".gz\n" for n in names))
        want = subprocess.run([ORACLE] + argv, cwd=str(d), capture_output=True, timeout=300)
        assert want.returncode == 0
        out.append((d, argv, want.stdout))
    return out


@pytest.mark.parametrize("form", ["plain", "gz"])
@pytest.mark.parametrize("pack", ["0", "2"])
def test_program_on_random_worlds_against_the_oracle(fuzz_worlds, form, pack):
    for d, argv, want in fuzz_worlds:
        if form == "gz":
            argv = ["-r", "strain.fa", "-A", "gz_A.txt", "-B", "gz_B.txt"]
        cache = d / ("cache_%s_%s" % (form, pack))
        fill = _run(argv, d, SK_PACK_CACHE=str(cache), SK_LIST_PACK=pack, SK_TIMING="1")
        serve = _run(argv, d, SK_PACK_CACHE=str(cache), SK_LIST_PACK=pack, SK_TIMING="1")
        assert (fill.returncode, fill.stdout) == (0, want), fill.stderr.decode()[-2000:]
        assert (serve.returncode, serve.stdout) == (0, want), serve.stderr.decode()[-2000:]
        assert _stats(fill) == (0, 3, 0, 0) and _stats(serve) == (3, 0, 0, 0)
        assert _quiet(fill.stderr) == _quiet(serve.stderr)


def test_scrub_multi_with_two_unions(tmp_path):
    """-S: four strains in two unions fed by one decode of the lists; every outfile the same with the cache off, filled, served"""
    rng = random.Random(5)
    base = _synth.rand_dna(rng, 9000)
    for s in range(4):
        g = bytearray(base if s % 2 == 0 else _synth.revcomp(base[2000:]) + _synth.rand_dna(rng, 700))
        for at in rng.sample(range(len(g)), 40):
            g[at] = rng.choice(b"ACGT")
        (tmp_path / ("s%d.fa" % s)).write_bytes(b">s%d\n" % s + bytes(g) + b"\n")
    reads = _synth.fuzz_stream(rng, base, 1500, p_junk=0.01, min_len=0, max_len=220).split(b"\n")[:-1]
    (tmp_path / "m1.fa").write_bytes(b"".join(b">r%d\n%s\n" % (i, r.replace(b"\r", b"A")) for i, r in enumerate(reads[:700])))
    with gzip.open(tmp_path / "m2.fq.gz", "wb") as f:
        f.write(b"".join(b"@q%d\n%s\n+\n%s\n" % (i, r.replace(b"\r", b"A"), b"I" * len(r)) for i, r in enumerate(reads[700:]) if r))
    (tmp_path / "A.txt").write_text("m1.fa\ns1.fa\n")
    (tmp_path / "B.txt").write_text("m2.fq.gz\nm1.fa\n")
    (tmp_path / "C.txt").write_text("s1.fa\nm2.fq.gz\n")
    got = {}
    for tag in ("off", "fill", "serve"):
        (tmp_path / "S.txt").write_text("".join("s%d.fa\t%s_%d.tsv\n" % (s, tag, s) for s in range(4)))
        extra = {} if tag == "off" else {"SK_PACK_CACHE": str(tmp_path / "cache")}
        argv = ["-S", "S.txt", "-A", "A.txt", "-B", "B.txt", "-C", "C.txt", "-p", tag + ".progress"]
        p = _run(argv, tmp_path, SK_SCRUB_GROUP="2", SK_TIMING="1", **extra)
        assert p.returncode == 0, p.stderr.decode()[-2000:]
        got[tag] = ([(tmp_path / ("%s_%d.tsv" % (tag, s))).read_bytes() for s in range(4)], p.stdout,
                    [l.split("\t")[0] for l in open(tmp_path / (tag + ".progress")).read().splitlines()], _stats(p))
        assert all(len(t) > 1000 for t in got[tag][0])
    assert got["off"][:3] == got["fill"][:3] == got["serve"][:3]
    assert got["off"][3] == (0, 0, 0, 0)
    assert got["fill"][3][1] >= 3 and got["fill"][3][2:] == (0, 0)
    assert got["serve"][3][1:] == (0, 0, 0) and got["serve"][3][0] == sum(got["fill"][3][:2])
    # the switch on the command line, for this main too
    (tmp_path / "S.txt").write_text("".join("s%d.fa\tcli_%d.tsv\n" % (s, s) for s in range(4)))
    p = _run(["-S", "S.txt", "--pack-cache", str(tmp_path / "cache"), "-A", "A.txt", "-B", "B.txt", "-C", "C.txt"], tmp_path, SK_SCRUB_GROUP="2", SK_TIMING="1")
    assert p.returncode == 0 and _stats(p) == got["serve"][3]
    assert [(tmp_path / ("cli_%d.tsv" % s)).read_bytes() for s in range(4)] == got["off"][0]


def test_context_switch_stats_and_what_is_not_cached(world, tmp_path, monkeypatch):
    """skh_pack_cache_set / skh_pack_cache_stats through the Python wrapper: a .gz item packed by the device while it is filled, a
    served item never sent to the device text parser, and the items that are not written -- cut into ranges, taken by the text parser"""
    ctx, _ks, strain = world
    rng = random.Random(9)
    reads = _synth.fuzz_stream(rng, strain, 6000, junk=b"NnRY\r", p_junk=0.002, min_len=20, max_len=300).split(b"\n")[:-1]
    (tmp_path / "a.fa").write_bytes(b"".join(b">r%d\n%s\n" % (i, r.replace(b"\r", b"A")) for i, r in enumerate(reads[:3000])))
    with gzip.open(tmp_path / "b.fa.gz", "wb") as f:
        f.write(b"".join(b">r%d\n%s\n" % (i, r.replace(b"\r", b"A")) for i, r in enumerate(reads[3000:])))
    lst = tmp_path / "list.txt"
    lst.write_text("%s\n%s\n" % (tmp_path / "a.fa", tmp_path / "b.fa.gz"))
    for k in [k for k in os.environ if k.startswith("SK_")]:
        monkeypatch.delenv(k)
    monkeypatch.setenv("SK_CHUNK_BYTES", "65536")
    monkeypatch.setenv("SK_THREADS", "4")
    monkeypatch.setenv("SK_NO_SPLIT", "1")

    def scan():
        ctx.zero_counts(1)
        bases = ctx.scan_list(str(lst), 1)
        return bases, ctx.counts(1).copy()
    want = scan()
    assert int(want[1].sum()) > 1000 and ctx.pack_cache_stats() == (0, 0, 0, 0)
    try:
        ctx.pack_cache(str(tmp_path / "cache"))
        fill = scan()
        assert ctx.pack_cache_stats(reset=True) == (0, 2, 0, 0)
        serve = scan()
        assert ctx.pack_cache_stats(reset=True) == (2, 0, 0, 0)
        ctx.set_option("device_parse", 1)                  # a cached item is served whatever the text parser would take
        ctx.text_stats(reset=True)
        served_text = scan()
        assert ctx.pack_cache_stats(reset=True) == (2, 0, 0, 0) and ctx.text_stats()[0] == 0
        for got in (fill, serve, served_text):
            assert got[0] == want[0] and np.array_equal(got[1], want[1])
        # what the text parser takes is not written: a.fa goes to it, b.fa.gz is the host's
        ctx.pack_cache(str(tmp_path / "cache_text"))
        got = scan()
        assert got[0] == want[0] and np.array_equal(got[1], want[1])
        assert ctx.pack_cache_stats(reset=True) == (0, 1, 0, 1) and ctx.text_stats()[0] >= 1
        assert [f.split(".")[0] for f in os.listdir(tmp_path / "cache_text")] == ["b"]
        ctx.set_option("device_parse", 0)
        # an item the plan cuts into byte ranges is not written either
        monkeypatch.delenv("SK_NO_SPLIT")
        monkeypatch.setenv("SK_SPLIT_BYTES", "100000")
        ctx.pack_cache(str(tmp_path / "cache_cut"))
        got = scan()
        assert got[0] == want[0] and np.array_equal(got[1], want[1])
        assert ctx.pack_cache_stats(reset=True) == (0, 1, 0, 1)
        # ... and served whole once it has a file: ro mode on the first directory
        ctx.pack_cache(str(tmp_path / "cache"), "ro")
        got = scan()
        assert np.array_equal(got[1], want[1]) and ctx.pack_cache_stats(reset=True) == (2, 0, 0, 0)
        # scan_file goes the same way
        ctx.zero_counts(2)
        b_off = None
        ctx.pack_cache("")
        b_off = ctx.scan_file(str(tmp_path / "b.fa.gz"), 2)
        c_off = ctx.counts(2).copy()
        ctx.pack_cache(str(tmp_path / "cache"), "ro")
        ctx.zero_counts(2)
        assert ctx.scan_file(str(tmp_path / "b.fa.gz"), 2) == b_off and np.array_equal(ctx.counts(2), c_off)
        assert ctx.pack_cache_stats(reset=True) == (1, 0, 0, 0)
    finally:
        ctx.set_option("device_parse", 0)
        ctx.pack_cache(None)
