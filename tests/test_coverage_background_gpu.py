"""The background of step 4's numbers on the device (include/strainer_kmer.h has the rule): sk_scan_batch against sk_scan_stream row by
row in every batch form, the finishing sweep of one context on crafted columns, the union's sweep against per-member scans into plain
contexts, and strain_detect --coverage-background in the forms it runs in -- against kmer_scrub_count run with the target's files as
its -B list (another host path), against the model (tests/_background_model.py), and against the tables that already exist."""
import gzip
import os
import random
import zlib

import numpy as np
import pytest

import _background_model as model
import _synth
import strainer2_amd as sk
from strainer2_amd import native

pytestmark = pytest.mark.gpu

HEAD = model.HEAD
SK_E_ARG, SK_E_STATE = -3, -7
# background_sweep runs at most 256 workgroups of 256 threads (sk_background.hip): 70 001 rows are more than one turn of its loop
SIZES = [1, 255, 257, 70001]


def _mutate(rng, seq, rate):
    b = bytearray(seq)
    for i in range(len(b)):
        if rng.random() < rate:
            b[i] = rng.choice(b"ACGT")
    return bytes(b)


def _starts(recs):
    return np.cumsum([0] + [len(r) + 1 for r in recs[:-1]]).astype(np.uint32)


def _fa(reads):
    return b"".join(b">r%d\n%s\n" % (i, x) for i, x in enumerate(reads))


def _fq(reads):
    return b"".join(b"@r%d\n%s\n+\n%s\n" % (i, x, b"I" * len(x)) for i, x in enumerate(reads))


# ---------------------------------------------------------------------------------------------------------------------------------
# sk_scan_batch against sk_scan_stream, per row
# ---------------------------------------------------------------------------------------------------------------------------------
class Strain:
    pass


@pytest.fixture(scope="module")
def plain():
    """a strain of 9 000 bases (pure A/C/G/T and one N) with its text stage, four columns"""
    rng = random.Random(77)
    s = Strain()
    g = bytearray(_synth.rand_dna(rng, 9000))
    g[4000] = ord("N")
    s.g = bytes(g)
    s.ks = sk.Keyset.from_stream(s.g + b"\n", default_val=1, incr=0)
    s.ctx = sk.KmerContext(0)
    s.ctx.load_keyset(s.ks, 4)
    s.batch = native.TallyBatch(s.ctx)
    yield s
    s.batch.close()
    s.ctx.close()
    s.ks.close()


@pytest.fixture(scope="module")
def wide():
    """a strain with byte-string keys: an R and a Y in its text"""
    rng = random.Random(78)
    s = Strain()
    g = bytearray(_synth.rand_dna(rng, 2500))
    g[700], g[1600] = ord("R"), ord("Y")
    s.g = bytes(g)
    s.ks = sk.Keyset.from_stream(s.g + b"\n", default_val=1, incr=0)
    assert s.ks.nwide > 0
    s.ctx = sk.KmerContext(0)
    s.ctx.load_keyset(s.ks, 4)
    s.batch = native.TallyBatch(s.ctx)
    yield s
    s.batch.close()
    s.ctx.close()
    s.ks.close()


def _pieces(rng, g, n, ln=100):
    out = []
    for _ in range(n):
        a = rng.randrange(len(g) - ln)
        r = g[a:a + ln]
        out.append(_synth.revcomp(r) if rng.random() < 0.5 and b"R" not in r and b"Y" not in r else r)
    return out


def _stream_of(rng, g, nbytes, long_nl=None):
    """records of the strain whose stream has exactly nbytes: records of 100 bases, then a long one (1 300 bases or more) whose
    newline is byte long_nl (default: the stream's last byte), then records of 100 bases again and a last one that fills the stream"""
    long_nl = nbytes - 1 if long_nl is None else long_nl
    recs, total = [], 0
    while long_nl - total > 1400:
        recs.append(_pieces(rng, g, 1)[0])
        total += 101
    a = rng.randrange(len(g) - (long_nl - total))
    recs.append(g[a:a + long_nl - total])
    long_at = len(recs) - 1
    total = long_nl + 1
    while nbytes - total > 250:
        recs.append(_pieces(rng, g, 1)[0])
        total += 101
    if nbytes > total:
        a = rng.randrange(len(g) - 300)
        recs.append(g[a:a + nbytes - total - 1])
    starts = _starts(recs)
    assert sum(len(r) + 1 for r in recs) == nbytes and len(recs[long_at]) >= 1300 and int(starts[long_at]) + len(recs[long_at]) == long_nl
    return recs


def _worlds(s):
    rng = random.Random(5)
    g = s.g.replace(b"N", b"A")
    w = {
        "one_record_of_31": [g[100:131]],
        "one_record_of_30": [g[100:130]],
        "n_every_31": [bytes(b"N"[0] if i % 31 == 30 else c for i, c in enumerate(g[2000:2400]))],     # every window holds an N
        "n_every_32": [bytes(b"N"[0] if i % 32 == 31 else c for i, c in enumerate(g[2000:2400]))],     # one window between two N
        "lower_case_and_short": [g[10:200].lower(), g[300:320], g[500:531], _synth.revcomp(g[600:700]).lower()],
    }
    for nbytes in (32767, 32768, 32769):                       # the stream ends one byte before, at, and one byte behind the 2^15 tile edge
        w["stream_of_%d" % nbytes] = _stream_of(rng, g, nbytes)
    for beyond in (1, 15, 31, 700):                            # a long record straddles the edge: `beyond` of its bases lie behind it
        w["straddle_%d" % beyond] = _stream_of(rng, g, 40000, 32768 + beyond)
    w["stream_of_70000"] = _stream_of(rng, g, 70000, 65536 + 200)   # ... and the second edge
    return w


FORMS = ["bytes", "packed", "fasta", "fastq"]


def _fill(batch, recs, form):
    stream = b"\n".join(recs) + b"\n"
    if form in ("bytes", "packed"):
        batch.fill(stream, _starts(recs), packed=form == "packed")
        return
    info, starts = batch.fill_text(_fa(recs) if form == "fasta" else _fq(recs))
    assert info.status == native.SK_TEXT_OK and int(info.nrecords) == len(recs) and int(info.stream_bytes) == len(stream)


@pytest.mark.parametrize("form", FORMS)
def test_scan_batch_counts_what_scan_stream_counts(plain, form):
    s = plain
    for name, recs in _worlds(s).items():
        stream = b"\n".join(recs) + b"\n"
        s.ctx.zero_counts(1)
        s.ctx.zero_counts(2)
        s.ctx.scan_stream(stream, 1)
        _fill(s.batch, recs, form)
        s.ctx.scan_batch(s.batch, 2)
        s.ctx.sync()
        want, got = s.ctx.counts(1), s.ctx.counts(2)
        assert np.array_equal(got, want), (name, int(got.sum()), int(want.sum()))
        if len(stream) < 2000:                                 # (the small worlds: the model's counts as well)
            assert np.array_equal(want.astype(np.uint64), model.row_counts(s.ks.keys(), recs)), name
        if name in ("one_record_of_30", "n_every_31"):
            assert not got.any()
        elif name in ("one_record_of_31", "n_every_32"):
            assert int(got.sum()) == (1 if name == "one_record_of_31" else 12)
        else:
            assert int(got.sum()) > 0, name
        s.ctx.scan_batch(s.batch, 2)                           # once more into the same column: twice the counts
        s.ctx.sync()
        assert np.array_equal(s.ctx.counts(2), 2 * want), name


@pytest.mark.parametrize("form", ["bytes", "fasta", "fastq"])
def test_scan_batch_on_byte_string_keys(wide, form):
    s = wide
    rng = random.Random(9)
    recs = _pieces(rng, s.g, 150) + [s.g[680:720], s.g[1590:1621], s.g[690:711].lower() + s.g[711:760], s.g[660:700]]
    stream = b"\n".join(recs) + b"\n"
    s.ctx.zero_counts(1)
    s.ctx.zero_counts(2)
    s.ctx.scan_stream(stream, 1)
    _fill(s.batch, recs, form)
    s.ctx.scan_batch(s.batch, 2)
    s.ctx.sync()
    want = s.ctx.counts(1)
    assert np.array_equal(s.ctx.counts(2), want)
    assert np.array_equal(want.astype(np.uint64), model.row_counts(s.ks.keys(), recs))
    wide_rows = [i for i, k in enumerate(s.ks.keys()) if b"R" in k or b"Y" in k]
    assert want[wide_rows].sum() > 0, "no window fell on a byte-string key: this world tests nothing"


def test_a_count_scan_spares_the_tally_bitmap_unless_it_writes_the_type_column(plain):
    """sk_launch_scan drops the informative-row bitmap of the TALLY scan only when the count scan writes the column the bitmap was
    made from: TALLY, a count scan into another column, TALLY again -- the same; a count scan into the TYPE column -- the TALLY
    that follows sees the new types, as a fresh context with those types does"""
    s = plain
    rng = random.Random(3)
    recs = _pieces(rng, s.g.replace(b"N", b"A"), 300)
    stream, starts = b"\n".join(recs) + b"\n", _starts(recs)
    typ = np.ones(s.ctx.nrows, dtype=np.uint32)
    typ[::5] = 2
    try:
        s.ctx.set_counts(0, typ)
        t0, h0 = s.ctx.tally_batch(stream, starts, 0, 2)
        assert int(t0[:, 1].sum()) > 0
        s.ctx.zero_counts(2)
        s.batch.fill(stream, starts)
        s.ctx.scan_batch(s.batch, 2)                           # another column: the bitmap stands
        s.ctx.scan_stream(stream, 2)
        t1, h1 = s.ctx.tally_batch(stream, starts, 0, 2)
        assert np.array_equal(t0, t1) and np.array_equal(h0, h1)
        s.ctx.scan_batch(s.batch, 0)                           # the type column itself: rows that were hit once turn informative, informative ones plain
        s.ctx.sync()
        changed = s.ctx.counts(0)
        assert not np.array_equal(changed, typ)
        t2, h2 = s.ctx.tally_batch(stream, starts, 0, 2)
        with sk.KmerContext(0) as fresh:
            fresh.load_keyset(s.ks, 4)
            fresh.set_counts(0, changed)
            t3, h3 = fresh.tally_batch(stream, starts, 0, 2)
        assert np.array_equal(t2, t3) and np.array_equal(h2, h3)
        assert not np.array_equal(t2, t0)
    finally:
        s.ctx.set_counts(0, np.ones(s.ctx.nrows, dtype=np.uint32))


def test_scan_batch_refusals(plain):
    s = plain
    _fill(s.batch, [s.g[:100]], "bytes")
    with pytest.raises(sk.SKError) as e:
        s.ctx.scan_batch(s.batch, 4)
    assert e.value.code == SK_E_ARG
    with native.TallyBatch(s.ctx) as empty:
        with pytest.raises(sk.SKError) as e:
            s.ctx.scan_batch(empty, 2)
        assert e.value.code == SK_E_STATE
        info, _ = empty.fill_text(b"no record here\n")
        assert info.status == native.SK_TEXT_DECLINED
        with pytest.raises(sk.SKError) as e:
            s.ctx.scan_batch(empty, 2)
        assert e.value.code == SK_E_STATE
    with sk.KmerContext(0) as bare:
        with pytest.raises(sk.SKError) as e:
            bare.scan_batch(s.batch, 0)
        assert e.value.code == SK_E_STATE
    with sk.KmerUnion([s.ctx], 0, 2) as u:                     # a union's context without count columns
        with pytest.raises(sk.SKError) as e:
            u.scan_batch(s.batch, 0)
        assert e.value.code == SK_E_STATE


# ---------------------------------------------------------------------------------------------------------------------------------
# the sweep on crafted columns
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tables():
    """contexts of exactly 1, 255, 257 and 70 001 rows, three columns: 0 the type, 2 the counts"""
    rng = random.Random(4242)
    out, sets = {}, []
    for n in SIZES:
        ks = sk.Keyset.from_stream(_synth.rand_dna(rng, n + 30) + b"\n", default_val=1, incr=0)
        assert ks.nrows == n
        c = sk.KmerContext(0)
        c.load_keyset(ks, 3)
        sets.append(ks)
        out[n] = c
    yield out
    for c in out.values():
        c.close()
    for ks in sets:
        ks.close()


def _sweep(c, counts, inf, D):
    n = c.nrows
    typ = np.ones(n, dtype=np.uint32)
    typ[np.asarray(inf, dtype=bool)] = 2
    c.set_counts(0, typ)
    c.set_counts(2, counts)
    got = c.background_finish(2, 0, 2, D)
    want = model.block(counts, inf, D)
    assert got.dtype == np.uint64 and got.shape == want.shape
    assert np.array_equal(got, want), (n, D, got[:, :HEAD + 3].tolist(), want[:, :HEAD + 3].tolist())
    model.check_block(got)
    assert not c.counts(2).any(), "the column is zero afterwards"
    again = c.background_finish(2, 0, 2, D)                    # a second call returns kmers and zeros
    assert np.array_equal(again, model.block(np.zeros(n, np.uint32), inf, D))
    assert np.array_equal(c.counts(0), typ), "the type column is untouched"
    return got


@pytest.mark.parametrize("D", [1, 2, 63, 255])
def test_sweep_depths_around_the_maximum(tables, D):
    rng = np.random.default_rng(D)
    for n in SIZES:
        counts = np.zeros(n, dtype=np.uint32)
        if n > 8:
            some = rng.choice(n, n // 3, replace=False)
            counts[some] = rng.integers(1, 2 * D + 3, len(some))
        edge = [D - 1, D, D + 1, 70000, 2**32 - 1, 2**32 - 1]
        at = [0, n // 5, n // 3, n // 2, n - 2, n - 1]
        for k in range(min(n, 6)):
            counts[at[k] if n >= 6 else k] = edge[k]
        inf = rng.random(n) < 0.05
        if n > 8:
            inf[[0, n // 3, n - 1]] = True                     # depths D - 1, D + 1 and 2^32 - 1 in the informative class ...
            inf[[n // 5, n // 2, n - 2]] = False               # ... D, 70 000 and another 2^32 - 1 in the background
        got = _sweep(tables[n], counts, inf, D)
        if n > 8:
            assert int(got[0, 2]) > 2**32 and int(got[1, 2]) > 2**32, "total_hits needs its 64 bits"
            assert int(got[1, 3]) >= 2 and int(got[1, 4]) >= 70000 + 2**32 - 1


def test_sweep_no_row_every_row_and_the_last_row_informative(tables):
    rng = np.random.default_rng(11)
    for n in SIZES:
        counts = rng.integers(0, 9, n).astype(np.uint32)
        last = np.zeros(n, bool)
        last[-1] = True
        for inf in (np.zeros(n, bool), np.ones(n, bool), last):
            got = _sweep(tables[n], counts, inf, 3)
            assert int(got[0, 0]) == int(inf.sum()) and int(got[1, 0]) == n - int(inf.sum())


def test_sweep_every_covered_row_at_depth_one(tables):
    """all LDS adds of a class on one bin"""
    for n in SIZES:
        inf = np.arange(n) % 3 == 0
        got = _sweep(tables[n], np.ones(n, dtype=np.uint32), inf, 2)
        assert got[:, HEAD + 1].tolist() == [int(inf.sum()), n - int(inf.sum())] and not got[:, 3:HEAD + 1].any()
        _sweep(tables[n], np.zeros(n, dtype=np.uint32), inf, 2)


def test_sweep_bad_calls(tables):
    c = tables[257]
    for args in ((2, 0, 2, 256), (2, 2, 2, 3), (3, 0, 2, 3), (2, 3, 2, 3)):
        with pytest.raises(sk.SKError) as e:
            c.background_finish(*args)
        assert e.value.code == SK_E_ARG, args


# ---------------------------------------------------------------------------------------------------------------------------------
# the union's sweep
# ---------------------------------------------------------------------------------------------------------------------------------
def _panel(rng, n):
    """n related strains: mutated copies of one base with a piece every member holds unchanged, and a tail of their own"""
    base = _synth.rand_dna(rng, 1500)
    common = _synth.rand_dna(rng, 80)
    return [_mutate(rng, base, [0.0, 0.004, 0.02, 0.05][s % 4]) + b"\n" + common + b"\n" + _synth.rand_dna(rng, 40 + 11 * s) for s in range(n)], common


def _panel_reads(rng, strains, common, n=500):
    recs = []
    for i in range(n):
        g = strains[rng.randrange(len(strains))].replace(b"\n", b"")
        ln = rng.choice([31, 50, 100, 150])
        a = rng.randrange(len(g) - ln)
        r = g[a:a + ln]
        if i % 11 == 0:
            r = r.lower()
        if i % 13 == 0:
            r = r[:ln // 2] + b"N" + r[ln // 2 + 1:]
        recs.append(_synth.revcomp(r) if i % 2 else r)
    return recs + [common] * 5 + [_synth.rand_dna(rng, 90) for _ in range(50)]


@pytest.mark.parametrize("n,D", [(2, 3), (3, 63), (32, 255), (32, 1)])
def test_union_sweep_against_per_member_scans(n, D):
    rng = random.Random(100 * n + D)
    strains, common = _panel(rng, n)
    recs = _panel_reads(rng, strains, common)
    stream = b"\n".join(recs) + b"\n"
    ckeys = {model.key_of(common[i:i + 31]) for i in range(len(common) - 30)}
    ctxs, sets, want, infs, keysets = [], [], [], [], []
    try:
        for s, g in enumerate(strains):
            ks = sk.Keyset.from_stream(g + b"\n", default_val=1, incr=0)
            sets.append(ks)
            c = sk.KmerContext(0)
            ctxs.append(c)
            c.load_keyset(ks, 6)
            keys = ks.keys()
            # a key informative in the even members and background in the odd ones; the common piece informative in member 0 only
            inf = np.array([(zlib.crc32(k) % 7 == 0 and s % 2 == 0) or (k in ckeys and s == 0) for k in keys])
            typ = np.ones(len(keys), dtype=np.uint32)
            typ[inf] = 2
            c.set_counts(0, typ)
            c.scan_stream(stream, 2)                           # the member's own plain scan
            want.append(model.block(c.counts(2), inf, D))
            infs.append({k for k, f in zip(keys, inf) if f})
            keysets.append(set(keys))
        assert all(ckeys <= k for k in keysets), "a key every member holds"
        if n > 1:
            assert infs[0] & (keysets[1] - infs[1]), "a shared key informative in one holder and background in another"
        with sk.KmerUnion(ctxs, 0, 2) as fresh, sk.KmerUnion(ctxs, 0, 2) as u, native.TallyBatch(ctxs[0]) as batch:
            t0, h0 = fresh.tally_batch(stream, _starts(recs))
            u.count_enable(1)
            batch.fill(stream, _starts(recs))
            u.scan_batch(batch, 0)
            t1, h1 = u.tally_filled(batch)                     # a TALLY launch on the count-enabled union, a count scan pending
            assert np.array_equal(t0, t1) and np.array_equal(h0, h1)
            got = u.background_finish(0, D)
            assert got.shape == (n, 2, HEAD + D + 1)
            for s in range(n):
                assert np.array_equal(got[s], want[s]), (s, got[s][:, :HEAD + 2].tolist(), want[s][:, :HEAD + 2].tolist())
                model.check_block(got[s])
                # the records' "all" tallies of a TALLY of the same reads add up to the member's hits, both classes together
                assert int(t1[:, s, 0].sum()) == int(got[s][0, 2]) + int(got[s][1, 2])
            assert not u.counts(0).any(), "the union's column is zero afterwards"
            zeros = u.background_finish(0, D)                  # a second call: kmers and zeros
            for s in range(n):
                assert np.array_equal(zeros[s], model.block(np.zeros(sets[s].nrows, np.uint32), ctxs[s].counts(0) == 2, D))
            batch.fill(stream, _starts(recs), packed=True)
            u.scan_batch(batch, 0)                             # the packed form, twice, and a host stream on top
            u.scan_batch(batch, 0)
            u.scan_stream(stream, 0)
            three = u.background_finish(0, D)
            for s in range(n):
                assert np.array_equal(three[s], model.block(3 * ctxs[s].counts(2).astype(np.uint64), ctxs[s].counts(0) == 2, D)), s
            for s in range(n):                                 # nothing was folded into the members' columns
                assert not ctxs[s].counts(1).any() and not ctxs[s].counts(3).any()
            t2, h2 = u.tally_filled(batch)
            assert np.array_equal(t0, t2) and np.array_equal(h0, h2)
            with pytest.raises(sk.SKError):
                u.background_finish(0, 256)
            with pytest.raises(sk.SKError):
                u.background_finish(1, 3)
        with sk.KmerUnion(ctxs[:1], 0, 2) as bare:
            with pytest.raises(sk.SKError) as e:
                bare.background_finish(0, 3)
            assert e.value.code == SK_E_STATE
    finally:
        for c in ctxs:
            c.close()
        for k in sets:
            k.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# the programs
# ---------------------------------------------------------------------------------------------------------------------------------
NAME = "Genus_species_st%d.kmer_hits.gz"
SMALL = {"SK_SD_CHUNK_BYTES": "6000"}                          # several chunks per file
SUFFIXES = ("coverage_background", "coverage_background_spectrum", "coverage_depth", "kmer_hits.gz")


class Job:
    pass


def _env_run(fn, argv, env, out, err):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        rc = fn(argv, str(out), str(err))
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return rc, open(out, "rb").read(), open(err, "rb").read()


@pytest.fixture(scope="module")
def job(tmp_path_factory):
    """36 strains: 0-2 of 400, 3 000 and 12 000 bases (1 and 2 related), 3-35 small mutated copies of one base (two unions' worth).
    Targets: SE (.gz FASTQ, reads shorter than k, a block read 40 times), PE over two plain FASTQ files (PE2 holds reads beyond
    PE1's last: missing mates), PEI (plain FASTA, an odd number of records: the last read has no mate), and a clean SE target whose reads all have k bases."""
    d = tmp_path_factory.mktemp("covbackground")
    rng = random.Random(20261020)
    j = Job()
    j.d = d
    g1 = _synth.rand_dna(rng, 12000)
    small = _synth.rand_dna(rng, 700)
    j.strains = [_synth.rand_dna(rng, 400), g1[:3000] + _synth.rand_dna(rng, 100), _mutate(rng, g1, 0.01)]
    j.strains += [_mutate(rng, small, 0.01 * (s % 5)) + _synth.rand_dna(rng, 35 + s) for s in range(33)]
    j.inf = []
    for s, g in enumerate(j.strains):
        (d / f"s{s}.fa").write_bytes(b">s%d\n%s\n" % (s, g))
        kms = sorted({model.key_of(g[i:i + 31]) for i in range(s % 7, len(g) - 31, 37)} | {model.key_of(g[i:i + 31]) for i in range(200, 230)})
        j.inf.append(set(kms))
        with gzip.open(d / f"s{s}.inf.gz", "wb") as f:
            f.write(b"#informative\n" + b"\n".join(kms) + b"\n")

    def reads(n, seed, short_every=0, pool=[0, 1, 2] * 8 + list(range(3, 36))):
        r = random.Random(seed)
        out = []
        for i in range(n):
            ln = r.choice([31, 31, 75, 100, 150, r.randrange(31, 151)])
            if r.random() < 0.6:
                g = j.strains[r.choice(pool)]
                ln = min(ln, len(g) - 1)
                a = r.randrange(0, len(g) - ln)
                rd = g[a:a + ln]
                rd = _synth.revcomp(rd) if r.random() < 0.5 else rd
                if r.random() < 0.1:
                    rd = rd.lower()
                if r.random() < 0.05:
                    rd = rd[:ln // 2] + b"N" + rd[ln // 2 + 1:]
            else:
                rd = _synth.rand_dna(r, ln)
            out.append(rd)
            if short_every and i % short_every == short_every - 1:
                out.append(rd[: 5 + i % 25])                   # a read shorter than k behind it
        return out

    deep = [j.strains[1][150:300] if i % 2 else _synth.revcomp(j.strains[1][150:300]) for i in range(40)]
    j.files = {
        "se.fq.gz": reads(300, 1, short_every=40) + deep,
        "pe_1.fq": reads(200, 2, short_every=50),
        "pe_2.fq": reads(200, 3, short_every=50) + reads(150, 6),          # (as many as PE1 holds, then reads without a mate)
        "il.fa": reads(301, 4, short_every=70),
        "clean.fa": reads(250, 5) + deep[:6],
    }
    assert len(j.files["pe_2.fq"]) == len(j.files["pe_1.fq"]) + 150
    if len(j.files["il.fa"]) % 2 == 0:
        j.files["il.fa"].append(_synth.rand_dna(rng, 60))
    for name, recs in j.files.items():
        raw = _fq(recs) if ".fq" in name else _fa(recs)
        if name.endswith(".gz"):
            with gzip.open(d / name, "wb", compresslevel=1) as f:
                f.write(raw)
        else:
            (d / name).write_bytes(raw)
    assert all(len(x) >= 31 for x in j.files["clean.fa"]) and any(len(x) < 31 for x in j.files["se.fq.gz"])
    j.targets = [("se.fq.gz", ["se.fq.gz"]), ("pe_1.fq", ["pe_1.fq", "pe_2.fq"]), ("il.fa", ["il.fa"])]
    (d / "T.txt").write_text(f"SE\t{d}/se.fq.gz\nPE\t{d}/pe_1.fq\t{d}/pe_2.fq\nPEI\t{d}/il.fa\n")
    (d / "clean.txt").write_text(f"SE\t{d}/clean.fa\n")
    (d / "other.fa").write_bytes(b">o\n" + _synth.rand_dna(rng, 200) + b"\n")
    (d / "A.txt").write_text(f"{d}/other.fa\n")
    j.expected = {}
    return j


def _expected(job, s, D=63):
    """strain s's blocks over T.txt's targets from kmer_scrub_count, the target's files as its -B list: the metagenome_count column,
    split by the -a list here"""
    if (s, D) in job.expected:
        return job.expected[s, D]
    d = job.d / f"ksc{s}_{D}"
    d.mkdir()
    blocks = []
    for first, files in job.targets:
        (d / "B.txt").write_text("".join(f"{job.d}/{f}\n" for f in files))
        rc, out, err = _env_run(native.run_cli_inprocess, ["-r", str(job.d / f"s{s}.fa"), "-A", str(job.d / "A.txt"), "-B", str(d / "B.txt")], {},
                                d / "out", d / "err")
        assert rc == 0, err.decode()[-400:]
        rows = [ln.split(b"\t") for ln in out.split(b"\n")[1:] if ln]
        counts = np.array([int(r[3]) for r in rows], dtype=np.uint64)
        inf = np.array([r[0] in job.inf[s] for r in rows])
        assert int(inf.sum()) == len(job.inf[s]) and len(rows) == len(model.strain_keys([job.strains[s]]))
        blocks.append((first, model.block(counts, inf, D)))
    job.expected[s, D] = blocks
    return blocks


def _run(job, tag, flags, strains=(0, 1, 2), targets="T.txt", env=None, ok=True):
    """one run of strain_detect: ({strain: {suffix: bytes or None}}, stdout, stderr)"""
    d = job.d / tag
    d.mkdir()
    if len(strains) > 1:
        (d / "S.txt").write_text("".join(f"{job.d}/s{s}.fa\t{job.d}/s{s}.inf.gz\t{d}/{NAME % s}\n" for s in strains))
        argv = ["-S", str(d / "S.txt")]
    else:
        s = strains[0]
        argv = ["-r", str(job.d / f"s{s}.fa"), "-a", str(job.d / f"s{s}.inf.gz"), "-o", str(d / (NAME % s))]
    rc, out, err = _env_run(native.run_strain_detect_inprocess, argv + ["-B", str(job.d / targets)] + flags, dict(SMALL, **(env or {})), d / "run.out", d / "run.err")
    assert (rc == 0) == ok, err.decode()[-600:]
    files = {}
    for s in strains:
        b = str(d / (NAME % s))[: -len(".kmer_hits.gz")]
        files[s] = {x: (open(b + "." + x, "rb").read() if os.path.exists(b + "." + x) else None) for x in SUFFIXES}
    return files, out, err


BG = ["--coverage-background", "--background-spectrum"]


@pytest.fixture(scope="module")
def base(job):
    """three strains in one union under --coverage-only: the run every other form is compared with"""
    files, _, _ = _run(job, "base", ["--coverage-only"] + BG)
    return files


def _same_tables(a, b, strains):
    for s in strains:
        for x in SUFFIXES[:2]:
            assert a[s][x] is not None and a[s][x] == b[s][x], (s, x)


def test_tables_against_kmer_scrub_count_and_the_model(job, base):
    for s in (0, 1, 2):
        want = _expected(job, s)
        name = model.strain_name(NAME % s)
        assert base[s]["coverage_background"] == model.table(name, want), s
        assert base[s]["coverage_background_spectrum"] == model.spectrum(name, want), s
        model.blocks_of_tables(base[s]["coverage_background"], base[s]["coverage_background_spectrum"])
        for _, b in want:
            model.check_block(b)
    # ... and strain 1 over the PE target against the pure-Python model: every record of both files, paired or not, short or not
    keys = model.strain_keys([job.strains[1]])
    counts = model.row_counts(keys, job.files["pe_1.fq"] + job.files["pe_2.fq"])
    assert np.array_equal(model.block(counts, [k in job.inf[1] for k in keys], 63), _expected(job, 1)[1][1])
    t, _ = model.parse_table(base[1]["coverage_background"])
    deep_target = t[(model.strain_name(NAME % 1), "se.fq.gz", "background")]
    assert deep_target[1] > 100 and deep_target[2] > 40 * 100, "the block read 40 times shows in the background's hits"


def test_coverage_depth_writes_the_same_tables(job, base):
    files, _, _ = _run(job, "depth", ["--coverage-depth"] + BG)
    _same_tables(files, base, (0, 1, 2))
    assert all(files[s]["kmer_hits.gz"] for s in (0, 1, 2))


@pytest.mark.parametrize("tag,env", [("no_union", {"SK_SD_NO_UNION": "1"}), ("two_devices", {"SK_DEVICES": "0,0", "SK_SD_GROUP": "2"}),
                                     ("pack", {"SK_SD_PACK": "1"}), ("device_parse", {"SK_DEVICE_PARSE": "1"}),
                                     ("one_chunk", {"SK_SD_CHUNK_BYTES": str(32 << 20)})])
def test_every_run_form_writes_the_same_tables(job, base, tag, env):
    files, _, _ = _run(job, tag, ["--coverage-only"] + BG, env=env)
    _same_tables(files, base, (0, 1, 2))


def test_target_cache_filling_served_and_off(job, base):
    cache = job.d / "tcache"
    cache.mkdir()
    native.target_cache_stats(reset=True)
    filled, _, _ = _run(job, "tc_fill", ["--coverage-only", "--target-cache", str(cache)] + BG)
    assert native.target_cache_stats(reset=True)[1] > 0, "nothing was written to the cache"
    served, _, _ = _run(job, "tc_served", ["--coverage-only", "--target-cache", str(cache)] + BG)
    assert native.target_cache_stats(reset=True)[0] > 0, "nothing was served from the cache"
    _same_tables(filled, base, (0, 1, 2))
    _same_tables(served, base, (0, 1, 2))


def test_single_strain_with_named_files_and_a_small_depth(job):
    d = job.d
    files, _, _ = _run(job, "single", ["--coverage-depth", f"--coverage-background={d}/one.bg", f"--background-spectrum={d}/one.bgs", "--background-max", "2"],
                       strains=(1,))
    want = _expected(job, 1, D=2)
    name = model.strain_name(NAME % 1)
    assert files[1]["coverage_background"] is None
    assert (d / "one.bg").read_bytes() == model.table(name, want)
    assert (d / "one.bgs").read_bytes() == model.spectrum(name, want)
    assert any(int(b[1, 3]) > 0 for _, b in want), "no row deeper than 2: the '>D' line tests nothing"


def test_thirty_three_strains_two_unions_and_ranks(job):
    strains = tuple(range(3, 36))
    union, _, _ = _run(job, "u33", ["--coverage-only", "--coverage-background"], strains=strains)
    alone, _, _ = _run(job, "n33", ["--coverage-only", "--coverage-background"], strains=strains, env={"SK_SD_NO_UNION": "1"})
    for s in strains:
        assert union[s]["coverage_background"] == alone[s]["coverage_background"] and union[s]["coverage_background_spectrum"] is None
    for s in (3, 20, 35):                                      # (members of both unions)
        assert union[s]["coverage_background"] == model.table(model.strain_name(NAME % s), _expected(job, s)), s
    for rank in (0, 1):                                        # strains are dealt to the ranks: each writes its own strains' tables
        mine = tuple(s for i, s in enumerate(strains) if i % 2 == rank)
        d = job.d / f"rank{rank}"
        d.mkdir()
        (d / "S.txt").write_text("".join(f"{job.d}/s{s}.fa\t{job.d}/s{s}.inf.gz\t{d}/{NAME % s}\n" for s in strains))
        rc, _, err = _env_run(native.run_strain_detect_inprocess, ["-S", str(d / "S.txt"), "-B", str(job.d / "T.txt"), "--coverage-only", "--coverage-background"],
                              dict(SMALL, WORLD_SIZE="2", RANK=str(rank)), d / "o", d / "e")
        assert rc == 0, err.decode()[-400:]
        for s in strains:
            p = str(d / (NAME % s))[: -len(".kmer_hits.gz")] + ".coverage_background"
            assert os.path.exists(p) == (s in mine)
            if s in mine:
                assert open(p, "rb").read() == union[s]["coverage_background"]


def test_cross_checks_against_step_fours_table(job):
    """every read of the target has k bases and --min-kmer-hits is 0: the informative line is step 4's two columns"""
    files, _, _ = _run(job, "clean", ["--coverage-depth", "--min-kmer-hits", "0", "--coverage-background"], targets="clean.txt")
    for s in (0, 1, 2):
        t, _ = model.parse_table(files[s]["coverage_background"])
        kmers, covered, total = t[(model.strain_name(NAME % s), "clean.fa", "informative")]
        lines = files[s]["coverage_depth"].decode().split("\n")
        head, row = lines[0].split("\t"), lines[1].split("\t")
        assert int(row[head.index("unique_observed_informative_kmers")]) == covered, s
        assert int(row[head.index("total_observed_informative_kmers")]) == total, s
        assert int(row[head.index("genome_num_informative_kmers")]) == kmers == len(job.inf[s]), s
        both = kmers + t[(model.strain_name(NAME % s), "clean.fa", "background")][0]
        assert int(row[head.index("genome_num_total_kmers")]) == both, "informative + background kmers == table rows"
    assert any(model.parse_table(files[s]["coverage_background"])[0][(model.strain_name(NAME % s), "clean.fa", "informative")][1] for s in (0, 1, 2))


@pytest.mark.parametrize("table_flag,env", [("--coverage-only", {}), ("--coverage-depth", {}), ("--coverage-depth", {"SK_SD_NO_UNION": "1"})])
def test_flag_off_every_byte_is_the_same(job, table_flag, env):
    tag = table_flag.strip("-").replace("-", "_") + ("_nu" if env else "")
    on, out1, err1 = _run(job, "on_" + tag, [table_flag, "--coverage-spectrum"] + BG, env=env)
    off, out0, err0 = _run(job, "off_" + tag, [table_flag, "--coverage-spectrum"], env=env)
    here_on, here_off = str(job.d / ("on_" + tag)).encode(), str(job.d / ("off_" + tag)).encode()
    assert out1.replace(here_on, b"") == out0.replace(here_off, b"") and err1.replace(here_on, b"") == err0.replace(here_off, b"")
    for s in (0, 1, 2):
        assert on[s]["coverage_depth"] == off[s]["coverage_depth"] and on[s]["kmer_hits.gz"] == off[s]["kmer_hits.gz"]
        assert off[s]["coverage_background"] is None and off[s]["coverage_background_spectrum"] is None
        b = str(job.d / ("%s_" + tag) / (NAME % s))[: -len(".kmer_hits.gz")] + ".coverage_spectrum"
        assert open(b % "on", "rb").read() == open(b % "off", "rb").read()


def test_refusals(job):
    """each gives its message and a non-zero exit and writes nothing"""
    d = job.d
    (d / "x").mkdir()
    (d / "y").mkdir()
    for sub in ("x", "y"):
        (d / sub / "same.fa").write_bytes(_fa(job.files["clean.fa"][:20]))
    (d / "dup.txt").write_text(f"SE\t{d}/x/same.fa\nSE\t{d}/y/same.fa\n")
    cases = [
        ("r_dup", ["--coverage-only", "--coverage-background"], "dup.txt", b"share a file name"),
        ("r_max", ["--coverage-only", "--coverage-background", "--background-max", "256"], "T.txt", b"--background-max 256: a depth from 1 to 255"),
        ("r_alone", ["--coverage-only", "--background-spectrum"], "T.txt", b"--background-spectrum goes with --coverage-background"),
    ]
    for tag, flags, targets, words in cases:
        files, out, err = _run(job, tag, flags, targets=targets, ok=False)
        assert words in err and err.count(b"\n") == 1 and out == b"", err
        assert sorted(os.listdir(d / tag)) == ["S.txt", "run.err", "run.out"]
    # behind kmer_scrub_count --detect: refused before anything is read
    t = d / "r_detect"
    t.mkdir()
    rc, out, err = _env_run(native.run_cli_inprocess, ["-r", str(d / "s1.fa"), "-A", str(d / "A.txt"), "-B", str(d / "A.txt"), "--scrub", "0.5", "--detect",
                                                       "-o", str(t / (NAME % 1)), "-B", str(d / "T.txt"), "--coverage-depth", "--coverage-background"],
                            {}, t / "o", t / "e")
    assert rc != 0 and out == b"" and b"--coverage-background does not go behind --detect" in err and err.count(b"\n") == 1
    assert sorted(os.listdir(t)) == ["e", "o"]
