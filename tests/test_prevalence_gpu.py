"""kmer_scrub_count --prevalence on the device: the item slots and the item fold (sk_item_slots / sk_item_slot / sk_item_fold) against
the CPU oracle run item by item (tests/_prevalence_model.py restates the rule), and the program -- every golden case, the list-walk's
submit paths, more items than slots, scrub by prevalence, the refusals.  The ground truth is never the code under test.

The progress file holds a time stamp per line: it is compared with the time column taken out, everything else byte for byte."""
import gzip
import json
import os
import random
import shutil
import subprocess

import numpy as np
import pytest

import _oracle
import _prevalence_model as model
import _synth
import strainer2_amd as sk

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(REPO, "strainer2_amd", "bin")
EXE = sk.cli_path()
CASES_DIR = os.path.join(REPO, "tests", "golden", "cases")
CASES = sorted(os.listdir(CASES_DIR))
BIG = 10 ** 6                                               # a min_count above every count of these worlds


# ---------------------------------------------------------------------------------------------------------- the device API
def _reads(rng, strain, n, max_len=120):
    """records of the strain (either strand, whole now and then), of noise, and shorter than k"""
    out = []
    for i in range(n):
        x = rng.random()
        if len(strain) <= 40:
            r = strain if x < 0.5 else _synth.revcomp(strain) if x < 0.8 else _synth.rand_dna(rng, 31)
        elif x < 0.75:
            ln = rng.randint(31, min(max_len, len(strain)))
            a = rng.randrange(0, len(strain) - ln + 1)
            r = strain[a:a + ln]
            if i % 2:
                r = _synth.revcomp(r)
        elif x < 0.9:
            r = _synth.rand_dna(rng, rng.randint(1, max_len))
        else:
            r = strain[:20]
        out.append(r)
    return b"\n".join(out) + b"\n"


def _world(strain_stream, chunks_a, chunks_b, build=None):
    """oracle columns of two items (A: chunks_a, B: chunks_b) over the strain, and of A's first chunk alone: (keys, vA, vB, vA1)"""
    t = _oracle.OracleTable(ncols=4)
    assert (build(t) if build else t.build_stream(strain_stream)) == 0
    for col, chunks in ((1, chunks_a), (2, chunks_b), (3, chunks_a[:1])):
        for ch in chunks:
            t.scan_stream(ch, col)
    keys, c = t.rows()
    t.close()
    return keys, c[:, 1].astype(np.uint32), c[:, 2].astype(np.uint32), c[:, 3].astype(np.uint32)


def _record(ctx, ptr):
    return [int(x) for x in ctx.dev_download(ptr, 16).view(np.uint64)]


def _scan(ctx, data, col, via):
    if via == "stream":
        ctx.scan_stream(data, col)
        return None
    buf = np.frombuffer(data + b"\n" * ((-len(data)) % 16 + 16), dtype=np.uint8)       # (a resident batch: the two scan lanes take turns)
    p = ctx.dev_alloc(buf.size)
    ctx.dev_upload(p, buf)
    ctx.scan_device(p, len(data), col)
    return p


def _two_slots(ks, want, chunks_a, chunks_b, min_count, text_stage=1, via="stream"):
    """A1, B1, A2, B2 ... into slots 0 and 1 in turn; fold A, then B; fold the empty slots again: columns and both records"""
    keys, va, vb, va1 = want
    rng = np.random.default_rng(len(keys) + min_count)
    with sk.KmerContext(0) as ctx:
        ctx.set_option("text_stage", text_stage)
        ctx.load_keyset(ks, 4)
        assert ctx.nrows == len(keys) and ks.keys() == keys
        base_c = rng.integers(0, 2 ** 32, len(keys), dtype=np.uint64).astype(np.uint32)    # the columns hold something already: the fold ADDS, mod 2^32
        base_p = rng.integers(0, 1000, len(keys), dtype=np.uint64).astype(np.uint32)
        ctx.set_counts(1, base_c)
        ctx.set_counts(2, base_p)
        other = ctx.counts(3).copy()
        rec = ctx.dev_alloc(64)
        ctx.dev_upload(rec, np.zeros(8, dtype=np.uint64))
        ctx.item_slots(2)
        held = []
        for i in range(max(len(chunks_a), len(chunks_b))):
            for slot, chunks in ((0, chunks_a), (1, chunks_b)):
                if i < len(chunks):
                    ctx.item_slot(slot)
                    held.append(_scan(ctx, chunks[i], 1, via))
        ctx.item_slot(-1)
        assert np.array_equal(ctx.counts(1), base_c), "a slot scan leaves the column alone until the fold"
        ctx.item_fold(0, 1, 2, min_count, rec)
        assert np.array_equal(ctx.counts(1), base_c + va)
        assert np.array_equal(ctx.counts(2), base_p + (va >= min_count))
        ctx.item_fold(1, 1, 2, min_count, rec + 16)
        ctx.sync()
        want_c, want_p = base_c + va + vb, base_p + (va >= min_count) + (vb >= min_count)
        assert np.array_equal(ctx.counts(1), want_c)
        assert np.array_equal(ctx.counts(2), want_p)
        assert _record(ctx, rec) == [int((va >= min_count).sum()), int(va.astype(np.uint64).sum())]
        assert _record(ctx, rec + 16) == [int((vb >= min_count).sum()), int(vb.astype(np.uint64).sum())]
        # the apply kernel left the slots zero: folding them again changes nothing
        ctx.item_fold(0, 1, 2, 1, rec + 32)
        ctx.item_fold(1, 1, 2, 1, rec + 32)
        assert np.array_equal(ctx.counts(1), want_c) and np.array_equal(ctx.counts(2), want_p)
        assert _record(ctx, rec + 32) == [0, 0]
        # no slot: a scan goes into the column it names, as ever
        ctx.scan_stream(chunks_a[0], 3)
        assert np.array_equal(ctx.counts(3), other + va1)
        assert np.array_equal(ctx.counts(1), want_c) and np.array_equal(ctx.counts(2), want_p)
        assert np.array_equal(ctx.counts(0), ks.first_count())
        for p in held:
            if p:
                ctx.dev_free(p)
        ctx.item_slots(0)


@pytest.fixture(scope="module")
def sized():
    """strains of exactly n distinct k-mers around SK_DIFF_PER_BLOCK = 4096 (the arrays hold nrows + 1 live entries), their items and
    the oracle's columns, made once"""
    out = {}
    for n in (1, 2, 4095, 4096, 4097, 8193):
        rng = random.Random(9000 + n)
        strain = _synth.rand_dna(rng, n + 30)
        nreads = 6 if n < 3 else 60
        ca = [_reads(rng, strain, nreads) for _ in range(2)]
        cb = [_reads(rng, strain, nreads) for _ in range(2)]
        ks = sk.Keyset.from_stream(strain + b"\n")
        assert ks.nrows == n
        out[n] = (ks, _world(strain + b"\n", ca, cb), ca, cb)
    return out


@pytest.mark.parametrize("n", [1, 2, 4095, 4096, 4097, 8193])
@pytest.mark.parametrize("min_count", [1, 2, BIG])
def test_two_slots_take_chunks_in_turn(sized, n, min_count):
    ks, want, ca, cb = sized[n]
    assert int(want[1].sum()) > 0 and int(want[2].sum()) > 0
    if n > 2:
        assert (want[1] >= 2).any() and (want[1] == 1).any() and (want[1] == 0).any()       # (min_count 2 splits the rows)
    _two_slots(ks, want, ca, cb, min_count)


@pytest.mark.parametrize("n", [4096, 8193])
def test_resident_batches_on_both_scan_lanes_into_slots(sized, n):
    ks, want, ca, cb = sized[n]
    _two_slots(ks, want, ca, cb, 1, via="device")


@pytest.mark.parametrize("n", [2, 4097])
def test_table_without_a_text_stage(sized, n):
    """every hit is an atomic add to sink.counts: the slot's scratch column, not its difference array"""
    ks, want, ca, cb = sized[n]
    _two_slots(ks, want, ca, cb, 2, text_stage=0)


def test_repeated_kmer_and_reverse_complement_item():
    """a strain that holds a stretch twice: one row, hit through either place; item B is the strain's reverse complement"""
    rng = random.Random(31)
    x, y = _synth.rand_dna(rng, 70), _synth.rand_dna(rng, 500)
    strain = x + y + x
    ks = sk.Keyset.from_stream(strain + b"\n")
    assert ks.nrows == len(strain) - 30 - 40                                           # (the second x's 40 windows are repeats)
    ca = [strain[:70] + b"\n" + strain[-70:] + b"\n" + strain[-100:] + b"\n", strain[540:] + b"\n"]
    cb = [_synth.revcomp(strain) + b"\n"]
    want = _world(strain + b"\n", ca, cb)
    assert want[1].max() >= 3 and (want[2][want[2] > 0] >= 1).all() and (want[2] == 2).sum() == 40
    for m in (1, 2, 3):
        _two_slots(ks, want, ca, cb, m)


def test_byte_string_kernel_writes_into_the_slot(golden):
    """the iupac_strain golden's strain: keys with IUPAC letters are counted by the byte-string kernel, which adds to sink.counts"""
    d = os.path.join(golden, "cases", "iupac_strain")
    ks = sk.Keyset.from_file(os.path.join(d, "strain.fa"))
    assert ks.nwide > 0
    data, _, _ = _oracle.decode_file(os.path.join(d, "m.fa"))
    strain, _, _ = _oracle.decode_file(os.path.join(d, "strain.fa"))
    ca, cb = [data, strain], [_synth.revcomp(strain.replace(b"\n", b"N")) + b"\n", data]
    want = _world(None, ca, cb, build=lambda t: t.build_file(os.path.join(d, "strain.fa")))
    wide = np.array([len(k) != 31 or any(c not in b"ACGT" for c in k) for k in want[0]])
    assert wide.any() and int(want[1][wide].sum()) > 0, "the items hit byte-string keys"
    for m in (1, 2):
        _two_slots(ks, want, ca, cb, m)


def test_slot_calls_are_checked():
    rng = random.Random(5)
    ks = sk.Keyset.from_stream(_synth.rand_dna(rng, 100) + b"\n")
    with sk.KmerContext(0) as ctx:
        with pytest.raises(sk.SKError):
            ctx.item_slots(1)                               # no table
        ctx.load_keyset(ks, 4)
        with pytest.raises(sk.SKError):
            ctx.item_slot(0)                                # nothing allocated unless asked for
        with pytest.raises(sk.SKError):
            ctx.item_fold(0, 1, 2, 1, None)
        ctx.item_slots(3)
        for bad in (lambda: ctx.item_slot(3), lambda: ctx.item_slot(-2), lambda: ctx.item_fold(3, 1, 2, 1, None),
                    lambda: ctx.item_fold(0, 1, 1, 1, None), lambda: ctx.item_fold(0, 1, 4, 1, None), lambda: ctx.item_fold(0, 1, 2, 0, None)):
            with pytest.raises(sk.SKError):
                bad()
        with pytest.raises(sk.SKError):
            ctx.item_slots(257)                             # above SK_ITEM_SLOTS_MAX
        ctx.item_slots(2)                                   # the failure left nothing behind: the next call works
        ctx.item_slot(1)
        ctx.item_slots(0)
        with pytest.raises(sk.SKError):
            ctx.item_slot(0)


# ---------------------------------------------------------------------------------------------------------- the program
def _strip_times(progress):
    return None if progress is None else [ln.split(b"\t")[0] for ln in progress.split(b"\n")]


class Run:
    pass


def _run(d, argv, tmp, extra=(), env=None, exe=EXE):
    """the program in directory d with the case's argv; -p goes to tmp; returns what it said and wrote"""
    argv = list(argv)
    os.makedirs(tmp, exist_ok=True)
    prog = None
    if "-p" in argv:
        prog = os.path.join(tmp, "progress")
        argv[argv.index("-p") + 1] = prog
    e = dict(os.environ, SK_CHUNK_BYTES="4096", SK_THREADS="3")
    e.update(env or {})
    p = subprocess.run([exe] + argv + list(extra), cwd=d, env=e, capture_output=True, timeout=120)
    r = Run()
    r.rc, r.out, r.err = p.returncode, p.stdout, p.stderr
    r.progress = open(prog, "rb").read() if prog and os.path.exists(prog) else None
    return r


_off, _models = {}, {}


def _case(name):
    d = os.path.join(CASES_DIR, name)
    with open(os.path.join(d, "case.json")) as f:
        return d, json.load(f)


def _baseline(name, tmp_path_factory):
    if name not in _off:
        d, meta = _case(name)
        _off[name] = _run(d, meta["argv"], str(tmp_path_factory.mktemp("off_" + name)))
    return _off[name]


def _model_of(name, m=1):
    if (name, m) not in _models:
        d, meta = _case(name)
        a = meta["argv"]
        opt = {a[i]: a[i + 1] for i in range(len(a) - 1) if a[i] in ("-r", "-A", "-B", "-C")}
        _models[(name, m)] = model.Model(opt["-r"], [opt.get("-A"), opt.get("-B"), opt.get("-C")], m, d)
    return _models[(name, m)]


def _check_case(name, tmp_path, tmp_path_factory, env, m=1, pre=()):
    d, meta = _case(name)
    off = _baseline(name, tmp_path_factory)
    pf, itf = str(tmp_path / "prev.tsv"), str(tmp_path / "items.tsv")
    extra = list(pre) + ["--prevalence=" + pf, "--prevalence-items=" + itf] + (["--prevalence-min-count", str(m)] if m != 1 else [])
    on = _run(d, meta["argv"], str(tmp_path / "on"), extra, env)
    assert (on.rc, on.out, on.err) == (off.rc, off.out, off.err), on.err.decode()[-2000:]
    assert _strip_times(on.progress) == _strip_times(off.progress)
    if off.rc != 0 or "-B" not in meta["argv"]:
        assert not os.path.exists(pf) and not os.path.exists(itf), "a run that fails reports nothing"
        return
    want = _model_of(name, m)
    got_p, got_i = open(pf, "rb").read(), open(itf, "rb").read()
    assert on.out == want.count_table(), "the oracle item by item adds up to the count table"
    assert got_i == want.items_file()
    assert got_p == want.prevalence_file()
    model.check_identities(got_p, got_i, on.out)


@pytest.mark.parametrize("threads", ["1", "3", "16"])
@pytest.mark.parametrize("name", CASES)
def test_golden_cases(name, threads, tmp_path, tmp_path_factory):
    _check_case(name, tmp_path, tmp_path_factory, {"SK_THREADS": threads})


@pytest.mark.parametrize("env", [{"SK_LIST_PACK": "0"}, {"SK_LIST_PACK": "2"}, {"SK_DEVICE_PARSE": "1"}], ids=["pack0", "pack2", "device_parse"])
@pytest.mark.parametrize("name", CASES)
def test_golden_cases_on_the_other_submit_paths(name, env, tmp_path, tmp_path_factory):
    _check_case(name, tmp_path, tmp_path_factory, env, m=2 if env.get("SK_LIST_PACK") == "2" else 1)


@pytest.mark.parametrize("name", CASES)
def test_golden_cases_pack_cache_filled_then_served(name, tmp_path, tmp_path_factory):
    cache = str(tmp_path / "cache")
    os.makedirs(cache)
    _check_case(name, tmp_path / "fill", tmp_path_factory, {}, pre=["--pack-cache", cache])
    filled = os.listdir(cache)
    _check_case(name, tmp_path / "serve", tmp_path_factory, {}, pre=["--pack-cache", cache])
    if _baseline(name, tmp_path_factory).rc == 0 and "-B" in _case(name)[1]["argv"]:
        assert filled, "the first run wrote cache files, the second was served from them"


def _write_world(d, rng):
    strain = _synth.rand_dna(rng, 3000)
    (d / "s.fa").write_bytes(b">s\n" + strain + b"\n")
    return strain


def test_gz_item_parsed_by_helper_threads(tmp_path):
    """one .gz item of many chunks whose text is cut into segments for parse_gz_split's helpers: their submits are their parent's item's"""
    rng = random.Random(77)
    strain = _write_world(tmp_path, rng)
    reads = [_reads(rng, strain, 1).strip() for _ in range(1500)]
    with gzip.open(tmp_path / "big.fq.gz", "wb") as f:
        f.write(b"".join(b"@r%d\n%s\n+\n%s\n" % (i, r, b"I" * len(r)) for i, r in enumerate(reads)))
    (tmp_path / "g.fa").write_bytes(b">g\n" + _synth.mutate(rng, strain, 0.02) + b"\n")
    (tmp_path / "m.fa").write_bytes(b"".join(b">m%d\n%s\n" % (i, r) for i, r in enumerate(reads[:200])))
    (tmp_path / "A.txt").write_text("g.fa\n")
    (tmp_path / "B.txt").write_text("m.fa\nbig.fq.gz\nm.fa\n")
    argv = ["-r", "s.fa", "-A", "A.txt", "-B", "B.txt"]
    env = {"SK_THREADS": "4", "SK_GZ_THREADS": "3", "SK_GZ_SEG": "3000", "SK_PARSE_THREADS": "3"}
    off = _run(str(tmp_path), argv, str(tmp_path / "off"), env=env)
    on = _run(str(tmp_path), argv, str(tmp_path / "on"), ["--prevalence=p.tsv", "--prevalence-items=i.tsv", "--prevalence-min-count=2"], env)
    assert (on.rc, on.out, on.err) == (0, off.out, off.err), on.err.decode()[-2000:]
    want = model.Model("s.fa", ["A.txt", "B.txt", None], 2, str(tmp_path))
    assert on.out == want.count_table()
    assert (tmp_path / "i.tsv").read_bytes() == want.items_file()
    assert (tmp_path / "p.tsv").read_bytes() == want.prevalence_file()
    assert want.records[2][3] > 20 * 4096, "the .gz item spans many chunks"
    model.check_identities((tmp_path / "p.tsv").read_bytes(), (tmp_path / "i.tsv").read_bytes(), on.out)


def _forty(tmp_path):
    rng = random.Random(40)
    strain = _write_world(tmp_path, rng)
    names = []
    for i in range(38):
        r = _reads(random.Random(i), strain, 1 + i % 5, max_len=90)
        (tmp_path / f"i{i}.fa").write_bytes(b"".join(b">x\n%s\n" % x for x in r.split(b"\n") if x))
        names.append(f"i{i}.fa")
    (tmp_path / "empty.fa").write_bytes(b"")
    names[7:7] = ["empty.fa"]
    names[20:20] = ["i3.fa"]                                 # a duplicated line: two items
    assert len(names) == 40
    (tmp_path / "A.txt").write_text("\n".join(names[:25]) + "\n")
    (tmp_path / "B.txt").write_text("\n".join(names[25:]) + "\n")
    (tmp_path / "C.txt").write_text("i1.fa\ns.fa\ni2.fa\n")  # the -C line equal to -r is no item
    return ["-r", "s.fa", "-A", "A.txt", "-B", "B.txt", "-C", "C.txt", "-p", "x"]


def test_more_items_than_slots(tmp_path):
    argv = _forty(tmp_path)
    d = str(tmp_path)
    off = _run(d, argv, str(tmp_path / "off"))
    on = _run(d, argv, str(tmp_path / "on"), ["--prevalence", "--prevalence-items=i.tsv"])
    assert (on.rc, on.out, on.err) == (0, off.out, off.err), on.err.decode()[-2000:]
    assert off.err == b"skipping s.fa (identical match)\n"
    assert _strip_times(on.progress) == _strip_times(off.progress)
    pf = str(tmp_path / "on" / "progress") + ".prevalence.tsv"    # the default name: <progress file>.prevalence.tsv
    want = model.Model("s.fa", ["A.txt", "B.txt", "C.txt"], 1, d)
    got_p, got_i = open(pf, "rb").read(), (tmp_path / "i.tsv").read_bytes()
    assert got_p.split(b"\n")[1:3] == [b"#items\t25\t15\t2", b"#min_count\t1"]
    assert [r[2] for r in want.records].count("i3.fa") == 2 and ("A", 8, "empty.fa", 0, 0, 0) in want.records
    assert got_i == want.items_file() and len(got_i.split(b"\n")) == 1 + 42 + 1
    assert got_p == want.prevalence_file() and on.out == want.count_table()
    model.check_identities(got_p, got_i, on.out)
    # a file that cannot be opened is reported as ever, and nothing is written
    with open(tmp_path / "B.txt", "a") as f:
        f.write("nope.fa\ni5.fa\n")
    off = _run(d, argv, str(tmp_path / "off2"))
    on = _run(d, argv, str(tmp_path / "on2"), ["--prevalence=p2.tsv", "--prevalence-items=i2.tsv"])
    assert (on.rc, on.out, on.err) == (off.rc, off.out, off.err) and off.rc == 1 and b"nope.fa" in off.err
    assert not (tmp_path / "p2.tsv").exists() and not (tmp_path / "i2.tsv").exists()


def test_through_the_communicator_with_a_world_of_one(tmp_path):
    """SK_FORCE_COMM=1: the one-process-per-GPU path with a world of one -- the plan agreements, the items' records through
    sk_comm_max_u64 (75, 45 and 9 values: above the eight that fit the flag block's scratch words), the all-reduce of seven columns"""
    argv = _forty(tmp_path)[:-2]
    d = str(tmp_path)
    env = {"SK_FORCE_COMM": "1", "SK_RCCL_ID_FILE": str(tmp_path / "rccl_id")}
    on = _run(d, argv, str(tmp_path / "on"), ["--prevalence=p.tsv", "--prevalence-items=i.tsv", "--prevalence-min-count", "2"], env)
    assert on.rc == 0, on.err.decode()[-2000:]
    want = model.Model("s.fa", ["A.txt", "B.txt", "C.txt"], 2, d)
    assert on.out == want.count_table() and on.err.endswith(b"skipping s.fa (identical match)\n")
    assert (tmp_path / "i.tsv").read_bytes() == want.items_file()
    assert (tmp_path / "p.tsv").read_bytes() == want.prevalence_file()


def test_default_file_name_without_a_progress_file(tmp_path):
    argv = _forty(tmp_path)[:-2]
    on = _run(str(tmp_path), argv, str(tmp_path / "on"), ["--prevalence"])
    assert on.rc == 0 and (tmp_path / "kmer_scrub_count.prevalence.tsv").exists()


# ---------------------------------------------------------------------------------------------------------- scrub by prevalence
@pytest.fixture(scope="module")
def scrub_world(tmp_path_factory):
    """a strain, genomes that share parts of it, metagenomes of which one is deep: counts and prevalence rank differently"""
    d = tmp_path_factory.mktemp("scrubprev")
    rng = random.Random(2025)
    strain = _synth.rand_dna(rng, 4000)
    (d / "s.fa").write_bytes(b">s\n" + strain + b"\n")
    a, b = [], []
    for i in range(6):
        lo = 400 * i
        (d / f"g{i}.fa").write_bytes(b">g\n" + _synth.rand_dna(rng, 300) + strain[lo:lo + 900 + 150 * i] + b"\n")
        a.append(f"g{i}.fa")
    for i in range(5):
        n = 400 if i == 0 else 30                           # m0 is deep and holds one stretch over and over
        reads = [strain[1000:1100] if i == 0 and k % 2 else _reads(rng, strain, 1, 100).strip() for k in range(n)]
        (d / f"m{i}.fa").write_bytes(b"".join(b">r\n%s\n" % r for r in reads))
        b.append(f"m{i}.fa")
    (d / "d0.fa").write_bytes(b">d\n" + strain[3000:3400] + b"\n")
    (d / "A.txt").write_text("\n".join(a) + "\n")
    (d / "B.txt").write_text("\n".join(b) + "\n")
    (d / "C.txt").write_text("d0.fa\n")
    targets = d / "T.txt"
    (d / "t.fa").write_bytes(b"".join(b">t%d\n%s\n" % (k, _reads(rng, strain, 1, 100).strip()) for k in range(200)))
    targets.write_text(f"SE\t{d}/t.fa\n")
    return d


@pytest.mark.parametrize("lists", [("A", "B"), ("A", "B", "C")], ids=["no_drug", "drug"])
@pytest.mark.parametrize("independent", [False, True], ids=["joint", "independent"])
def test_scrub_by_prevalence_equals_step_2_on_the_prevalence_file(scrub_world, lists, independent, tmp_path):
    d = str(scrub_world)
    argv = ["-r", "s.fa"] + [x for l in lists for x in ("-" + l, l + ".txt")]
    pf = str(tmp_path / "prev.tsv")
    ind = ["--independent"] if independent else []
    on = _run(d, argv, str(tmp_path / "on"), ["--prevalence=" + pf, "--scrub", "0.25", "--scrub-by", "prevalence"] + ind)
    assert on.rc == 0, on.err.decode()[-2000:]
    step2 = subprocess.run([os.path.join(BIN, "kmer_scrub_filter"), "-s", pf, "-m", "0.25"] + (["-i"] if independent else []), capture_output=True, timeout=120)
    assert step2.returncode == 0 and (on.out, on.err) == (step2.stdout, step2.stderr)
    assert open(pf, "rb").read() == model.Model("s.fa", [l + ".txt" for l in lists] + [None] * (3 - len(lists)), 1, d).prevalence_file()
    by_count = _run(d, argv, str(tmp_path / "cnt"), ["--scrub", "0.25"] + ind)
    assert by_count.rc == 0 and by_count.out != on.out and len(on.out) > 0, "prevalence ranks the k-mers differently from the counts"
    same = _run(d, argv, str(tmp_path / "cnt2"), ["--prevalence=" + str(tmp_path / "p2.tsv"), "--scrub", "0.25", "--scrub-by", "count"] + ind)
    assert (same.rc, same.out, same.err) == (0, by_count.out, by_count.err)


def test_scrub_by_prevalence_with_detect(scrub_world, tmp_path):
    """the hit list equals strain_detect -a on the list step 2 made: the adopted table tolerates the three columns behind its six"""
    d = str(scrub_world)
    pf, so = str(tmp_path / "prev.tsv"), str(tmp_path / "inf.txt")
    on = _run(d, ["-r", "s.fa", "-A", "A.txt", "-B", "B.txt"], str(tmp_path / "on"),
              ["--prevalence=" + pf, "--scrub", "0.25", "--scrub-by", "prevalence", "--scrub-out", so, "--detect", "-B", "T.txt", "-o", str(tmp_path / "fused.kmer_hits.gz")])
    assert on.rc == 0, on.err.decode()[-2000:]
    step2 = subprocess.run([os.path.join(BIN, "kmer_scrub_filter"), "-s", pf, "-m", "0.25"], capture_output=True, timeout=120)
    assert step2.returncode == 0 and open(so, "rb").read() == step2.stdout and len(step2.stdout) > 0
    sd = subprocess.run([os.path.join(BIN, "strain_detect"), "-r", "s.fa", "-a", so, "-B", "T.txt", "-o", str(tmp_path / "plain.kmer_hits.gz")],
                        cwd=d, capture_output=True, timeout=120)
    assert sd.returncode == 0, sd.stderr.decode()[-2000:]
    fused, plain = gzip.open(tmp_path / "fused.kmer_hits.gz").read(), gzip.open(tmp_path / "plain.kmer_hits.gz").read()
    assert fused == plain and len(plain) > 0


# ---------------------------------------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("extra,say", [
    (["--scrub", "0.25", "--scrub-by", "prevalence"], b"--scrub-by prevalence needs --prevalence"),
    (["--prevalence", "--scrub", "0.25,0.1", "--scrub-by", "prevalence", "--detect", "-B", "T.txt", "-o", "x.gz", "--coverage-scrub-sweep"], b"does not go with a list of fractions"),
    (["--prevalence", "--prevalence-min-count", "0"], b"--prevalence-min-count needs an integer of at least 1"),
    (["--prevalence", "--prevalence-min-count=two"], b"--prevalence-min-count needs an integer of at least 1"),
    (["--prevalence-items=i.tsv"], b"need --prevalence"),
    (["--prevalence", "--scrub-by", "prevalence"], b"--scrub-by needs --scrub"),
])
def test_refused_before_anything_is_read(scrub_world, extra, say, tmp_path):
    d = tmp_path / "w"
    shutil.copytree(scrub_world, d)
    before = sorted(os.listdir(d))
    p = subprocess.run([EXE, "-r", "nonexistent.fa", "-A", "A.txt", "-B", "B.txt", "-p", "prog"] + extra, cwd=d, capture_output=True, timeout=60)
    assert p.returncode == 1 and say in p.stderr and p.stdout == b"" and p.stderr.count(b"\n") == 1
    assert b"nonexistent" not in p.stderr, "refused before the strain is opened"
    assert sorted(os.listdir(d)) == before, "nothing was created"


def test_strains_file_with_prevalence_is_refused(scrub_world, tmp_path):
    d = tmp_path / "w"
    shutil.copytree(scrub_world, d)
    (d / "S.txt").write_text("s.fa\tout0.tsv\n")
    before = sorted(os.listdir(d))
    p = subprocess.run([EXE, "-S", "S.txt", "-A", "A.txt", "-B", "B.txt", "--prevalence"], cwd=d, capture_output=True, timeout=60)
    assert p.returncode == 1 and b"--prevalence does not go with -S" in p.stderr and p.stderr.count(b"\n") == 1 and p.stdout == b""
    assert sorted(os.listdir(d)) == before
