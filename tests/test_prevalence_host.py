"""kmer_scrub_count --prevalence on the CPU: the host layer (sk_host.c: the uncut plan, a slot per decode thread named before every
submit, the fold where an item ends, the records' merge, the two files) over tests/native/prevalence_double.c -- the device double
plus plain-C stand-ins for sk_item_slots / sk_item_slot / sk_item_fold -- as a stand-alone program under AddressSanitizer + UBSan
and again under ThreadSanitizer.  Ground truth is the oracle item by item (tests/_prevalence_model.py).

What only this build can show: every submit is preceded by its item's slot and every item ends in one fold (the double logs each
call); without the flag no slot call is ever made; two processes issue the same collectives and print what one prints; a rank with
another --prevalence-min-count makes every rank leave with the plan error.

The double has no byte-string keys and no U in reads (tests/native/device_double.c): the iupac_strain case is left to the GPU tests,
and where the double's own table without the flag is not the oracle's (mixed and drug: m1.fasta holds a read with U) the files are held to the identities
and to the flag-off run alone."""
import gzip
import json
import os
import random
import subprocess

import pytest

import _prevalence_model as model
import _synth

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(REPO, "tests", "native")
CSRC = os.path.join(REPO, "strainer2_amd", "csrc")
HOST = [os.path.join(CSRC, f) for f in ("sk_host.c", "sk_host_sd.c", "sk_host_cov.c")]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1", TSAN_OPTIONS="halt_on_error=1")
CASES_DIR = os.path.join(REPO, "tests", "golden", "cases")
CASES = [c for c in sorted(os.listdir(CASES_DIR)) if c != "iupac_strain"]


def _build(tmp_path_factory, sanitizer):
    out = str(tmp_path_factory.mktemp("pvdouble") / ("prevalence_" + sanitizer.split(",")[0]))
    subprocess.run(["gcc", "-O1", "-g", "-fsanitize=" + sanitizer, "-fno-omit-frame-pointer", "-DDOUBLE_MAIN=skh_kmer_scrub_count_main",
                    os.path.join(NATIVE, "prevalence_double.c")] + HOST + ["-lz", "-lpthread", "-o", out], check=True)
    return out


@pytest.fixture(scope="module", params=["address,undefined", "thread"])
def exe(request, tmp_path_factory):
    return _build(tmp_path_factory, request.param)


@pytest.fixture(scope="module")
def asan_exe(tmp_path_factory):
    return _build(tmp_path_factory, "address,undefined")


class Run:
    pass


def _run(exe, d, argv, tmp, extra=(), env=None):
    argv = list(argv)
    os.makedirs(tmp, exist_ok=True)
    prog = None
    if "-p" in argv:
        prog = os.path.join(tmp, "progress")
        argv[argv.index("-p") + 1] = prog
    log = os.path.join(tmp, "item_log")
    e = dict(ENV, SK_CHUNK_BYTES="4096", SK_THREADS="3", DOUBLE_ITEM_LOG=log)
    e.update(env or {})
    p = subprocess.run([exe] + argv + list(extra), cwd=d, env=e, capture_output=True, timeout=300)
    for bad in (b"runtime error", b"AddressSanitizer", b"ThreadSanitizer"):
        assert bad not in p.stderr, p.stderr.decode()[-3000:]
    r = Run()
    r.rc, r.out, r.err = p.returncode, p.stdout, p.stderr
    r.progress = [ln.split(b"\t")[0] for ln in open(prog, "rb").read().split(b"\n")] if prog and os.path.exists(prog) else None
    r.log = open(log).read().split("\n")[:-1] if os.path.exists(log) else []
    return r


def _check_log(log, n_lists_with_items, n_items):
    """slots once per list and freed again; a slot named before anything is folded; one fold per item"""
    assert [ln for ln in log if ln.startswith("slots ")].count("slots 0") == n_lists_with_items
    assert len([ln for ln in log if ln.startswith("slots ") and ln != "slots 0"]) == n_lists_with_items
    assert len([ln for ln in log if ln.startswith("fold ")]) == n_items
    nslots = 0
    for ln in log:
        what, v = ln.split()
        if what == "slots":
            nslots = int(v)
        else:
            assert -1 <= int(v) < nslots, ln


def _case(name):
    d = os.path.join(CASES_DIR, name)
    with open(os.path.join(d, "case.json")) as f:
        return d, json.load(f)


_models = {}


def _model_of(name, m):
    if (name, m) not in _models:
        d, meta = _case(name)
        a = meta["argv"]
        opt = {a[i]: a[i + 1] for i in range(len(a) - 1) if a[i] in ("-r", "-A", "-B", "-C")}
        _models[(name, m)] = model.Model(opt["-r"], [opt.get("-A"), opt.get("-B"), opt.get("-C")], m, d)
    return _models[(name, m)]


def _check_case(exe, name, tmp_path, env, m=1, pre=()):
    d, meta = _case(name)
    off = _run(exe, d, meta["argv"], str(tmp_path / "off"), pre, env)
    assert off.log == [], "without the flag no slot call is ever made"
    pf, itf = str(tmp_path / "prev.tsv"), str(tmp_path / "items.tsv")
    extra = list(pre) + ["--prevalence=" + pf, "--prevalence-items=" + itf, "--prevalence-min-count", str(m)]
    on = _run(exe, d, meta["argv"], str(tmp_path / "on"), extra, env)
    assert (on.rc, on.out, on.err, on.progress) == (off.rc, off.out, off.err, off.progress), on.err.decode()[-2000:]
    if off.rc != 0 or "-B" not in meta["argv"]:
        assert not os.path.exists(pf) and not os.path.exists(itf), "a run that fails reports nothing"
        return
    want = _model_of(name, m)
    got_p, got_i = open(pf, "rb").read(), open(itf, "rb").read()
    model.check_identities(got_p, got_i, on.out)
    assert got_p.split(b"\n")[:3] == want.prevalence_file().split(b"\n")[:3]
    assert [ln.split(b"\t")[:4] for ln in got_i.split(b"\n")] == [ln.split(b"\t")[:4] for ln in want.items_file().split(b"\n")]
    _check_log(on.log, sum(1 for n in want.n_items if n), sum(want.n_items))
    if on.out == want.count_table():                       # (the double counts what the oracle counts: then to the byte)
        assert got_i == want.items_file() and got_p == want.prevalence_file()
    else:
        assert name in ("mixed", "drug")                   # (m1.fasta holds a read with U)


@pytest.mark.parametrize("threads", ["1", "3", "16"])
@pytest.mark.parametrize("name", CASES)
def test_golden_cases_over_the_double(exe, name, threads, tmp_path):
    _check_case(exe, name, tmp_path, {"SK_THREADS": threads}, m=1 if threads != "16" else 2)


@pytest.mark.parametrize("pack", ["0", "2"])
@pytest.mark.parametrize("name", ["mixed", "drug", "truncated_fastq", "skip_after_missing"])
def test_golden_cases_packed_and_not(exe, name, pack, tmp_path):
    _check_case(exe, name, tmp_path, {"SK_LIST_PACK": pack})


@pytest.mark.parametrize("name", ["mixed", "drug"])
def test_golden_cases_pack_cache_filled_then_served(exe, name, tmp_path):
    cache = str(tmp_path / "cache")
    os.makedirs(cache)
    _check_case(exe, name, tmp_path / "fill", {}, pre=["--pack-cache", cache])
    assert os.listdir(cache)
    _check_case(exe, name, tmp_path / "serve", {}, pre=["--pack-cache", cache])


def _reads(rng, strain, n, max_len=120):
    out = []
    for i in range(n):
        x = rng.random()
        if x < 0.7:
            ln = rng.randint(31, max_len)
            a = rng.randrange(0, len(strain) - ln + 1)
            r = strain[a:a + ln]
            out.append(_synth.revcomp(r) if i % 2 else r)
        else:
            out.append(_synth.rand_dna(rng, rng.randint(1, max_len)))
    return out


def _forty(d):
    """40 tiny items in -A and -B: a duplicated line, an empty file; a -C list with the line equal to -r"""
    rng = random.Random(40)
    strain = _synth.rand_dna(rng, 3000)
    (d / "s.fa").write_bytes(b">s\n" + strain + b"\n")
    names = []
    for i in range(38):
        (d / f"i{i}.fa").write_bytes(b"".join(b">x\n%s\n" % x for x in _reads(random.Random(i), strain, 1 + i % 5, 90)))
        names.append(f"i{i}.fa")
    (d / "empty.fa").write_bytes(b"")
    names[7:7] = ["empty.fa"]
    names[20:20] = ["i3.fa"]
    (d / "A.txt").write_text("\n".join(names[:25]) + "\n")
    (d / "B.txt").write_text("\n".join(names[25:]) + "\n")
    (d / "C.txt").write_text("i1.fa\ns.fa\ni2.fa\n")
    return strain, ["-r", "s.fa", "-A", "A.txt", "-B", "B.txt", "-C", "C.txt"]


def test_more_items_than_slots(exe, tmp_path):
    _strain, argv = _forty(tmp_path)
    d = str(tmp_path)
    off = _run(exe, d, argv, str(tmp_path / "off"))
    on = _run(exe, d, argv, str(tmp_path / "on"), ["--prevalence=p.tsv", "--prevalence-items=i.tsv"])
    assert (on.rc, on.out, on.err) == (0, off.out, off.err) and off.log == []
    want = model.Model("s.fa", ["A.txt", "B.txt", "C.txt"], 1, d)
    assert want.n_items == [25, 15, 2] and on.out == want.count_table()
    assert (tmp_path / "i.tsv").read_bytes() == want.items_file()
    assert (tmp_path / "p.tsv").read_bytes() == want.prevalence_file()
    assert [ln for ln in on.log if ln.startswith("slots")] == ["slots 3", "slots 0", "slots 3", "slots 0", "slots 2", "slots 0"]
    _check_log(on.log, 3, 42)
    # a file that cannot be opened: reported as ever, nothing written, and what was scanned did not stay in a slot (the folds were made)
    with open(tmp_path / "B.txt", "a") as f:
        f.write("nope.fa\ni5.fa\n")
    off = _run(exe, d, argv, str(tmp_path / "off2"))
    on = _run(exe, d, argv, str(tmp_path / "on2"), ["--prevalence=p2.tsv", "--prevalence-items=i2.tsv"])
    assert (on.rc, on.out, on.err) == (off.rc, off.out, off.err) and off.rc == 1 and b"nope.fa" in off.err
    assert not (tmp_path / "p2.tsv").exists() and not (tmp_path / "i2.tsv").exists()
    assert on.log[-1] == "slots 0"


def test_slots_that_do_not_fit_fail_the_run_cleanly(asan_exe, tmp_path):
    _strain, argv = _forty(tmp_path)
    on = _run(asan_exe, str(tmp_path), argv, str(tmp_path / "on"), ["--prevalence=p.tsv"], {"DOUBLE_ITEM_NOMEM": "1"})
    assert on.rc == 1 and on.out == b"" and b"no room for 3 item slots" in on.err and not (tmp_path / "p.tsv").exists()


def test_gz_item_parsed_by_helper_threads(exe, tmp_path):
    rng = random.Random(77)
    strain = _synth.rand_dna(rng, 3000)
    (tmp_path / "s.fa").write_bytes(b">s\n" + strain + b"\n")
    reads = _reads(rng, strain, 900)
    with gzip.open(tmp_path / "big.fq.gz", "wb") as f:
        f.write(b"".join(b"@r%d\n%s\n+\n%s\n" % (i, r, b"I" * len(r)) for i, r in enumerate(reads)))
    (tmp_path / "m.fa").write_bytes(b"".join(b">m%d\n%s\n" % (i, r) for i, r in enumerate(reads[:200])))
    (tmp_path / "A.txt").write_text("m.fa\n")
    (tmp_path / "B.txt").write_text("m.fa\nbig.fq.gz\nm.fa\n")
    argv = ["-r", "s.fa", "-A", "A.txt", "-B", "B.txt"]
    env = {"SK_THREADS": "4", "SK_GZ_THREADS": "3", "SK_GZ_SEG": "3000", "SK_PARSE_THREADS": "3"}
    on = _run(exe, str(tmp_path), argv, str(tmp_path / "on"), ["--prevalence=p.tsv", "--prevalence-items=i.tsv", "--prevalence-min-count=2"], env)
    want = model.Model("s.fa", ["A.txt", "B.txt", None], 2, str(tmp_path))
    assert on.rc == 0 and on.out == want.count_table()
    assert (tmp_path / "i.tsv").read_bytes() == want.items_file() and (tmp_path / "p.tsv").read_bytes() == want.prevalence_file()
    _check_log(on.log, 2, 4)


# ---------------------------------------------------------------------------------------------------------- several processes
def _ranks(exe, world, argv_of, tmp, env_of=lambda r: {}):
    comm = tmp / ("comm_%d" % len(list(tmp.iterdir())))
    comm.mkdir()
    ps = []
    for r in range(world):
        env = dict(ENV, SK_THREADS="3", SK_CHUNK_BYTES="4096", WORLD_SIZE=str(world), RANK=str(r), LOCAL_RANK=str(r),
                   DOUBLE_COMM_DIR=str(comm), DOUBLE_COMM_TIMEOUT="30")
        env.update(env_of(r))
        ps.append(subprocess.Popen([exe] + argv_of(r), cwd=tmp, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE))
    out = []
    for p in ps:
        try:
            o, e = p.communicate(timeout=120)
        except subprocess.TimeoutExpired:
            for q in ps:
                q.kill()
            raise AssertionError("a rank hung")
        out.append((p.returncode, o, e))
    logs = [(comm / f"log.r{r}").read_text().splitlines() if (comm / f"log.r{r}").exists() else [] for r in range(world)]
    for rc, _o, e in out:
        assert rc not in (97, 98), e.decode()[-1500:]
        assert b"AddressSanitizer" not in e and b"runtime error" not in e, e.decode()[-3000:]
    return out, logs


def test_two_processes_print_what_one_prints(asan_exe, tmp_path):
    _strain, argv = _forty(tmp_path)
    one = _run(asan_exe, str(tmp_path), argv, str(tmp_path / "one"), ["--prevalence=p1.tsv", "--prevalence-items=i1.tsv", "--prevalence-min-count=2"])
    assert one.rc == 0
    out, logs = _ranks(asan_exe, 2, lambda r: argv + [f"--prevalence=pw{r}.tsv", f"--prevalence-items=iw{r}.tsv", "--prevalence-min-count=2"], tmp_path)
    assert [rc for rc, _o, _e in out] == [0, 0], out[0][2][-1500:] + out[1][2][-1500:]
    assert out[0][1] == one.out and out[1][1] == b"" and out[0][2] == one.err
    assert (tmp_path / "pw0.tsv").read_bytes() == (tmp_path / "p1.tsv").read_bytes()
    assert (tmp_path / "iw0.tsv").read_bytes() == (tmp_path / "i1.tsv").read_bytes()
    assert not (tmp_path / "pw1.tsv").exists() and not (tmp_path / "iw1.tsv").exists()         # rank 0 alone writes
    want = model.Model("s.fa", ["A.txt", "B.txt", "C.txt"], 2, str(tmp_path))
    assert (tmp_path / "iw0.tsv").read_bytes() == want.items_file() and (tmp_path / "pw0.tsv").read_bytes() == want.prevalence_file()
    assert logs[0] == logs[1]
    # rendezvous, the table-load agreement, 3 lists x (before, after, the items' records: 3 u64 per list line), the failure sum, the all-reduce
    assert logs[0] == ["rendezvous 1", "sum_u32 1"] + [x for n in (25, 15, 3) for x in ("max_u64 3", "max_u64 3", "max_u64 %d" % (3 * n))] + \
        ["sum_u32 1", "allreduce_u32 %d" % (7 * len(want.keys))]


def test_a_missing_file_on_one_rank_keeps_the_collectives_the_same(asan_exe, tmp_path):
    _strain, argv = _forty(tmp_path)
    with open(tmp_path / "B.txt", "a") as f:
        f.write("nope.fa\ni5.fa\n")
    out, logs = _ranks(asan_exe, 2, lambda r: argv + ["--prevalence=pw.tsv"], tmp_path)
    assert [rc for rc, _o, _e in out] == [1, 1] and logs[0] == logs[1]
    assert "max_u64 51" in logs[0], "the records' collective is issued whatever failed"
    assert not (tmp_path / "pw.tsv").exists()


def test_ranks_that_disagree_about_min_count_get_the_plan_error(asan_exe, tmp_path):
    _strain, argv = _forty(tmp_path)
    out, logs = _ranks(asan_exe, 2, lambda r: argv + ["--prevalence=pw.tsv", "--prevalence-min-count", str(1 + r)], tmp_path)
    assert [rc for rc, _o, _e in out] == [1, 1] and logs[0] == logs[1]
    assert all(b"the ranks computed different work plans" in e for _rc, _o, e in out)
    assert not (tmp_path / "pw.tsv").exists()
    out, logs = _ranks(asan_exe, 2, lambda r: argv + (["--prevalence=pw.tsv"] if r else []), tmp_path)      # ... and about the flag itself
    assert [rc for rc, _o, _e in out] == [1, 1] and logs[0] == logs[1]
    assert all(b"the ranks computed different work plans" in e for _rc, _o, e in out)
