"""Thresholds on the device (include/strainer_kmer.h has the rule): the classifying folds and the finishing pass
(sk_covacc_set_thresholds / sk_covacc_add_rows_hits / sk_covacc_add / sk_covacc_finish_target_thresholds), sk_distinct_thresholds,
and the programs in every form they run in, all against tests/_thresholds_model.py.

Library level: accumulators are built from row counts alone and fed through add_rows_hits; members of 0, 1, 255, 257 and 70 001 rows
sit in one accumulator (70 001 rows are more than 256 workgroups x 256 threads, so the finishing pass's grid-stride loop turns more
than once).  Real launches run in the world of test_coverage_regions_gpu.py; for every threshold t the expected numbers come from
test_coverage_only_gpu.py's model(min_hits=t)."""
import gzip
import hashlib
import json
import os
import random
import shutil
import subprocess

import numpy as np
import pytest

import _skt
import _synth
import strainer2_amd as sk
from _thresholds_model import DEFAULT, check_invariants, main_table, parse_table, table_from_hits
from strainer2_amd import native
from test_coverage_only_gpu import NAME, WENT, _fa, _union_collect, model
from test_coverage_regions_gpu import STRAIN_ORDER, _base, _run_sd, _stream, world  # noqa: F401  (world: the fixture)
from test_coverage_spectrum_gpu import SMALL_CHUNKS, job  # noqa: F401  (job: the fixture)
from test_sanitizers import COV_CASES, prepare_cov_case

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 255, 257, 70001]
SK_E_ARG, SK_E_STATE = -3, -7
TOP = 2 ** 31 - 2
LISTS = [[0], [0, 4], list(range(16)), [1, 6, TOP]]


@pytest.fixture(scope="module")
def ctx():
    with sk.KmerContext(0) as c:
        yield c


def _numbers(rows, totals, lst):
    rows, totals = np.asarray(rows, dtype=np.int64), np.asarray(totals, dtype=np.int64)
    return ([len(np.unique(rows[totals > t])) for t in lst], [int((totals > t).sum()) for t in lst])


def _depth(n, rows, totals, min_hits):
    rows, totals = np.asarray(rows, dtype=np.int64), np.asarray(totals, dtype=np.int64)
    return np.bincount(rows[totals > min_hits], minlength=n).astype(np.uint32)[:n] if n else np.zeros(0, dtype=np.uint32)


def _feed(acc, entries):
    for m, (rows, totals) in enumerate(entries):
        if len(rows):
            acc.add_rows_hits(m, rows, totals)


def _finish_and_check(acc, entries, lst):
    uq, tot = acc.finish_target_thresholds()
    assert uq.shape == tot.shape == (len(entries), len(lst))
    for m, (rows, totals) in enumerate(entries):
        wu, wt = _numbers(rows, totals, lst)
        assert uq[m].tolist() == wu and tot[m].tolist() == wt, ("member", m)
    uq2, tot2 = acc.finish_target_thresholds()                 # the threshold state is zero afterwards
    assert not uq2.any() and not tot2.any()
    return uq, tot


def _entries(lst, rng, primary=0):
    """per member of SIZES: every row at least once where there is room, extras on random rows; totals drawn from 0, every t and
    t + 1 of the list, the primary threshold and its neighbour"""
    pool = sorted({0, primary, primary + 1} | {t for t in lst} | {t + 1 for t in lst if t != TOP})
    out = []
    for n in SIZES:
        if not n:
            out.append((np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.uint32)))
            continue
        rows = np.concatenate([np.arange(n), rng.integers(0, n, min(3 * n, 5000) + 7)]).astype(np.uint32)
        out.append((rows, rng.choice(pool, len(rows)).astype(np.uint32)))
    return out


@pytest.mark.parametrize("lst", LISTS, ids=lambda l: "list%d" % len(l))
def test_members_of_every_size_totals_at_and_above_every_threshold(ctx, lst):
    rng = np.random.default_rng(len(lst))
    entries = _entries(lst, rng)
    with sk.CoverageAcc(ctx, SIZES, 0) as acc:
        acc.set_thresholds(lst)
        _feed(acc, entries)
        uq, tot = _finish_and_check(acc, entries, lst)
        assert 70001 > int(uq[4, 0]) > 0 and int(tot[4, 0]) > int(uq[4, 0])   # (a total of 0 passes no threshold: some rows have no other)
        if lst[-1] == TOP:
            assert not uq[:, -1].any() and not tot[:, -1].any()     # the top value exceeds every total
        d = acc.finish_target()                                # the main counters: everything above min_kmer_hits = 0
        for m, (rows, totals) in enumerate(entries):
            assert (int(d[0][m]), int(d[1][m])) == (len(np.unique(rows[totals > 0])), int((totals > 0).sum()))


def test_one_row_three_totals_and_the_last_row_alone(ctx):
    with sk.CoverageAcc(ctx, SIZES, 1) as acc:
        acc.set_thresholds([0, 4, 8, 12])
        acc.add_rows_hits(3, [200, 200, 200], [1, 5, 9])
        uq, tot = acc.finish_target_thresholds()
        assert uq[3].tolist() == [1, 1, 1, 0] and tot[3].tolist() == [3, 2, 1, 0]
        assert not uq[[0, 1, 2, 4]].any() and not tot[[0, 1, 2, 4]].any()
        assert [x.tolist() for x in acc.finish_target()] == [[0, 0, 0, 1, 0], [0, 0, 0, 2, 0]]        # 5 and 9 exceed min_kmer_hits = 1
        entries = [(np.array([n - 1] * (m + 1), dtype=np.uint32), np.array([4, 5, 13, 8, 9][: m + 1], dtype=np.uint32)) if n else
                   (np.zeros(0, dtype=np.uint32),) * 2 for m, n in enumerate(SIZES)]
        _feed(acc, entries)
        uq, tot = _finish_and_check(acc, entries, [0, 4, 8, 12])
        assert uq[:, 0].tolist() == [0, 1, 1, 1, 1] and tot[4].tolist() == [5, 4, 2, 1]
        acc.finish_target()


def test_300000_entries_on_one_row_over_all_classes(ctx):
    lst = list(range(16))
    totals = (np.arange(300000) % 18).astype(np.uint32)       # classes 0 .. 16, 16 twice
    with sk.CoverageAcc(ctx, SIZES, 0) as acc:
        acc.set_thresholds(lst)
        acc.add_rows_hits(3, np.full(300000, 100, dtype=np.uint32), totals)
        acc.add_rows_hits(4, np.full(300000, 70000, dtype=np.uint32), totals[::-1].copy())
        uq, tot = acc.finish_target_thresholds()
        want = [int((totals > t).sum()) for t in lst]
        assert tot[3].tolist() == want == tot[4].tolist() and uq[3].tolist() == [1] * 16 == uq[4].tolist()
        assert not uq[:3].any() and not tot[:3].any()
        assert acc.finish_target()[1].tolist() == [0, 0, 0, want[0], want[0]]


@pytest.mark.parametrize("primary", [0, 5, 100])              # below t[0], inside the list, above its top
def test_the_sweeps_return_what_they_return_without_thresholds(ctx, primary):
    lst = [2, 4, 8, 16]
    rng = np.random.default_rng(primary)
    entries = _entries(lst, rng, primary)
    got = {}
    with sk.CoverageAcc(ctx, SIZES, primary) as acc:
        for on in (False, True):
            acc.set_thresholds(lst if on else [])
            for sweep in ("plain", "regions", "spectrum"):
                _feed(acc, entries)
                if on:
                    _finish_and_check(acc, entries, lst)       # the pass in front: the depth counters stay
                    for m, (rows, totals) in enumerate(entries):
                        assert np.array_equal(acc.rows(m), _depth(SIZES[m], rows, totals, primary)), m
                if sweep == "spectrum":
                    acc.set_spectrum(3)
                got[on, sweep] = {"plain": acc.finish_target, "regions": acc.finish_target_regions,
                                  "spectrum": acc.finish_target_spectrum}[sweep]()
                acc.set_spectrum(0)
    for sweep in ("plain", "regions", "spectrum"):
        for a, b in zip(got[False, sweep][:2] + (got[False, sweep][2:4] if sweep == "spectrum" else ()),
                        got[True, sweep][:2] + (got[True, sweep][2:4] if sweep == "spectrum" else ())):
            assert np.array_equal(a, b)
    depth = [_depth(SIZES[m], r, t, primary) for m, (r, t) in enumerate(entries)]
    assert got[True, "plain"][0].tolist() == [int(np.count_nonzero(d)) for d in depth]
    assert got[True, "plain"][1].tolist() == [int(d.sum()) for d in depth] and got[True, "plain"][1][4] > 0


def test_set_thresholds_discards_and_bad_calls(ctx):
    with sk.CoverageAcc(ctx, [10, 300], 2) as acc:
        with pytest.raises(sk.SKError) as e:
            acc.finish_target_thresholds()                     # off after create
        assert e.value.code == SK_E_STATE
        acc.add_rows_hits(1, [7, 7, 8], [3, 2, 9])             # thresholds off: the main counters alone
        assert [x.tolist() for x in acc.finish_target()] == [[0, 2], [0, 2]]
        for bad in ([1, 1], [2, 1], [-1], [TOP + 1], [0, 5, 5], list(range(17)), [0, 1, 2, 1]):
            with pytest.raises(sk.SKError) as e:
                acc.set_thresholds(bad)
            assert e.value.code == SK_E_ARG, bad
        acc.set_thresholds([0, TOP])
        acc.set_thresholds([1, 3])
        with pytest.raises(sk.SKError) as e:
            acc.add_rows(0, [1, 2])                            # filtered rows carry no totals
        assert e.value.code == SK_E_STATE
        acc.add_rows_hits(0, [9, 9, 1], [2, 4, 1])
        acc.add_rows_hits(1, [299], [50])
        acc.set_thresholds([1, 2])                             # between targets: what was classified is gone, the depth counters stay
        acc.add_rows_hits(1, [0, 0], [3, 2])
        uq, tot = acc.finish_target_thresholds()
        assert uq.tolist() == [[0, 0], [1, 1]] and tot.tolist() == [[0, 0], [2, 1]]
        assert [x.tolist() for x in acc.finish_target()] == [[1, 2], [1, 2]]
        acc.set_thresholds([])
        with pytest.raises(sk.SKError):
            acc.finish_target_thresholds()
        acc.add_rows(0, [1, 2])                                # ... and the filtered call works again
        assert acc.finish_target()[1].tolist() == [2, 0]


# ---------------------------------------------------------------------------------------------------------------------------------
# real launches (the world of test_coverage_regions_gpu.py)
# ---------------------------------------------------------------------------------------------------------------------------------
T_REAL = [0, 1, 3, 5, 10, 30, 100, 400]


def _check_real(acc, nrows, ns, is_union, sides, npairs, primary, lst=T_REAL):
    uq, tot = acc.finish_target_thresholds()
    some = False
    for q, t in enumerate(lst):
        want = model(nrows, ns, is_union, sides, npairs, t)
        assert uq[:, q].tolist() == [int(np.count_nonzero(d)) for d in want], t
        assert tot[:, q].tolist() == [int(d.sum()) for d in want], t
        some |= q > 0 and 0 < int(tot[:, q].sum()) < int(tot[:, 0].sum())
    assert some                                                # the list cuts somewhere inside the totals
    want = model(nrows, ns, is_union, sides, npairs, primary)
    d = acc.finish_target()
    assert d[0].tolist() == [int(np.count_nonzero(x)) for x in want] and d[1].tolist() == [int(x.sum()) for x in want]
    again = acc.finish_target_thresholds()
    assert not again[0].any() and not again[1].any()


@pytest.mark.parametrize("primary", [0, 5, 1000])
def test_union_of_three(world, primary):  # noqa: F811
    w, u = world, world.union
    r1, h1 = w.uni[0]
    with sk.CoverageAcc(w.ctxs[0], w.nrows, primary) as acc:
        acc.set_thresholds(T_REAL)
        u.tally_launch(w.b1, results_stay=True)
        u.tally_collect_counts()
        acc.add(u, 0, 1, w.b1.nrec)
        _check_real(acc, w.nrows, 3, True, [(r1, h1, w.st1, 0, 1)], w.b1.nrec, primary)


def test_single_reads_interleaved_pairs_and_pairs_over_two_batches(world):  # noqa: F811
    w, primary = world, 5
    (r1, h1), (r2, h2) = w.single
    c = w.ctxs[1]
    np_ = w.b1.nrec // 2
    with sk.CoverageAcc(c, [w.nrows[1]], primary) as acc:
        acc.set_thresholds(T_REAL)
        c.tally_launch(w.b1)
        c.tally_collect_counts()
        acc.add(c, 0, 1, w.b1.nrec)
        _check_real(acc, [w.nrows[1]], 1, False, [(r1, h1, w.st1, 0, 1)], w.b1.nrec, primary)
        c.tally_launch(w.b1)
        c.tally_collect_counts()
        acc.add(c, 0, 2, np_, mate=("same", 1, 2))             # interleaved pairs from record 0 ...
        _check_real(acc, [w.nrows[1]], 1, False, [(r1, h1, w.st1, 0, 2), (r1, h1, w.st1, 1, 2)], np_, primary)
        c.tally_launch(w.b1)
        c.tally_collect_counts()
        acc.add(c, 1, 2, np_ - 1, mate=("same", 2, 2))         # ... and from record 1
        _check_real(acc, [w.nrows[1]], 1, False, [(r1, h1, w.st1, 1, 2), (r1, h1, w.st1, 2, 2)], np_ - 1, primary)
        c.tally_launch(w.b1)
        c.tally_collect_counts()
        acc.hold(c)
        c.tally_launch(w.b2)
        c.tally_collect_counts()
        acc.add(c, 4, 1, w.b1.nrec - 4, mate=("held", 2, 1))
        _check_real(acc, [w.nrows[1]], 1, False, [(r2, h2, w.st2, 4, 1), (r1, h1, w.st1, 2, 1)], w.b1.nrec - 4, primary)


def test_union_of_32_members():
    """SK_UNION_MAX members of a few hundred bases: member 31's bins of the fold's LDS table"""
    rng = random.Random(3232)
    M = native.SK_UNION_MAX
    assert M == 32
    genomes = [_synth.rand_dna(rng, 300 + 7 * i) for i in range(M)]
    ctxs, sets = [], []
    try:
        for g in genomes:
            ks = sk.Keyset.from_stream(g + b"\n", initial_slots=STRAIN_ORDER, default_val=1, incr=0)
            c = sk.KmerContext(0)
            c.load_keyset(ks, 6)
            typ = np.full(ks.nrows, 1, dtype=np.uint32)
            typ[::5] = 2
            c.set_counts(0, typ)
            ctxs.append(c)
            sets.append(ks)
        reads = []
        for i in range(400):
            g = genomes[(i * 7) % M] if i % 3 else genomes[M - 1]
            ln = rng.choice([31, 40, 75, 120])
            a = rng.randrange(len(g) - ln)
            reads.append(g[a:a + ln] if i % 2 else _synth.revcomp(g[a:a + ln]))
        s, st = _stream(reads)
        b = native.TallyBatch(ctxs[0])
        b.fill(s, st)
        u = sk.KmerUnion(ctxs, 0, 2)
        try:
            u.tally_launch(b)
            recs, hits = _union_collect(u, b)
            nrows = [k.nrows for k in sets]
            lst = [0, 2, 8, 20, 60]
            with sk.CoverageAcc(ctxs[0], nrows, 8) as acc:
                acc.set_thresholds(lst)
                u.tally_launch(b, results_stay=True)
                u.tally_collect_counts()
                acc.add(u, 0, 1, b.nrec)
                uq, tot = acc.finish_target_thresholds()
                for q, t in enumerate(lst):
                    want = model(nrows, M, True, [(recs, hits, st, 0, 1)], b.nrec, t)
                    assert uq[:, q].tolist() == [int(np.count_nonzero(d)) for d in want], t
                    assert tot[:, q].tolist() == [int(d.sum()) for d in want], t
                assert int(tot[M - 1, 0]) > int(tot[M - 1, -1]) and int(uq[M - 1, 0]) > 0 and int(tot[0, 0]) > 0
                assert np.array_equal(acc.finish_target()[1], tot[:, 2])                    # min_kmer_hits = 8 is in the list
        finally:
            u.close()
            b.close()
    finally:
        for c in ctxs:
            c.close()
        for k in sets:
            k.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# sk_distinct_thresholds
# ---------------------------------------------------------------------------------------------------------------------------------
def _distinct_check(ctx, keys, sample, totals, nsamples, lst):
    keys, sample, totals = np.asarray(keys, dtype=np.uint64), np.asarray(sample, dtype=np.uint32), np.asarray(totals, dtype=np.uint32)
    uq, tot = ctx.distinct_thresholds(keys, sample, totals, nsamples, lst)
    assert uq.shape == tot.shape == (nsamples, len(lst))
    for s in range(nsamples):
        wu, wt = _numbers(keys[sample == s].astype(np.int64), totals[sample == s], lst)
        assert uq[s].tolist() == wu and tot[s].tolist() == wt, s
    for q, t in enumerate(lst):                                 # sk_distinct_count on the lines above t: the same two numbers
        keep = totals.astype(np.int64) > t
        u2, t2 = ctx.distinct_count(keys[keep], sample[keep], nsamples)
        assert np.array_equal(u2, uq[:, q]) and np.array_equal(t2, tot[:, q])
    return uq, tot


def test_distinct_thresholds(ctx):
    rng = np.random.default_rng(99)
    _distinct_check(ctx, [], [], [], 3, [0, 1])                                          # n = 0
    _distinct_check(ctx, rng.integers(0, 40, 500), np.zeros(500), rng.integers(0, 12, 500), 1, [0, 4, 5, 11, 12])     # one sample
    smp = np.repeat(np.arange(257), np.arange(257) % 23)                                 # 257 samples, some of them empty
    keys = rng.integers(0, 2 ** 40, len(smp), dtype=np.uint64)
    keys[::3] = keys[1::3][: len(keys[::3])]
    order = rng.permutation(len(smp))
    uq, tot = _distinct_check(ctx, keys[order], smp[order], rng.integers(0, 9, len(smp)), 257, list(range(16)))
    assert not tot[0].any() and tot[22, 0] > 0 and not tot[:, 8:].any()
    uq, tot = _distinct_check(ctx, [5, 5, 5, 6], [1, 1, 1, 1], [1, 5, 9, 0], 3, [0, 4, 8, 12])     # a key whose lines carry different totals
    assert uq.tolist() == [[0] * 4, [1, 1, 1, 0], [0] * 4] and tot[1].tolist() == [3, 2, 1, 0]
    uq, tot = _distinct_check(ctx, [1, 2], [0, 0], [2 ** 32 - 1, TOP], 1, [TOP])
    assert (uq.tolist(), tot.tolist()) == ([[1]], [[1]])
    with pytest.raises(sk.SKError) as e:
        ctx.distinct_thresholds([1, 2], [0, 3], [1, 1], 3, [0])
    assert e.value.code == SK_E_ARG
    for bad in ([], [1, 1], [3, 2], [-1], [TOP + 1], list(range(17))):
        with pytest.raises(sk.SKError) as e:
            ctx.distinct_thresholds([1], [0], [1], 1, bad)
        assert e.value.code == SK_E_ARG, bad


def _cov_case(name):
    d = os.path.join(COV_CASES, name)
    prepare_cov_case(name, d)
    meta = json.load(open(os.path.join(d, "case.json")))
    argv = meta["argv"]
    hits = argv[argv.index("-k") + 1]
    m = 1
    for flag in ("-m", "--min_kmer_hits"):
        if flag in argv:
            m = int(argv[argv.index(flag) + 1])
    return d, meta, hits, m


@pytest.mark.parametrize("name", sorted(set(os.listdir(COV_CASES)) - {"general_text", "short_line", "zero_informative"}))
def test_coverage_depth_thresholds_on_the_golden_hit_lists(tmp_path, name):
    d, meta, hits, m = _cov_case(name)
    want_main = open(os.path.join(d, "expected.stdout"), "rb").read()
    text = gzip.open(os.path.join(d, hits), "rb").read()
    for lst in (None, [m], [0, m + 1, 7]):
        out = tmp_path / ("th%d.tsv" % len(lst or DEFAULT))
        p = subprocess.run([sk.cli_path("coverage_depth")] + meta["argv"] + ["--thresholds=" + str(out)] +
                           (["--threshold-list", ",".join(map(str, lst))] if lst else []), cwd=d, capture_output=True)
        assert (p.returncode, p.stdout) == (0, want_main), p.stderr.decode()[-500:]       # the main table's bytes are unchanged
        got = out.read_bytes()
        assert got == table_from_hits(text, hits, lst or DEFAULT, m)
        check_invariants(got, want_main, lst or DEFAULT, m)
        if lst == [m]:                                                                   # ... and the reference's two numbers
            assert {s: r[0][1:] for s, r in parse_table(got).items()} == {s: (max(u, 0), n) for s, (u, n) in main_table(want_main).items()}


def test_coverage_depth_refuses_general_text(tmp_path):
    d, meta, hits, m = _cov_case("general_text")
    out = tmp_path / "th.tsv"
    p = subprocess.run([sk.cli_path("coverage_depth")] + meta["argv"] + ["--thresholds=" + str(out)], cwd=d, capture_output=True)
    assert p.returncode != 0 and p.stdout == b"" and p.stderr.count(b"\n") == 1 and b"--thresholds" in p.stderr
    assert not out.exists()


# ---------------------------------------------------------------------------------------------------------------------------------
# the programs: the job of test_coverage_spectrum_gpu.py (SE .gz with reads shorter than k -- so runs are replayed on the host and
# reach the device through add_rows_hits --, PE over two files, PEI), a target without a hit, interleaved pairs whose last read has
# no mate, and two targets with one basename
# ---------------------------------------------------------------------------------------------------------------------------------
SUFFIXES = ("coverage_depth", "coverage_thresholds", "coverage_spectrum", "coverage_regions", "coverage_recurrence", "kmer_hits.gz")
LST = [0, 1, 2, 30, 150, 400]
TH = ["--coverage-thresholds", "--threshold-list", ",".join(map(str, LST))]


@pytest.fixture(scope="module")
def tjob(job):  # noqa: F811
    r = random.Random(77)
    h = job.hit
    some = [_synth.rand_dna(r, 80) for _ in range(30)]
    odd = some[:11] + [h, _synth.revcomp(h), h[20:100]] + some[11:]
    odd = odd if len(odd) % 2 else odd + [h]
    (job.d / "th_none.fa").write_bytes(_fa([_synth.rand_dna(r, 80) for _ in range(100)]))
    (job.d / "th_odd.fa").write_bytes(_fa(odd))
    (job.d / "T5.txt").write_text(f"SE\t{job.d}/se.fq.gz\nSE\t{job.d}/th_none.fa\nPE\t{job.d}/pe_1.fa\t{job.d}/pe_2.fa\nPEI\t{job.d}/il.fq\n"
                                  f"PEI\t{job.d}/th_odd.fa\n")
    return job


def _prog(job, tag, flags, strains=(1,), targets="T5.txt", env=None):  # noqa: F811
    d = job.d / ("thr_" + tag)
    d.mkdir()
    if len(strains) > 1:
        (d / "S.txt").write_text("".join(f"{job.d}/s{s}.fa\t{job.d}/s{s}.inf.gz\t{d}/{NAME % s}\n" for s in strains))
        argv = ["-S", str(d / "S.txt")]
    else:
        s = strains[0]
        argv = ["-r", str(job.d / f"s{s}.fa"), "-a", str(job.d / f"s{s}.inf.gz"), "-o", str(d / (NAME % s))]
    rc, err, stats = _run_sd(argv + ["-B", str(job.d / targets)] + flags, dict(SMALL_CHUNKS, SK_SD_RESULT_BYTES="1", **(env or {})), d, "run")
    assert rc == 0, err.decode()[-600:]
    out = {}
    for s in strains:
        b = _base(d / (NAME % s))
        out[s] = {x: open(b + "." + x, "rb").read() for x in SUFFIXES if os.path.exists(b + "." + x)}
    return out, stats, err, open(d / "run.out", "rb").read()


def test_program_every_form_gives_the_models_table(tjob):
    plain, _, perr, pout = _prog(tjob, "plain_depth", ["--coverage-depth"])                # a -o run without the flag: the model's input
    hits = str(tjob.d / "thr_plain_depth" / (NAME % 1))
    text = gzip.decompress(plain[1]["kmer_hits.gz"])
    want = table_from_hits(text, hits, LST, 1)
    rows = parse_table(want)
    assert list(rows) == [b"se.fq.gz", b"pe_1.fa", b"il.fq", b"th_odd.fa", b"th_none.fa"]
    assert rows[b"th_none.fa"] == [(t, 0, 0) for t in LST] and rows[b"se.fq.gz"][0][2] > rows[b"se.fq.gz"][3][2] > 0
    only, stats, err, out = _prog(tjob, "only", ["--coverage-only"] + TH)
    assert WENT.search(err) and stats[0] > 0 and stats[1] > 0 and stats[2] == 0, stats    # folded on the device AND replayed
    depth, _, derr, dout = _prog(tjob, "depth", ["--coverage-depth"] + TH)
    for got in (only, depth):
        assert got[1]["coverage_thresholds"] == want
        assert got[1]["coverage_depth"] == plain[1]["coverage_depth"]
    assert "kmer_hits.gz" not in only[1] and gzip.decompress(depth[1]["kmer_hits.gz"]) == text
    assert (dout, derr) == (pout, perr)                                                   # stdout and stderr are the unflagged run's
    ponly, _, poerr, poout = _prog(tjob, "plain_only", ["--coverage-only"])
    assert (out, err) == (poout, poerr) and ponly[1] == {"coverage_depth": plain[1]["coverage_depth"]}
    check_invariants(want, plain[1]["coverage_depth"], LST, 1)
    # each line equals the main table of a separate run with that --min-kmer-hits
    for q, t in enumerate(LST):
        sep, _, _, _ = _prog(tjob, "sep%d" % t, ["--coverage-only", "--min-kmer-hits", str(t)])
        mt = main_table(sep[1]["coverage_depth"])
        assert {s: r[q][1:] for s, r in rows.items()} == {s: (max(u, 0), n) for s, (u, n) in mt.items()}, t
    # the run's own --min-kmer-hits inside the list and above it: the same thresholds table, another main table
    for m in (30, 1000):
        for table in ("--coverage-only", "--coverage-depth"):
            a, _, _, _ = _prog(tjob, "m%d%s" % (m, table), [table, "--min-kmer-hits", str(m)] + TH)
            b, _, _, _ = _prog(tjob, "m%dplain%s" % (m, table), [table, "--min-kmer-hits", str(m)])
            assert parse_table(a[1]["coverage_thresholds"]) == {s: rows[s] for s in main_table(b[1]["coverage_depth"])}
            assert a[1]["coverage_depth"] == b[1]["coverage_depth"]
            check_invariants(a[1]["coverage_thresholds"], a[1]["coverage_depth"], LST, m)
    # coverage_depth --thresholds on the -o list of the same job; the default list and path; an explicit file
    o1 = tjob.d / "cd_thr.tsv"
    p = subprocess.run([sk.cli_path("coverage_depth"), "-k", hits, "--thresholds=" + str(o1), "--threshold-list", TH[2]], capture_output=True)
    assert (p.returncode, p.stdout) == (0, plain[1]["coverage_depth"]), p.stderr.decode()[-400:]
    assert o1.read_bytes() == want
    dflt, _, _, _ = _prog(tjob, "default", ["--coverage-only", "--coverage-thresholds"])
    assert dflt[1]["coverage_thresholds"] == table_from_hits(text, hits, DEFAULT, 1)
    expl, _, _, _ = _prog(tjob, "explicit", ["--coverage-only", "--coverage-thresholds=" + str(tjob.d / "x.tsv"), "--threshold-list=" + TH[2]])
    assert (tjob.d / "x.tsv").read_bytes() == want and "coverage_thresholds" not in expl[1]
    shutil.copy(hits, tjob.d / "copy.kmer_hits.gz")
    p = subprocess.run([sk.cli_path("coverage_depth"), "-k", "copy.kmer_hits.gz", "--thresholds"], cwd=tjob.d, capture_output=True)
    assert p.returncode == 0 and (tjob.d / "copy.coverage_thresholds").read_bytes() == table_from_hits(text, "copy.kmer_hits.gz", DEFAULT, 1)


def test_program_many_strains_unions_devices_the_cache_and_the_other_tables(tjob):
    md, _, _, _ = _prog(tjob, "S_plain", ["--coverage-depth"], strains=(0, 1, 2))
    want = {s: table_from_hits(gzip.decompress(md[s]["kmer_hits.gz"]), str(tjob.d / "thr_S_plain" / (NAME % s)), LST, 1) for s in (0, 1, 2)}
    assert want[1] != want[2]                                                            # (the related strain)
    extra = ["--coverage-regions", "--region-window", "500", "--coverage-spectrum", "--spectrum-max", "3", "--coverage-recurrence"]
    ref, _, _, _ = _prog(tjob, "S_other", ["--coverage-only"] + extra, strains=(0, 1, 2))
    cache = tjob.d / "thr_cache"
    cache.mkdir()
    forms = [("S", {}, []), ("dev2", {"SK_DEVICES": "0,0", "SK_SD_GROUP": "2"}, []), ("nounion", {"SK_SD_NO_UNION": "1"}, []),
             ("S_all", {}, extra), ("cache_fill", {"SK_SD_TIMING": "1"}, ["--target-cache", str(cache)]),
             ("cache_served", {"SK_SD_TIMING": "1"}, ["--target-cache", str(cache)])]
    for form, env, flags in forms:
        for table in ("--coverage-only", "--coverage-depth") if form == "S" else ("--coverage-only",):
            many, st, err, _ = _prog(tjob, form + table, [table] + TH + flags, strains=(0, 1, 2), env=env)
            if form.startswith("cache"):                                                 # (served, written, stale, not cached)
                cs = _skt.stats(err)
                assert cs and (cs[1] > 0 and cs[0] == 0 if form == "cache_fill" else cs[0] > 0 and cs[1] == 0), (form, cs)
            for s in (0, 1, 2):
                assert many[s]["coverage_thresholds"] == want[s], (form, table, s)
                assert many[s]["coverage_depth"] == md[s]["coverage_depth"]
                if flags == extra:                                                       # the other tables beside it are what they are without it
                    for x in ("coverage_regions", "coverage_spectrum", "coverage_recurrence"):
                        assert many[s][x] == ref[s][x] and len(ref[s][x]) > 40, x
            if table == "--coverage-only":
                assert st[0] > 0 and st[2] == 0
    assert os.listdir(cache)
    one, _, _, _ = _prog(tjob, "one_of_S", ["--coverage-only"] + TH)                       # one strain and -S: the same table
    assert one[1]["coverage_thresholds"] == want[1]


def test_program_two_targets_with_one_basename(tjob):
    """the host path: both targets are one sample, counted by the host accumulator"""
    only, stats, err, _ = _prog(tjob, "dup_only", ["--coverage-only"] + TH, targets="dup.txt")
    depth, _, _, _ = _prog(tjob, "dup_depth", ["--coverage-depth"] + TH, targets="dup.txt")
    assert stats[2] == 2 and stats[0] == 0 and err.count(b"share a file name") == 1
    hits = str(tjob.d / "thr_dup_depth" / (NAME % 1))
    want = table_from_hits(gzip.open(hits, "rb").read(), hits, LST, 1)
    assert only[1]["coverage_thresholds"] == depth[1]["coverage_thresholds"] == want
    assert list(parse_table(want)) == [b"same.fa"] and parse_table(want)[b"same.fa"][0][2] > 0
    check_invariants(want, only[1]["coverage_depth"], LST, 1)


def test_program_fused_with_the_scrub(golden, tjob):
    """kmer_scrub_count -S .. --scrub .. --detect .. --coverage-thresholds on the bundled pair: both modes write the model's table,
    computed from the hit lists --coverage-depth writes; the coverage tables are the reference chain's"""
    facts = json.load(open(os.path.join(golden, "pair_workflow_facts.json")))
    b = tjob.d / "thr_bundled_pair"
    b.mkdir()
    src = os.path.join(golden, "bundled")
    for n in ("strains", "metagenomes"):
        os.symlink(os.path.join(src, n), b / n)
    for n in ("genomes_to_scrub.txt", "metagenomes_to_scrub.txt", "target_metagenomes.txt"):
        shutil.copy(os.path.join(src, n), b / n)
    (b / facts["c_name"]).write_text("".join(ln + "\n" for ln in facts["c_list"]))
    c = facts["cases"]["plain"]
    lst = [0, 1, 5, 20]
    got = {}
    for flag in ("--coverage-depth", "--coverage-only"):
        t = tjob.d / ("thr_pair" + flag)
        t.mkdir()
        base = {n: str(t / os.path.basename(g)[: -len(".fna.gz")]) for n, g in facts["strains"].items()}
        with open(t / "S.txt", "w") as f:
            for n, g in facts["strains"].items():
                f.write("\t".join((g, base[n] + ".scrubbed_kmers", base[n] + ".kmer_hits.gz")) + "\n")
        argv = (["-S", str(t / "S.txt"), "-A", "genomes_to_scrub.txt", "-B", "metagenomes_to_scrub.txt"] + c["kmer_scrub_count"] +
                ["--scrub", facts["min_fraction"], "--detect"] + facts["detect_args"] +
                [flag, "--coverage-thresholds", "--threshold-list", ",".join(map(str, lst))])
        p = subprocess.run([sk.cli_path()] + argv, cwd=str(b), capture_output=True, env=dict(os.environ, SK_SD_RESULT_BYTES="1"))
        assert p.returncode == 0, p.stderr.decode()[-800:]
        for n in base:
            assert hashlib.md5(open(base[n] + ".coverage_depth", "rb").read()).hexdigest() == c["strains"][n]["coverage_md5"], (flag, n)
        got[flag] = {n: open(base[n] + ".coverage_thresholds", "rb").read() for n in base}
        if flag == "--coverage-depth":
            for n in base:
                want = table_from_hits(gzip.open(base[n] + ".kmer_hits.gz", "rb").read(), base[n] + ".kmer_hits.gz", lst, 1)
                assert got[flag][n] == want and want.count(b"\n") > len(lst), n
                check_invariants(want, open(base[n] + ".coverage_depth", "rb").read(), lst, 1)
        else:
            went = WENT.search(p.stderr)
            assert went and int(went.group(1)) >= 2
    assert got["--coverage-depth"] == got["--coverage-only"]
