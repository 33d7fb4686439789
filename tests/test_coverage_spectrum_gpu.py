"""The depth spectrum on the device (include/strainer_kmer.h has the rule): the sweep that ends a target
(sk_covacc_set_spectrum / sk_covacc_finish_target_spectrum), sk_distinct_spectrum, and the programs in every form they run in,
all against tests/_spectrum_model.py.

Library level: accumulators are built from row counts alone and fed through add_rows, which sets exact depths cheaply; members of
0, 1, 255, 257 and 70 001 rows sit in one accumulator (70 001 rows are more than 256 workgroups x 256 threads, so the grid-stride
loop turns more than once and max_rows differs from every other member's).  Real launches run in the world of
test_coverage_regions_gpu.py, their expected depths come from test_coverage_only_gpu.py's model()."""
import gzip
import hashlib
import json
import os
import random
import shutil
import subprocess

import numpy as np
import pytest

import _synth
import strainer2_amd as sk
from _spectrum_model import check_invariants, parse_table, spectrum, table_from_hits
from test_coverage_only_gpu import NAME, WENT, _canon, _fa, _fq, _mutate, model
from test_coverage_regions_gpu import _base, _run_sd, fold, world  # noqa: F401  (world: the fixture)

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 255, 257, 70001]
SK_E_ARG = -3


def _feed(acc, depths):
    for m, d in enumerate(depths):
        if len(d):
            acc.add_rows(m, np.repeat(np.arange(len(d), dtype=np.uint32), d))


def _expect(depths, D):
    sp = [spectrum(d, D) for d in depths]
    return (np.array([np.count_nonzero(d) for d in depths], dtype=np.uint64), np.array([int(d.astype(np.int64).sum()) for d in depths], dtype=np.uint64),
            np.array([s[0] for s in sp], dtype=np.uint64).reshape(len(depths), D + 1), np.array([s[1] for s in sp], dtype=np.uint64))


def _sweep_and_check(acc, depths, D, regions=False):
    got = acc.finish_target_spectrum(regions=regions)
    for g, w, what in zip(got[:4], _expect(depths, D), ("unique", "total", "spectrum", "deep")):
        assert np.array_equal(g, w), what
    for m in range(len(depths)):                               # every counter is zero ...
        assert not acc.rows(m).any()
    again = acc.finish_target_spectrum(regions=regions)        # ... and a second call returns zeros
    assert not any(np.asarray(x).any() for x in again[:4])
    return got


@pytest.fixture(scope="module")
def ctx():
    with sk.KmerContext(0) as c:
        yield c


def _around(n, D, rng):
    """a member of n rows with rows at depth D - 1, D, D + 1 and 70 000 (as many of them as n has room for), the deepest last, and
    about 1 % of the others at depth 1"""
    d = np.zeros(n, dtype=np.uint32)
    if n > 8:
        d[rng.choice(n, max(n // 100, 1), replace=False)] = 1
    want = [D + 1, D, D - 1, 70000]
    at = [0, n // 3, n // 2, n - 1]
    for k in range(min(n, 4)):
        d[at[k] if n >= 4 else k] = want[k]
    return d


@pytest.mark.parametrize("D", [1, 2, 64, 1023])
def test_members_of_every_size_with_depths_around_the_maximum(ctx, D):
    rng = np.random.default_rng(D)
    depths = [_around(n, D, rng) for n in SIZES]
    with sk.CoverageAcc(ctx, SIZES, 0) as acc:
        acc.set_spectrum(D)
        _feed(acc, depths)
        uq, tot, spec, deep = _sweep_and_check(acc, depths, D)
        # 70 000 lies above every D: its hits are a sum of depths, which one u32 bin times its depth could not hold for many rows
        assert int(deep[4]) == 70000 + D + 1 and int(spec[4, D]) == 2 and int(spec[4, D - 1]) >= 1
        assert spec[0].tolist() == [0] * (D + 1) and int(spec[1].sum()) == 1 and int(spec[1, D]) == 1
        assert int(spec[:, :D].dot(np.arange(1, D + 1, dtype=np.uint64)).sum() + deep.sum()) == int(tot.sum())     # the hits sum to the total


def test_every_row_in_one_bin_no_row_at_all_and_the_last_row_alone(ctx):
    with sk.CoverageAcc(ctx, SIZES, 0) as acc:
        acc.set_spectrum(3)
        ones = [np.ones(n, dtype=np.uint32) for n in SIZES]    # all 70 001 rows at depth 1: every LDS add on one bin
        _feed(acc, ones)
        _, _, spec, deep = _sweep_and_check(acc, ones, 3)
        assert spec[:, 0].tolist() == SIZES and not spec[:, 1:].any() and not deep.any()
        _sweep_and_check(acc, [np.zeros(n, dtype=np.uint32) for n in SIZES], 3)
        last = [np.zeros(n, dtype=np.uint32) for n in SIZES]
        for m, d in enumerate(last):
            if len(d):
                d[-1] = m + 2                                  # depths 3, 4, 5, 6 with D = 3: one at D, three above
        _feed(acc, last)
        _, _, spec, deep = _sweep_and_check(acc, last, 3)
        assert spec.tolist() == [[0, 0, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1], [0, 0, 0, 1], [0, 0, 0, 1]] and deep.tolist() == [0, 0, 4, 5, 6]


def test_the_other_sweeps_return_what_they_return_without_the_spectrum(ctx):
    rng = np.random.default_rng(5)
    depths = [_around(n, 7, rng) for n in SIZES]
    with sk.CoverageAcc(ctx, SIZES, 0) as acc:
        got = {}
        for D in (0, 7):
            acc.set_spectrum(D)
            _feed(acc, depths)
            got[D, "plain"] = acc.finish_target()
            _feed(acc, depths)
            got[D, "regions"] = acc.finish_target_regions()
        for a, b in zip(got[0, "plain"] + got[0, "regions"][:2], got[7, "plain"] + got[7, "regions"][:2]):
            assert np.array_equal(a, b) and a.any()
        for (u0, t0), (u7, t7) in zip(got[0, "regions"][2], got[7, "regions"][2]):
            assert np.array_equal(u0, u7) and np.array_equal(t0, t7)
        assert np.array_equal(got[7, "plain"][0], _expect(depths, 7)[0]) and np.array_equal(got[7, "plain"][1], _expect(depths, 7)[1])


def test_bad_calls(ctx):
    with sk.CoverageAcc(ctx, [10], 0) as acc:
        with pytest.raises(sk.SKError):
            acc.finish_target_spectrum()                       # off after create
        for D in (1024, 1 << 20):
            with pytest.raises(sk.SKError) as e:
                acc.set_spectrum(D)
            assert e.value.code == SK_E_ARG
        acc.set_spectrum(1023)
        acc.set_spectrum(5)
        acc.add_rows(0, [9] * 6 + [0])
        uq, tot, spec, deep = acc.finish_target_spectrum()
        assert (uq.tolist(), tot.tolist(), spec.tolist(), deep.tolist()) == ([2], [7], [[1, 0, 0, 0, 0, 1]], [6])
        acc.set_spectrum(0)
        with pytest.raises(sk.SKError):
            acc.finish_target_spectrum()


# ---------------------------------------------------------------------------------------------------------------------------------
# with regions, and real launches (the world of test_coverage_regions_gpu.py)
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("min_hits", [0, 5])
def test_union_of_three_with_regions_in_the_one_sweep(world, min_hits):  # noqa: F811
    """members with 1, 48 and 1500 regions: the last keeps its region pairs in HBM (global atomics) beside the spectrum's LDS bins"""
    w, u, D = world, world.union, 2
    r1, h1 = w.uni[0]
    with sk.CoverageAcc(w.ctxs[0], w.nrows, min_hits) as acc:
        acc.set_spectrum(D)
        for m in range(3):
            acc.set_regions(m, w.ctxs[m], w.starts[m])

        def launch():
            u.tally_launch(w.b1, results_stay=True)
            u.tally_collect_counts()
            acc.add(u, 0, 1, w.b1.nrec)
        want = model(w.nrows, 3, True, [(r1, h1, w.st1, 0, 1)], w.b1.nrec, min_hits)
        launch()
        uq, tot, spec, deep, per = _sweep_and_check(acc, want, D, regions=True)
        assert [len(p[0]) for p in per] == [2, 49, 1501] and all(int(t) > 0 for t in tot)
        for m, d in enumerate(want):                           # the region pairs are the model's ...
            ru, rt = fold(d, w.fp[m], w.starts[m])
            assert np.array_equal(per[m][0], ru) and np.array_equal(per[m][1], rt), m
        launch()
        uq2, tot2, per2 = acc.finish_target_regions()          # ... and finish_target_regions' for the same launch
        assert np.array_equal(uq2, uq) and np.array_equal(tot2, tot)
        assert all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) for a, b in zip(per, per2))
        launch()
        uq3, tot3, spec3, deep3 = acc.finish_target_spectrum() # the spectrum without regions: the same
        assert np.array_equal(spec3, spec) and np.array_equal(deep3, deep) and np.array_equal(uq3, uq) and np.array_equal(tot3, tot)
        if min_hits == 0:
            assert spec[:, D].any()                            # some row is deeper than D


@pytest.mark.parametrize("min_hits", [0, 5])
def test_single_reads_interleaved_pairs_and_pairs_over_two_batches(world, min_hits):  # noqa: F811
    w, D = world, 2
    (r1, h1), (r2, h2) = w.single
    c = w.ctxs[1]
    np_ = w.b1.nrec // 2
    with sk.CoverageAcc(c, [w.nrows[1]], min_hits) as acc:
        acc.set_spectrum(D)
        c.tally_launch(w.b1)
        c.tally_collect_counts()
        acc.add(c, 0, 1, w.b1.nrec)
        uq, _, _, _ = _sweep_and_check(acc, model([w.nrows[1]], 1, False, [(r1, h1, w.st1, 0, 1)], w.b1.nrec, min_hits), D)
        assert int(uq[0]) > 0
        c.tally_launch(w.b1)
        c.tally_collect_counts()
        acc.add(c, 0, 2, np_, mate=("same", 1, 2))
        _sweep_and_check(acc, model([w.nrows[1]], 1, False, [(r1, h1, w.st1, 0, 2), (r1, h1, w.st1, 1, 2)], np_, min_hits), D)
        c.tally_launch(w.b1)
        c.tally_collect_counts()
        acc.hold(c)
        c.tally_launch(w.b2)
        c.tally_collect_counts()
        acc.add(c, 4, 1, w.b1.nrec - 4, mate=("held", 2, 1))
        _sweep_and_check(acc, model([w.nrows[1]], 1, False, [(r2, h2, w.st2, 4, 1), (r1, h1, w.st1, 2, 1)], w.b1.nrec - 4, min_hits), D)


# ---------------------------------------------------------------------------------------------------------------------------------
# sk_distinct_spectrum
# ---------------------------------------------------------------------------------------------------------------------------------
def _distinct_model(keys, sample, nsamples, D):
    uq, tot, spec, deep = (np.zeros(nsamples, dtype=np.uint64), np.zeros(nsamples, dtype=np.uint64),
                           np.zeros((nsamples, D + 1), dtype=np.uint64), np.zeros(nsamples, dtype=np.uint64))
    for s in range(nsamples):
        _, mult = np.unique(keys[sample == s], return_counts=True)
        uq[s], tot[s] = len(mult), int(mult.sum())
        spec[s], deep[s] = spectrum(mult, D)
    return uq, tot, spec, deep


def _distinct_check(ctx, keys, sample, nsamples, D):
    keys, sample = np.asarray(keys, dtype=np.uint64), np.asarray(sample, dtype=np.uint32)
    got = ctx.distinct_spectrum(keys, sample, nsamples, D)
    for g, w, what in zip(got, _distinct_model(keys, sample, nsamples, D), ("unique", "total", "spectrum", "deep")):
        assert np.array_equal(g, w), what
    uq, tot = ctx.distinct_count(keys, sample, nsamples)       # sk_distinct_count on the same input: the same two numbers
    assert np.array_equal(uq, got[0]) and np.array_equal(tot, got[1])
    return got


def test_distinct_spectrum(ctx):
    rng = np.random.default_rng(77)
    _distinct_check(ctx, [], [], 3, 5)                                                  # n = 0
    _distinct_check(ctx, rng.integers(0, 40, 500), np.zeros(500), 1, 4)                 # one sample
    smp = np.repeat(np.arange(300), np.arange(300))                                     # 300 samples with 0, 1, 2, ... keys
    keys = rng.integers(0, 2 ** 62, len(smp), dtype=np.uint64)
    keys[::3] = keys[1::3][: len(keys[::3])]                                            # (some of them twice)
    order = rng.permutation(len(smp))
    got = _distinct_check(ctx, keys[order], smp[order], 300, 1)
    assert not got[0][0] and got[2][:, 1].any()
    keys = np.concatenate([np.full(5000, 12345, dtype=np.uint64), np.arange(5000, dtype=np.uint64) + (1 << 40)])
    got = _distinct_check(ctx, keys, np.ones(10000), 2, 255)                            # one key 5 000 times beside 5 000 singletons
    assert got[2][1, 0] == 5000 and got[2][1, 255] == 1 and got[3][1] == 5000 and not got[2][0].any()
    for D in (1, 2, 64, 1023):                                                          # depths around D
        mult = np.array([D + 1, D, max(D - 1, 1), 1, 70000])
        keys = np.repeat(np.arange(len(mult), dtype=np.uint64) * 977 + 5, mult)
        got = _distinct_check(ctx, rng.permutation(keys), np.full(len(keys), 2), 4, D)
        assert got[2][2, D] == 2 and got[3][2] == 70000 + D + 1
    with pytest.raises(sk.SKError) as e:                                                # an out-of-range sample
        ctx.distinct_spectrum([1, 2], [0, 3], 3, 5)
    assert e.value.code == SK_E_ARG
    for D in (0, 1024):
        with pytest.raises(sk.SKError) as e:
            ctx.distinct_spectrum([1], [0], 1, D)
        assert e.value.code == SK_E_ARG


# ---------------------------------------------------------------------------------------------------------------------------------
# the programs
# ---------------------------------------------------------------------------------------------------------------------------------
class Job:
    pass


@pytest.fixture(scope="module")
def job(tmp_path_factory):
    """four strains of about 3 kbp (1 and 2 related: 2 % apart), every 97th k-mer informative and a block of them at 1000..1060;
    SE (.gz FASTQ), PE over two files and PEI targets with some reads shorter than 31 bases -- so some runs are replayed on the
    host -- and in the SE target the block read 40 times over, so bins above a small D fill"""
    d = tmp_path_factory.mktemp("covspectrum")
    rng = random.Random(424242)
    j = Job()
    j.d = d
    g1 = _synth.rand_dna(rng, 3000)
    j.strains = [_synth.rand_dna(rng, 3100), g1, _mutate(rng, g1, 0.02, (1000, 1100)), _synth.rand_dna(rng, 2900)]
    for s, g in enumerate(j.strains):
        (d / f"s{s}.fa").write_bytes(b">s%d\n%s\n" % (s, g))
        kms = sorted({_canon(g[i:i + 31]) for i in range(s, len(g) - 31, 97)} | {_canon(g[i:i + 31]) for i in range(1000, 1060)})
        with gzip.open(d / f"s{s}.inf.gz", "wb") as f:
            f.write(b"#informative\n" + b"\n".join(kms) + b"\n")

    def reads(n, seed, short_every=0):
        r = random.Random(seed)
        out = []
        for i in range(n):
            ln = r.choice([31, 31, 75, 100, 150, r.randrange(31, 151)])
            if r.random() < 0.4:
                g = j.strains[r.randrange(4)]
                a = r.randrange(900, 1100) if r.random() < 0.5 else r.randrange(0, len(g) - ln)
                rd = g[a:a + ln]
                rd = _synth.revcomp(rd) if r.random() < 0.5 else rd
            else:
                rd = _synth.rand_dna(r, ln)
            out.append(rd)
            if short_every and i % short_every == short_every - 1:
                out.append(rd[: 5 + i % 25])                   # a read shorter than k behind it
        return out

    j.hit = j.strains[1][1000:1100]
    deep = [j.hit if i % 2 else _synth.revcomp(j.hit) for i in range(40)]
    se = reads(600, 1) + deep + reads(300, 5, short_every=60)
    p1, p2 = reads(400, 2, short_every=90), reads(400, 3, short_every=90)
    il = reads(400, 4, short_every=100)
    assert len(p1) == len(p2) and len(il) % 2 == 0 and any(len(x) < 31 for x in se)
    with gzip.open(d / "se.fq.gz", "wb", compresslevel=1) as f:
        f.write(_fq(se))
    (d / "pe_1.fa").write_bytes(_fa(p1))
    (d / "pe_2.fa").write_bytes(_fa(p2))
    (d / "il.fq").write_bytes(_fq(il))
    (d / "T.txt").write_text(f"SE\t{d}/se.fq.gz\nPE\t{d}/pe_1.fa\t{d}/pe_2.fa\nPEI\t{d}/il.fq\n")
    for sub, seed in (("x", 31), ("y", 32)):
        (d / sub).mkdir()
        (d / sub / "same.fa").write_bytes(_fa(reads(60, seed) + [j.hit, _synth.revcomp(j.hit)] * (3 if sub == "x" else 1)))
    (d / "dup.txt").write_text(f"SE\t{d}/x/same.fa\nSE\t{d}/y/same.fa\n")
    return j


SMALL_CHUNKS = {"SK_SD_CHUNK_BYTES": "6000"}                   # chunks of about sixty reads: clean runs between the short reads


def _run(job, tag, flags, strains=(1,), targets="T.txt", env=None):
    """one run of strain_detect in the job: {strain: {suffix: bytes of the file written beside the -o path}}, stats, stderr"""
    d = job.d / tag
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
        out[s] = {x: open(b + "." + x, "rb").read() for x in ("coverage_depth", "coverage_spectrum", "coverage_regions", "kmer_hits.gz")
                  if os.path.exists(b + "." + x)}
    return out, stats, err


@pytest.mark.parametrize("D", [3, None])
def test_program_six_ways_to_one_table(job, D):
    """--coverage-only, --coverage-depth, coverage_depth --spectrum on the hit list the latter wrote, the model on that hit list,
    and the -S and two-device forms of the same job: one table, byte for byte"""
    sp = ["--coverage-spectrum"] + (["--spectrum-max", str(D)] if D else [])
    tag = f"six{D}_"
    only, stats, err = _run(job, tag + "only", ["--coverage-only"] + sp)
    went = WENT.search(err)
    assert went and (int(went.group(1)), int(went.group(2))) == stats[:2]
    assert stats[0] > 0 and stats[1] > 0 and stats[2] == 0, stats                       # both routes: folded on the device AND replayed
    depth, _, _ = _run(job, tag + "depth", ["--coverage-depth"] + sp)
    t = only[1]["coverage_spectrum"]
    assert t == depth[1]["coverage_spectrum"]
    assert only[1]["coverage_depth"] == depth[1]["coverage_depth"] and "kmer_hits.gz" not in only[1]
    hits = str(job.d / (tag + "depth") / (NAME % 1))
    assert t == table_from_hits(gzip.open(hits, "rb").read(), hits, D or 255, 1)
    out = job.d / (tag + "cd.tsv")
    p = subprocess.run([sk.cli_path("coverage_depth"), "-k", hits, "--spectrum=" + str(out)] + (["--spectrum-max", str(D)] if D else []),
                       capture_output=True)
    assert (p.returncode, p.stdout) == (0, depth[1]["coverage_depth"]), p.stderr.decode()[-400:]
    assert out.read_bytes() == t
    check_invariants(t, only[1]["coverage_depth"])
    rows = parse_table(t)
    assert list(rows) == [b"se.fq.gz", b"pe_1.fa", b"il.fq"] and all(r[0][0] == b"0" for r in rows.values())
    if D == 3:                                                                          # the block read 40 times over
        lab, n, h = rows[b"se.fq.gz"][-1]
        assert lab == b">3" and n >= 40 and h >= 40 * n
    else:
        assert any(lab == b"40" or int(lab) > 40 for lab, _, _ in rows[b"se.fq.gz"][1:])
    for form, env in (("S", {}), ("dev2", {"SK_DEVICES": "0,0", "SK_SD_GROUP": "2"}), ("nounion", {"SK_SD_NO_UNION": "1"})):
        many, st, _ = _run(job, tag + form, ["--coverage-only"] + sp, strains=(0, 1, 2), env=env)
        assert many[1]["coverage_spectrum"] == t, form
        assert st[0] > 0 and st[1] > 0
        for s in (0, 2):
            check_invariants(many[s]["coverage_spectrum"], many[s]["coverage_depth"])
        if form == "S":
            md, _, _ = _run(job, tag + "Sdepth", ["--coverage-depth"] + sp, strains=(0, 1, 2))
            for s in (0, 1, 2):
                assert md[s]["coverage_spectrum"] == many[s]["coverage_spectrum"], s
            assert parse_table(many[2]["coverage_spectrum"]) != parse_table(many[1]["coverage_spectrum"])      # (the related strain)


def test_program_without_the_flags_writes_what_it_wrote(job):
    """the flag changes neither the coverage table nor the hit list, and nothing is written for it when it is absent"""
    for table in ("--coverage-only", "--coverage-depth"):
        a, _, _ = _run(job, "plain" + table, [table])
        b, _, _ = _run(job, "flag" + table, [table, "--coverage-spectrum", "--spectrum-max", "9"])
        assert "coverage_spectrum" not in a[1] and "coverage_spectrum" in b[1]
        assert a[1]["coverage_depth"] == b[1]["coverage_depth"]
        if table == "--coverage-depth":
            assert gzip.decompress(a[1]["kmer_hits.gz"]) == gzip.decompress(b[1]["kmer_hits.gz"])


@pytest.mark.parametrize("table", ["--coverage-only", "--coverage-depth"])
def test_program_with_regions_too(job, table):
    rg = ["--coverage-regions", "--region-window", "500"]
    a, _, _ = _run(job, "rg" + table, [table] + rg)
    b, stats, _ = _run(job, "rgsp" + table, [table, "--coverage-spectrum", "--spectrum-max", "3"] + rg)
    c, _, _ = _run(job, "sp" + table, [table, "--coverage-spectrum", "--spectrum-max", "3"])
    assert a[1]["coverage_regions"] == b[1]["coverage_regions"] and a[1]["coverage_regions"].count(b"\n") > 10
    assert b[1]["coverage_spectrum"] == c[1]["coverage_spectrum"] and a[1]["coverage_depth"] == b[1]["coverage_depth"]
    if table == "--coverage-only":
        assert stats[0] > 0 and stats[1] > 0


def test_program_explicit_file(job):
    out = job.d / "explicit.tsv"
    a, _, _ = _run(job, "explicit", ["--coverage-only", "--coverage-spectrum=" + str(out), "--spectrum-max=3"])
    b, _, _ = _run(job, "explicit_default", ["--coverage-only", "--coverage-spectrum", "--spectrum-max", "3"])
    assert "coverage_spectrum" not in a[1] and out.read_bytes() == b[1]["coverage_spectrum"]


def test_program_two_targets_with_one_basename(job):
    """the host path: both targets are one sample, counted by the host accumulator"""
    only, stats, err = _run(job, "dup_only", ["--coverage-only", "--coverage-spectrum", "--spectrum-max", "2"], targets="dup.txt")
    depth, _, _ = _run(job, "dup_depth", ["--coverage-depth", "--coverage-spectrum", "--spectrum-max", "2"], targets="dup.txt")
    assert stats[2] == 2 and stats[0] == 0 and err.count(b"share a file name") == 1
    hits = str(job.d / "dup_depth" / (NAME % 1))
    want = table_from_hits(gzip.open(hits, "rb").read(), hits, 2, 1)
    assert only[1]["coverage_spectrum"] == depth[1]["coverage_spectrum"] == want
    rows = parse_table(want)
    assert list(rows) == [b"same.fa"] and rows[b"same.fa"][-1][0] == b">2"
    check_invariants(want, only[1]["coverage_depth"])


def test_program_fused_with_the_scrub(golden, job):
    """kmer_scrub_count -S .. --scrub .. --detect .. --coverage-spectrum on the bundled pair: both modes write the model's table,
    computed from the hit lists --coverage-depth writes; the coverage tables are the reference chain's"""
    facts = json.load(open(os.path.join(golden, "pair_workflow_facts.json")))
    b = job.d / "bundled_pair"
    b.mkdir()
    src = os.path.join(golden, "bundled")
    for n in ("strains", "metagenomes"):
        os.symlink(os.path.join(src, n), b / n)
    for n in ("genomes_to_scrub.txt", "metagenomes_to_scrub.txt", "target_metagenomes.txt"):
        shutil.copy(os.path.join(src, n), b / n)
    (b / facts["c_name"]).write_text("".join(ln + "\n" for ln in facts["c_list"]))
    c = facts["cases"]["plain"]
    got = {}
    for flag in ("--coverage-depth", "--coverage-only"):
        t = job.d / ("pair" + flag)
        t.mkdir()
        base = {n: str(t / os.path.basename(g)[: -len(".fna.gz")]) for n, g in facts["strains"].items()}
        with open(t / "S.txt", "w") as f:
            for n, g in facts["strains"].items():
                f.write("\t".join((g, base[n] + ".scrubbed_kmers", base[n] + ".kmer_hits.gz")) + "\n")
        argv = (["-S", str(t / "S.txt"), "-A", "genomes_to_scrub.txt", "-B", "metagenomes_to_scrub.txt"] + c["kmer_scrub_count"] +
                ["--scrub", facts["min_fraction"], "--detect"] + facts["detect_args"] + [flag, "--coverage-spectrum", "--spectrum-max", "2"])
        p = subprocess.run([sk.cli_path()] + argv, cwd=str(b), capture_output=True, env=dict(os.environ, SK_SD_RESULT_BYTES="1"))
        assert p.returncode == 0, p.stderr.decode()[-800:]
        for n in base:
            assert hashlib.md5(open(base[n] + ".coverage_depth", "rb").read()).hexdigest() == c["strains"][n]["coverage_md5"], (flag, n)
        got[flag] = {n: open(base[n] + ".coverage_spectrum", "rb").read() for n in base}
        if flag == "--coverage-depth":
            for n in base:
                want = table_from_hits(gzip.open(base[n] + ".kmer_hits.gz", "rb").read(), base[n] + ".kmer_hits.gz", 2, 1)
                assert got[flag][n] == want and want.count(b"\n") > 3, n
                check_invariants(want, open(base[n] + ".coverage_depth", "rb").read())
        else:
            went = WENT.search(p.stderr)
            assert went and int(went.group(1)) >= 2
    assert got["--coverage-depth"] == got["--coverage-only"]
