"""The scrub sweep on the device (include/strainer_kmer.h has the rule): sk_filter_classes_joint / _above against numpy,
sk_covacc_set_classes / _finish_target_classes and sk_distinct_classes against the model (tests/_sweep_model.py), and the programs --
kmer_scrub_filter --min_fraction_list, strain_detect --coverage-scrub-sweep in the forms it runs in, coverage_depth --scrub-sweep --
against SEPARATE runs of the existing chain, one per fraction: kmer_scrub_filter -m f, then strain_detect --coverage-only.  Every
comparison is exact."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import strainer2_amd as sk
from _sweep_model import (above_classes, class_file, classes, informative, joint_classes, main_rows, numbers_by_class, parse_sweep,
                          sweep_table)
from strainer2_amd import native
from test_coverage_only_gpu import NAME, _canon
from test_coverage_regions_gpu import STRAIN_ORDER, _base, _run_sd, world  # noqa: F401  (world: the fixture)
from test_coverage_spectrum_gpu import SMALL_CHUNKS, job  # noqa: F401  (job: the fixture)

pytestmark = pytest.mark.gpu

FILTER = sk.cli_path("kmer_scrub_filter")
COV = sk.cli_path("coverage_depth")
FRACTIONS = ["0.4", "0.2", "0.05", "0.01"]        # (2 x f0 below what the drug scrub leaves)


@pytest.fixture(scope="module")
def ctx():
    c = sk.KmerContext(0)
    yield c
    c.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# step 2: the class bytes
# ---------------------------------------------------------------------------------------------------------------------------------
def _keys(kind, n, rng):
    if kind == "equal":
        return np.full(n, 7, dtype=np.int64), np.full(n, 3, dtype=np.int64)
    if kind == "two":
        return rng.integers(1, 3, n).astype(np.int64) * 5, np.zeros(n, dtype=np.int64)
    pan = rng.integers(0, 40, n).astype(np.int64)
    meta = rng.integers(0, 3000, n).astype(np.int64)
    meta[rng.random(n) < 0.3] = 0
    return pan, meta


def _lists(n_alive, F):
    """non-decreasing n_scrub lists of length F: 0, 1 and n among them, two equal neighbours, cuts spread between"""
    if F == 1:
        return [[0], [min(1, n_alive)], [n_alive], [n_alive // 2]]
    if F == 2:
        return [[0, n_alive], [min(1, n_alive)] * 2, [n_alive // 3, n_alive // 3], [0, min(1, n_alive)]]
    spread = sorted(int(x) for x in np.linspace(0, n_alive, 14))
    return [sorted([0, min(1, n_alive)] + spread), [n_alive] * 16, [0] * 16]


@pytest.mark.parametrize("F", [1, 2, 16])
@pytest.mark.parametrize("n", [0, 1, 255, 257, 4096, 4097, 70001])
def test_classes_joint_against_numpy(ctx, n, F):
    rng = np.random.default_rng(n * 31 + F)
    for kind in ("equal", "two", "random"):
        pan, meta = _keys(kind, n, rng)
        gone = (rng.random(n) < 0.1).astype(np.uint8)
        f = native.ScrubFilter(ctx)
        f.load(pan, meta, gone)
        n_alive = int((gone == 0).sum())
        for ns in _lists(n_alive, F):
            want, kept, ps, ms = joint_classes(pan, meta, gone, ns)
            got, gk = f.classes_joint(ps, ms, ns)
            assert np.array_equal(got, want), (kind, ns, int((got != want).sum()))
            assert np.array_equal(gk, kept) and not got[gone != 0].any()
            assert [int(k) for k in gk] == [n_alive - int(k) for k in ns]
        f.close()


def test_classes_joint_cuts_inside_a_tie_run_across_a_chunk_boundary(ctx):
    """rows 4000 .. 4199 share the top score (FLT_CHUNK = 4096 lies inside the run): cuts at 50, 96, 97, 150 rows of it go in row
    order; every third row of the run was gone before"""
    n = 9000
    rng = np.random.default_rng(5)
    pan = rng.integers(1, 50, n).astype(np.int64)
    meta = np.zeros(n, dtype=np.int64)
    pan[4000:4200] = 1000
    gone = np.zeros(n, dtype=np.uint8)
    gone[4000:4200:3] = 1
    f = native.ScrubFilter(ctx)
    f.load(pan, meta, gone)
    ns = [0, 50, 64, 65, 100, 133, 134, 134, 5000]
    want, kept, ps, ms = joint_classes(pan, meta, gone, ns)
    got, gk = f.classes_joint(ps, ms, ns)
    assert np.array_equal(got, want) and np.array_equal(gk, kept)
    run = got[4000:4200]
    assert len(set(run.tolist())) >= 6 and (np.diff(run[gone[4000:4200] == 0].astype(int)) >= 0).all()      # later rows of the run stay longer
    assert len(set(got[4090:4103].tolist())) >= 2            # a cut falls between rows on both sides of row 4096
    with pytest.raises(sk.SKError):
        f.classes_joint(ps, ms, [5, 4])                      # a smaller fraction scrubs at least as many rows
    with pytest.raises(sk.SKError):
        f.classes_joint(ps, ms, [0] * 17)
    with pytest.raises(sk.SKError):
        f.classes_joint(ps, ms, [n + 1])                     # more than take part
    f.close()


@pytest.mark.parametrize("F", [1, 2, 16])
@pytest.mark.parametrize("n", [0, 1, 255, 257, 4096, 4097, 70001])
def test_classes_above_against_numpy(ctx, n, F):
    rng = np.random.default_rng(n * 17 + F)
    for kind in ("equal", "two", "random"):
        pan, meta = _keys(kind, n, rng)
        gone = (rng.random(n) < 0.1).astype(np.uint8)
        f = native.ScrubFilter(ctx)
        f.load(pan, meta, gone)
        tp = sorted((int(x) for x in rng.integers(0, 45, F)), reverse=True)
        tm = sorted((int(x) for x in rng.integers(0, 3200, F)), reverse=True)
        for a, b in ((tp, tm), ([10 ** 9] * F, [10 ** 9] * F), ([0] * F, [0] * F)):
            want, kept = above_classes(pan, meta, gone, a, b)
            got, gk = f.classes_above(a, b)
            assert np.array_equal(got, want) and np.array_equal(gk, kept), (kind, a, b)
        if F > 1 and n:
            with pytest.raises(sk.SKError):
                f.classes_above([1] * (F - 1) + [2], [0] * F)   # thresholds do not increase along the list
        f.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# step 4: the counters by class
# ---------------------------------------------------------------------------------------------------------------------------------
NROWS = [0, 1, 255, 257, 70001]


def _feed(acc, member, depth):
    rows = np.repeat(np.arange(len(depth), dtype=np.uint32), depth)
    if len(rows):
        acc.add_rows(member, rows)


def _set(acc, member, cls, ncls):
    rows = np.flatnonzero(cls).astype(np.uint32)
    acc.set_classes(member, rows, cls[rows], ncls)


@pytest.mark.parametrize("layout", ["random", "one_class", "class_per_lane"])
@pytest.mark.parametrize("F", [1, 2, 16])
def test_finish_target_classes_against_the_model(ctx, F, layout):
    rng = np.random.default_rng(F * 7 + len(layout))
    with sk.CoverageAcc(ctx, NROWS, 0) as acc:
        depth, cls = [], []
        for m, n in enumerate(NROWS):
            d = rng.integers(0, 4, n).astype(np.uint32)
            d[rng.random(n) < 0.5] = 0
            if layout == "random":
                c = rng.integers(0, F + 1, n).astype(np.uint8)
                c[: min(n, F)] = np.arange(1, F + 1, dtype=np.uint8)[: min(n, F)]          # every class present
                d[c == 0] = 0                                                               # (class 0 rows are never hit in a run)
            elif layout == "one_class":
                c = np.full(n, F, dtype=np.uint8)
                d[:] = np.maximum(d, 1)
            else:
                c = (np.arange(n) % F + 1).astype(np.uint8)                                 # lane l of every wave: class l % F + 1
                d[:] = np.maximum(d, 1)
            depth.append(d)
            cls.append(c)
            _set(acc, m, c, F)
            _feed(acc, m, d)
        want = [numbers_by_class(d, c, F) for d, c in zip(depth, cls)]
        uq, tot, stray = acc.finish_target_classes()
        uq2, tot2, stray2 = acc.finish_target_classes()      # it changes nothing: a second call agrees
        assert np.array_equal(uq, uq2) and np.array_equal(tot, tot2) and stray == stray2 == 0
        for m in range(len(NROWS)):
            assert np.array_equal(uq[m], want[m][0]) and np.array_equal(tot[m], want[m][1]), (m, layout)
            assert np.array_equal(acc.rows(m), depth[m])     # the counters are as they were
        u, t = acc.finish_target()                           # ... and the sweep returns what it returns without the class pass
        assert [int(x) for x in u] == [int(np.count_nonzero(d)) for d in depth] and [int(x) for x in t] == [int(d.sum()) for d in depth]
        if F > 1 and layout != "one_class":
            assert int(uq[4][0]) > int(uq[4][F - 1]) > 0     # the numbers differ by fraction


def test_stray_rows_members_without_classes_and_bad_calls(ctx):
    with sk.CoverageAcc(ctx, [300, 300, 10], 0) as acc:
        with pytest.raises(sk.SKError):
            acc.finish_target_classes()                      # no member has classes
        c = np.zeros(300, dtype=np.uint8)
        c[:200] = np.arange(200) % 3 + 1
        _set(acc, 0, c, 3)
        d = np.zeros(300, dtype=np.uint32)
        d[[0, 1, 2, 5, 250, 299]] = [1, 2, 3, 4, 9, 1]       # rows 250 and 299 have class 0
        _feed(acc, 0, d)
        _feed(acc, 1, d)                                     # member 1 has no classes: its pairs are zero, its rows are not stray
        uq, tot, stray = acc.finish_target_classes()
        wu, wt, ws = numbers_by_class(d, c, 3)
        assert stray == ws == 2 and np.array_equal(uq[0], wu) and np.array_equal(tot[0], wt)
        assert not uq[1].any() and not tot[1].any() and not uq[2].any()
        with pytest.raises(sk.SKError):
            _set(acc, 1, c, 2)                               # classes 1..2 allowed: the class 3 rows are refused before a launch
        _set(acc, 1, np.minimum(c, 2), 2)
        uq, tot, stray = acc.finish_target_classes()
        w1u, w1t, _ = numbers_by_class(d, np.minimum(c, 2), 2)
        assert stray == 4 and [int(x) for x in uq[1]] == [int(w1u[0]), int(w1u[1]), 0] and [int(x) for x in tot[1]] == [int(w1t[0]), int(w1t[1]), 0]
        acc.set_classes(1, [], [], 0)                        # ... and off again
        uq, tot, stray = acc.finish_target_classes()
        assert stray == 2 and not uq[1].any()
        for rows, cl, ncls in (([300], [1], 3), ([0], [4], 3), ([0], [0], 3), ([0], [1], 17), ([0], [1], 0)):
            with pytest.raises(sk.SKError):
                acc.set_classes(0, rows, cl, ncls)
        with pytest.raises(sk.SKError):
            acc.set_classes(3, [0], [1], 1)
        uq3, tot3, stray3 = acc.finish_target_classes()      # the refused calls changed nothing
        assert np.array_equal(uq3, uq) and np.array_equal(tot3, tot) and stray3 == 2
        acc.finish_target()


def test_classes_over_a_real_fold(world):  # noqa: F811
    """the union of three strains folded from a launch, classes over the informative rows: the class pass against the counters"""
    w = world
    rng = np.random.default_rng(3)
    with sk.CoverageAcc(w.ctxs[0], w.nrows, 0) as acc:
        cls = []
        for m in range(3):
            c = np.where(w.typ[m] == 2, rng.integers(1, 5, w.nrows[m]), 0).astype(np.uint8)
            cls.append(c)
            _set(acc, m, c, 4)
        w.union.tally_launch(w.b1)
        w.union.tally_collect_counts()
        acc.add(w.union, 0, 1, w.b1.nrec)
        depth = [acc.rows(m).copy() for m in range(3)]
        uq, tot, stray = acc.finish_target_classes()
        assert stray == 0 and sum(int(d.sum()) for d in depth) > 0
        for m in range(3):
            wu, wt, _ = numbers_by_class(depth[m], cls[m], 4)
            assert np.array_equal(uq[m], wu) and np.array_equal(tot[m], wt)
        u, t = acc.finish_target()
        assert [int(x) for x in u] == [int(x) for x in uq[:, 0]] and [int(x) for x in t] == [int(x) for x in tot[:, 0]]


def test_distinct_classes_against_the_model(ctx):
    rng = np.random.default_rng(11)
    for n, ns, F in ((0, 3, 4), (1, 1, 1), (5000, 3, 16), (70001, 5, 2)):
        pool = rng.integers(0, 2 ** 62, max(n // 3, 1)).astype(np.uint64)
        pcls = rng.integers(1, F + 1, len(pool)).astype(np.uint8)
        pick = rng.integers(0, len(pool), n)
        keys, cls = pool[pick], pcls[pick]                   # duplicates of one (sample, key) pair carry one class
        sample = rng.integers(0, ns, n).astype(np.uint32)
        uq, tot = ctx.distinct_classes(keys, sample, cls, ns, F)
        for s in range(ns):
            for q in range(F):
                sel = (sample == s) & (cls >= q + 1)
                assert int(tot[s, q]) == int(sel.sum()) and int(uq[s, q]) == len(set(keys[sel].tolist())), (n, s, q)
    with pytest.raises(sk.SKError):
        ctx.distinct_classes([1], [0], [3], 1, 2)
    with pytest.raises(sk.SKError):
        ctx.distinct_classes([1], [0], [0], 1, 2)
    with pytest.raises(sk.SKError):
        ctx.distinct_classes([1], [1], [1], 1, 2)


# ---------------------------------------------------------------------------------------------------------------------------------
# the programs
# ---------------------------------------------------------------------------------------------------------------------------------
def _table(path, g, rng, drug=False):
    """a count table of the strain's canonical 31-mers in strain order: few distinct counts, so the scores tie heavily"""
    seen, rows = set(), []
    for i in range(len(g) - 30):
        k = _canon(g[i:i + 31])
        if k not in seen:
            seen.add(k)
            rows.append(k)
    with gzip.GzipFile(path, "wb", mtime=0) as f:
        f.write(b"#kmer\treference_count\tpangenome_count\tmetagenome_count\tdrug_count\n")
        for k in rows:
            f.write(k + b"\t1\t%d\t%d" % (rng.choice([0, 0, 1, 1, 2, 3]), rng.choice([0, 1, 2, 2, 5, 9, 40])) +
                    (b"\t%d\n" % (1 if rng.random() < 0.05 else 0) if drug else b"\n"))


def _filter(args, out_path=None):
    p = subprocess.run([FILTER] + args, capture_output=True)
    assert p.returncode == 0, p.stderr.decode()[-400:]
    if out_path:
        with open(out_path, "wb") as f:
            f.write(p.stdout)
    return p


class Sweep:
    pass


@pytest.fixture(scope="module")
def sweep(job):  # noqa: F811
    """per strain and mode: the count table, the informative list of every fraction from a run of its own, and the list and class
    file of one --min_fraction_list run"""
    import random
    rng = random.Random(99)
    v = Sweep()
    v.d = job.d / "sweep"
    v.d.mkdir()
    v.modes = {"joint": ([], False), "independent": (["--independent"], False), "drug": ([], True)}
    v.sets = {}
    for s, g in enumerate(job.strains):
        for mode, (flag, drug) in v.modes.items():
            if s != 1 and mode != "joint":
                continue
            t = str(v.d / f"s{s}.{mode}.counts.gz")
            _table(t, g, rng, drug)
            sets = []
            for f in FRACTIONS:
                p = _filter(["-s", t, "-m", f] + flag, str(v.d / f"s{s}.{mode}.inf_{f}"))
                sets.append(informative(p.stdout))
            one = _filter(["-s", t, "-m", FRACTIONS[0]] + flag)
            lst = str(v.d / f"s{s}.{mode}.inf")
            p = _filter(["-s", t, "--min_fraction_list", ",".join(FRACTIONS), "--classes_out", lst + ".classes"] + flag, lst)
            assert (p.stdout, p.stderr) == (one.stdout, one.stderr), (s, mode)      # the run is the run at f0, byte for byte
            assert open(lst + ".classes", "rb").read() == class_file(FRACTIONS, sets), (s, mode)
            v.sets[(s, mode)] = sets
    return v


def test_filter_program_class_file_is_the_separate_runs(sweep):
    sets = sweep.sets[(1, "joint")]
    assert len({len(x) for x in sets}) >= 3                  # at least three of the sets differ
    cl = classes(sets)
    assert set(cl.values()) == {1, 2, 3, 4}
    t = str(sweep.d / "s1.joint.counts.gz")
    gz = str(sweep.d / "c.classes.gz")
    _filter(["-s", t, "--min_fraction_list=" + ",".join(FRACTIONS), "--classes_out=" + gz])
    assert gzip.open(gz, "rb").read() == class_file(FRACTIONS, sets)
    lst = sweep.d / "list.txt"
    lst.write_text(t + "\n")
    p = _filter(["-l", str(lst), "--min_fraction_list", ",".join(FRACTIONS[:2]), "--classes_out", str(sweep.d / "l.classes")])
    assert informative(p.stdout) == sets[0]
    assert open(sweep.d / "l.classes", "rb").read() == class_file(FRACTIONS[:2], sets[:2])
    p = _filter(["-s", t, "--min_fraction_list", FRACTIONS[1], "--classes_out", str(sweep.d / "one.classes")])      # F = 1
    assert open(sweep.d / "one.classes", "rb").read() == class_file(FRACTIONS[1:2], sets[1:2])


def _sd(job, sweep, tag, mode, flags, strains=(1,), env=None, fraction=None, targets="T.txt"):  # noqa: F811
    """one run of strain_detect over the job's targets with the informative lists of `mode` (of one fraction's own run, or the sweep
    run's): {strain: {suffix: bytes}}, stats, stderr"""
    d = job.d / ("sw_" + tag)
    d.mkdir()
    inf = {s: str(sweep.d / (f"s{s}.{mode}.inf" + (f"_{fraction}" if fraction else ""))) for s in strains}
    if len(strains) > 1:
        (d / "S.txt").write_text("".join(f"{job.d}/s{s}.fa\t{inf[s]}\t{d}/{NAME % s}\n" for s in strains))
        argv = ["-S", str(d / "S.txt")]
    else:
        s = strains[0]
        argv = ["-r", str(job.d / f"s{s}.fa"), "-a", inf[s], "-o", str(d / (NAME % s))]
    rc, err, stats = _run_sd(argv + ["-B", str(job.d / targets)] + flags, dict(SMALL_CHUNKS, SK_SD_RESULT_BYTES="1", **(env or {})), d, "run")
    assert rc == 0, err.decode()[-600:]
    out = {}
    for s in strains:
        b = _base(d / (NAME % s))
        out[s] = {x: open(b + "." + x, "rb").read() for x in ("coverage_depth", "coverage_scrub_sweep", "coverage_spectrum", "coverage_regions",
                                                               "coverage_recurrence", "coverage_thresholds", "kmer_hits.gz")
                  if os.path.exists(b + "." + x)}
    return out, stats, err


@pytest.fixture(scope="module")
def separate(job, sweep):  # noqa: F811
    """the existing chain once per fraction, strain and mode: {(strain, mode): expected sweep table}"""
    want = {}
    tables = {k: [] for k in sweep.sets}
    for f in FRACTIONS:
        for mode in sweep.modes:                                 # strain 1: a run of its own per fraction and mode
            out, _, _ = _sd(job, sweep, f"sep_1_{mode}_{f}", mode, ["--coverage-only"], strains=(1,), fraction=f)
            tables[(1, mode)].append(out[1]["coverage_depth"])
        out, _, _ = _sd(job, sweep, f"sep_S_{f}", "joint", ["--coverage-only"], strains=(0, 2, 3), fraction=f)   # the others: one -S run per fraction
        for s in (0, 2, 3):
            tables[(s, "joint")].append(out[s]["coverage_depth"])
    for k, t in tables.items():
        want[k] = (sweep_table(FRACTIONS, t), t[0])
    return want


def test_the_sweep_is_the_separate_runs(job, sweep, separate):  # noqa: F811
    """THE DEFINING TEST: four fractions, four runs of kmer_scrub_filter -m f + strain_detect --coverage-only, one sweep run"""
    want, table0 = separate[(1, "joint")]
    out, stats, _ = _sd(job, sweep, "only", "joint", ["--coverage-only", "--coverage-scrub-sweep"])
    got = out[1]["coverage_scrub_sweep"]
    assert got == want
    assert out[1]["coverage_depth"] == table0                # everything else keeps the bytes of the run at f0
    assert stats[0] >= 1 and stats[1] >= 1                   # runs counted on the device, and runs replayed by the host
    rows = parse_sweep(got)
    _, main = main_rows(table0)
    assert list(rows) == list(main)
    for s, r in rows.items():
        assert [x[0] for x in r] == FRACTIONS and (r[0][1], r[0][2], r[0][3]) == main[s]
    assert len({r[1] for r in next(iter(rows.values()))}) >= 3                                  # at least three sets differ
    assert any(len({(x[2], x[3]) for x in r}) >= 2 for r in rows.values())                      # a sample's numbers differ by fraction
    off, _, _ = _sd(job, sweep, "only_off", "joint", ["--coverage-only"])
    assert off[1] == {k: v for k, v in out[1].items() if k != "coverage_scrub_sweep"}


def test_coverage_depth_form_and_the_hit_list(job, sweep, separate):  # noqa: F811
    want, table0 = separate[(1, "joint")]
    out, _, _ = _sd(job, sweep, "depth", "joint", ["--coverage-depth", "--coverage-scrub-sweep"])
    assert out[1]["coverage_scrub_sweep"] == want and out[1]["coverage_depth"] == table0
    off, _, _ = _sd(job, sweep, "depth_off", "joint", ["--coverage-depth"])
    assert off[1] == {k: v for k, v in out[1].items() if k != "coverage_scrub_sweep"}        # the hit list too
    hits = _base(job.d / "sw_depth" / (NAME % 1)) + ".kmer_hits.gz"
    cls = str(sweep.d / "s1.joint.inf.classes")
    p = subprocess.run([COV, "-k", hits, "--scrub-classes", cls, "--scrub-sweep"], capture_output=True)
    q = subprocess.run([COV, "-k", hits], capture_output=True)
    assert p.returncode == 0 and (p.stdout, p.stderr) == (q.stdout, q.stderr), p.stderr.decode()[-400:]
    assert open(_base(hits) + ".coverage_scrub_sweep", "rb").read() == want
    short = sweep.d / "short.classes"                        # a class file that lacks k-mers of the hit list
    short.write_bytes(b"#min_fractions\t0.5\n#post_scrub_kmers\t1\n" + sweep.sets[(1, "joint")][0][0] + b"\t1\n")
    before = sorted(os.listdir(job.d / "sw_depth"))
    p = subprocess.run([COV, "-k", hits, "--scrub-classes", str(short), "--scrub-sweep=" + str(job.d / "sw_depth" / "x.tsv")], capture_output=True)
    assert p.returncode != 0 and p.stdout == b"" and p.stderr.count(b"\n") == 1 and b"does not name" in p.stderr
    assert sorted(os.listdir(job.d / "sw_depth")) == before


@pytest.mark.parametrize("mode", ["independent", "drug"])
def test_independent_mode_and_a_drug_column(job, sweep, separate, mode):  # noqa: F811
    want, table0 = separate[(1, mode)]
    assert len({len(x) for x in sweep.sets[(1, mode)]}) >= 2
    out, _, _ = _sd(job, sweep, "mode_" + mode, mode, ["--coverage-only", "--coverage-scrub-sweep"])
    assert out[1]["coverage_scrub_sweep"] == want and out[1]["coverage_depth"] == table0


@pytest.mark.parametrize("form,env", [("union", {}), ("two_unions", {"SK_SD_GROUP": "2"}), ("two_devices", {"SK_DEVICES": "0,0", "SK_SD_GROUP": "2"})])
@pytest.mark.parametrize("table", ["--coverage-only", "--coverage-depth"])
def test_many_strains(job, sweep, separate, table, form, env):  # noqa: F811
    out, _, _ = _sd(job, sweep, f"S_{form}{table}", "joint", [table, "--coverage-scrub-sweep"], strains=(0, 1, 2, 3), env=env)
    for s in range(4):
        want, table0 = separate[(s, "joint")]
        assert out[s]["coverage_scrub_sweep"] == want and out[s]["coverage_depth"] == table0, s


def test_next_to_the_other_tables_and_the_target_cache(job, sweep, separate):  # noqa: F811
    want, table0 = separate[(1, "joint")]
    others = ["--coverage-regions", "--region-window", "500", "--coverage-spectrum", "--coverage-recurrence", "--coverage-thresholds"]
    ref, _, _ = _sd(job, sweep, "others_off", "joint", ["--coverage-only"] + others)
    out, _, _ = _sd(job, sweep, "others_on", "joint", ["--coverage-only", "--coverage-scrub-sweep"] + others)
    assert out[1].pop("coverage_scrub_sweep") == want and out[1] == ref[1] and len(ref[1]) == 5
    cache = str(job.d / "sw_cache")
    os.mkdir(cache)
    for tag in ("fill", "served"):
        out, _, _ = _sd(job, sweep, "cache_" + tag, "joint", ["--coverage-only", "--coverage-scrub-sweep", "--target-cache", cache])
        assert out[1]["coverage_scrub_sweep"] == want and out[1]["coverage_depth"] == table0
    assert os.listdir(cache)


def test_a_class_file_that_does_not_fit_the_list_is_refused(job, sweep):  # noqa: F811
    d = job.d / "sw_bad"
    d.mkdir()
    inf = str(sweep.d / "s1.joint.inf")
    good = open(inf + ".classes", "rb").read().split(b"\n")
    cases = {"missing": None, "no_header": b"\n".join(good[2:]), "class_0": b"\n".join(good[:2] + [good[2].split(b"\t")[0] + b"\t0"] + good[3:]),
             "class_5": b"\n".join(good[:2] + [good[2].split(b"\t")[0] + b"\t5"] + good[3:]), "one_less": b"\n".join(good[:-2]) + b"\n",
             "swapped": b"\n".join(good[:2] + [good[3], good[2]] + good[4:]), "twice": b"\n".join(good[:3] + [good[2]] + good[4:])}
    for name, text in cases.items():
        cf = d / (name + ".classes")
        if text is not None:
            cf.write_bytes(text)
        before = sorted(os.listdir(d))
        argv = ["-r", str(job.d / "s1.fa"), "-a", inf, "-o", str(d / (NAME % 1)), "-B", str(job.d / "T.txt"), "--coverage-only",
                "--coverage-scrub-sweep", "--scrub-classes", str(cf)]
        rc, err, _ = _run_sd(argv, {}, job.d, "bad_" + name)
        assert rc != 0 and err.count(b"\n") == 1 and b"class file" in err, (name, err)
        assert sorted(os.listdir(d)) == before, name


# ---------------------------------------------------------------------------------------------------------------------------------
# fused: kmer_scrub_count ... --scrub f0,f1,... --detect ... --coverage-scrub-sweep
# ---------------------------------------------------------------------------------------------------------------------------------
def _scrub_lists(job, d):  # noqa: F811
    (d / "A.txt").write_text("".join(f"{job.d}/s{s}.fa\n" for s in (0, 3)))
    (d / "B.txt").write_text(f"{job.d}/se.fq.gz\n{job.d}/pe_1.fa\n")
    return ["-A", str(d / "A.txt"), "-B", str(d / "B.txt")]


def _chain(job, d, s, table, lists):  # noqa: F811
    """the separate programs over a count table of strain s: kmer_scrub_filter with the list (informative list + class file), then
    strain_detect with them: (class file, sweep table, coverage table)"""
    inf = str(d / f"chain{s}.inf")
    _filter(["-s", table, "--min_fraction_list", ",".join(FRACTIONS), "--classes_out", inf + ".classes"], inf)
    out = d / f"chain{s}"
    out.mkdir()
    rc, err, _ = _run_sd(["-r", str(job.d / f"s{s}.fa"), "-a", inf, "-o", str(out / (NAME % s)), "-B", str(job.d / "T.txt"), "--coverage-only",
                          "--coverage-scrub-sweep"], dict(SMALL_CHUNKS), d, f"chain{s}")
    assert rc == 0, err.decode()[-500:]
    b = _base(out / (NAME % s))
    return open(inf + ".classes", "rb").read(), open(b + ".coverage_scrub_sweep", "rb").read(), open(b + ".coverage_depth", "rb").read(), open(inf, "rb").read()


def test_fused_single_strain(job):  # noqa: F811
    d = job.d / "sw_fused_r"
    d.mkdir()
    lists = _scrub_lists(job, d)
    p = subprocess.run([sk.cli_path(), "-r", str(job.d / "s1.fa")] + lists, capture_output=True)
    assert p.returncode == 0, p.stderr.decode()[-400:]
    (d / "t1.txt").write_bytes(p.stdout)
    want_cls, want_sweep, want_cov, want_inf = _chain(job, d, 1, str(d / "t1.txt"), lists)
    hits = str(d / (NAME % 1))
    argv = ["-r", str(job.d / "s1.fa")] + lists + ["--scrub", ",".join(FRACTIONS), "--scrub-out", str(d / "f.inf"), "--detect", "-B", str(job.d / "T.txt"),
                                                  "-o", hits, "--coverage-only", "--coverage-scrub-sweep"]
    p = subprocess.run([sk.cli_path()] + argv, capture_output=True, env=dict(os.environ, **SMALL_CHUNKS))
    assert p.returncode == 0, p.stderr.decode()[-600:]
    assert open(d / "f.inf", "rb").read() == want_inf and open(d / "f.inf.classes", "rb").read() == want_cls
    assert open(_base(hits) + ".coverage_scrub_sweep", "rb").read() == want_sweep and open(_base(hits) + ".coverage_depth", "rb").read() == want_cov
    assert len({r[1] for r in next(iter(parse_sweep(want_sweep).values()))}) >= 3
    # a single value is today's run: no class file
    (d / "g").mkdir()
    one = subprocess.run([sk.cli_path(), "-r", str(job.d / "s1.fa")] + lists + ["--scrub", FRACTIONS[0], "--scrub-out", str(d / "g.inf"), "--detect", "-B",
                         str(job.d / "T.txt"), "-o", str(d / "g" / (NAME % 1)), "--coverage-only"], capture_output=True, env=dict(os.environ, **SMALL_CHUNKS))
    assert one.returncode == 0 and open(d / "g.inf", "rb").read() == want_inf and not os.path.exists(d / "g.inf.classes")
    assert open(_base(d / "g" / (NAME % 1)) + ".coverage_depth", "rb").read() == want_cov


def test_fused_many_strains(job):  # noqa: F811
    d = job.d / "sw_fused_S"
    d.mkdir()
    lists = _scrub_lists(job, d)
    (d / "S1.txt").write_text("".join(f"{job.d}/s{s}.fa\t{d}/t{s}.txt\n" for s in (1, 2)))
    p = subprocess.run([sk.cli_path(), "-S", str(d / "S1.txt")] + lists, capture_output=True)
    assert p.returncode == 0, p.stderr.decode()[-400:]
    want = {s: _chain(job, d, s, str(d / f"t{s}.txt"), lists) for s in (1, 2)}
    (d / "S3.txt").write_text("".join(f"{job.d}/s{s}.fa\t{d}/f{s}.inf\t{d}/{NAME % s}\n" for s in (1, 2)))
    p = subprocess.run([sk.cli_path(), "-S", str(d / "S3.txt")] + lists + ["--scrub", ",".join(FRACTIONS), "--detect", "-B", str(job.d / "T.txt"),
                        "--coverage-only", "--coverage-scrub-sweep"], capture_output=True, env=dict(os.environ, **SMALL_CHUNKS))
    assert p.returncode == 0, p.stderr.decode()[-600:]
    for s in (1, 2):
        cls, sweep_t, cov, inf = want[s]
        assert open(d / f"f{s}.inf", "rb").read() == inf and open(d / f"f{s}.inf.classes", "rb").read() == cls, s
        b = _base(d / (NAME % s))
        assert open(b + ".coverage_scrub_sweep", "rb").read() == sweep_t and open(b + ".coverage_depth", "rb").read() == cov, s
