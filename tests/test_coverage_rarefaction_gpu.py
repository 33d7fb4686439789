"""Rarefaction on the device (include/strainer_kmer.h has the rule): the classifying pass, the pair counts, the replayed rows' entry
and the finishing pass (sk_covacc_set_rarefaction / sk_covacc_set_pair_base / sk_covacc_add / sk_covacc_add_rows_hits_pairs /
sk_covacc_add_pairs / sk_covacc_finish_target_rarefaction), all against tests/_rarefaction_model.py.

Library level: accumulators are built from row counts alone and fed through add_rows_hits_pairs; members of 0, 1, 255, 257 and 70 001
rows sit in one accumulator (70 001 rows are more than 256 workgroups x 256 threads, so the grid-stride loops turn more than once).
The world and its premises are tests/_rarefaction_model.py's (tests/test_coverage_rarefaction_host.py checks the premises without a
device).  Real launches run in the world of test_coverage_regions_gpu.py; their lines come from what the existing collect calls return,
so the expected numbers owe nothing to the code under test."""
import numpy as np
import pytest

import _rarefaction_model as rm
import _support_model as sm
import strainer2_amd as sk
from test_coverage_only_gpu import ROW_BITS, _pair, model
from test_coverage_regions_gpu import world  # noqa: F401  (world: the fixture)

pytestmark = pytest.mark.gpu

SK_E_ARG, SK_E_STATE = -3, -7
EDGE = rm.EDGE


@pytest.fixture(scope="module")
def ctx():
    with sk.KmerContext(0) as c:
        yield c


def _want(entries, ranges, T, seed, min_hits):
    ords = rm.world_ordinals(ranges)
    out = []
    for rows, totals, o in entries:
        out.append(rm.table(np.stack([o, rows.astype(np.uint64), totals.astype(np.uint64)], axis=1), T, seed, min_hits, ords))
    return out


def _feed(acc, entries, ranges):
    for m, (rows, totals, o) in enumerate(entries):
        if len(rows):
            acc.add_rows_hits_pairs(m, rows, totals, o)
    for first, n in ranges:
        acc.add_pairs(first, n)


def _finish_and_check(acc, want):
    pairs, uq, tot = acc.finish_target_rarefaction()
    for m, (wp, wu, wt) in enumerate(want):
        assert pairs.tolist() == wp
        assert uq[m].tolist() == wu and tot[m].tolist() == wt, ("member", m)
    again = acc.finish_target_rarefaction()                    # the rarefaction state is zero afterwards
    assert not any(x.any() for x in again)
    return pairs, uq, tot


@pytest.mark.parametrize("seed", rm.SEEDS)
@pytest.mark.parametrize("which", range(len(rm.LISTS)), ids=lambda i: "list%d" % len(rm.LISTS[i].split(",")))
def test_members_of_every_size_ordinals_around_the_32_bit_edge(ctx, which, seed):
    T, _ = rm.parse_list(rm.LISTS[which])
    entries, ranges = rm.library_world(which)
    want = _want(entries, ranges, T, seed, rm.MIN_HITS)
    with sk.CoverageAcc(ctx, rm.SIZES, rm.MIN_HITS) as acc:
        plain = None
        for on in (False, True):                               # sk_covacc_finish_target's numbers are unchanged by the flag
            if on:
                acc.set_rarefaction(T, seed)
                _feed(acc, entries, ranges)
                pairs, uq, tot = _finish_and_check(acc, want)
                assert int(pairs[0]) > 0 and int(tot[4, 0]) > int(uq[4, 0]) > 0
            else:
                for m, (rows, totals, _) in enumerate(entries):
                    if len(rows):
                        acc.add_rows_hits(m, rows, totals)
            d = acc.finish_target()
            if plain is None:
                plain = d
            assert np.array_equal(plain[0], d[0]) and np.array_equal(plain[1], d[1])
        for m, (rows, totals, _) in enumerate(entries):
            ok = totals.astype(np.int64) > rm.MIN_HITS
            assert (int(plain[0][m]), int(plain[1][m])) == (len(np.unique(rows[ok])), int(ok.sum()))
        if T[0] == EDGE:                                       # f0 = 1: the main table's numbers, and every pair
            assert uq[:, 0].tolist() == plain[0].tolist() and tot[:, 0].tolist() == plain[1].tolist()
            assert int(pairs[0]) == sum(n for _, n in ranges)


def test_one_row_three_pairs_and_the_last_row_alone(ctx):
    T, seed = rm.parse_list("1,0.5,0.25")[0], 7
    by = {}
    for i in list(range(200)) + [EDGE - 1, EDGE, EDGE + 1]:    # a pair of every class, the 32-bit edge's among them
        by.setdefault(rm.klass(i, T, seed), []).append(i)
    assert sorted(by) == [1, 2, 3]
    o = [by[1][-1], by[2][-1], by[3][-1]]
    with sk.CoverageAcc(ctx, rm.SIZES, 1) as acc:
        acc.set_rarefaction(T, seed)
        acc.add_rows_hits_pairs(3, [200, 200, 200], [5, 5, 1], o)     # the class-3 pair's line does not pass min_kmer_hits = 1
        acc.add_rows_hits_pairs(4, [70000], [2], [o[2]])
        acc.add_pairs(o[2], 1)
        pairs, uq, tot = acc.finish_target_rarefaction()
        assert pairs.tolist() == [1, 1, 1]
        assert uq[3].tolist() == [1, 1, 0] and tot[3].tolist() == [2, 1, 0]
        assert uq[4].tolist() == [1, 1, 1] and tot[4].tolist() == [1, 1, 1]
        assert not uq[:3].any() and not tot[:3].any()
        assert [x.tolist() for x in acc.finish_target()] == [[0, 0, 0, 1, 1], [0, 0, 0, 2, 1]]


def test_300000_lines_on_one_row_over_all_classes(ctx):
    T, _ = rm.parse_list(rm.LISTS[3])
    o = np.arange(300000, dtype=np.uint64) + np.uint64(EDGE - 150000)
    totals = np.full(300000, 9, dtype=np.uint32)
    want = rm.table(np.stack([o, np.full(300000, 100, dtype=np.uint64), totals.astype(np.uint64)], axis=1), T, 3, 0, o)
    assert want[2][0] == 300000 and all(a > b > 0 for a, b in zip(want[2], want[2][1:]))
    with sk.CoverageAcc(ctx, rm.SIZES, 0) as acc:
        acc.set_rarefaction(T, 3)
        acc.add_rows_hits_pairs(3, np.full(300000, 100, dtype=np.uint32), totals, o)
        acc.add_rows_hits_pairs(4, np.full(300000, 70000, dtype=np.uint32), totals, o[::-1].copy())
        acc.add_pairs(int(o[0]), 300000)
        pairs, uq, tot = acc.finish_target_rarefaction()
        assert pairs.tolist() == want[0] == want[2]
        assert tot[3].tolist() == want[2] == tot[4].tolist() and uq[3].tolist() == [1] * 16 == uq[4].tolist()
        acc.finish_target()


def test_set_rarefaction_discards_and_bad_calls(ctx):
    with sk.CoverageAcc(ctx, [10, 300], 2) as acc:
        for call in (acc.finish_target_rarefaction, lambda: acc.add_pairs(0, 3),
                     lambda: acc.add_rows_hits_pairs(0, [1], [9], [0])):
            with pytest.raises(sk.SKError) as e:
                call()                                         # off after create
            assert e.value.code == SK_E_STATE
        acc.set_pair_base(EDGE - 3)                            # (the base is kept whether rarefaction is on or not)
        for bad in ([EDGE, EDGE], [1 << 31, EDGE], [EDGE + 1], [5, 4, 4], list(range(17, 0, -1)), [9, 5, 7]):
            with pytest.raises(sk.SKError) as e:
                acc.set_rarefaction(bad)
            assert e.value.code == SK_E_ARG, bad
        acc.set_rarefaction(list(range(16, 0, -1)))
        acc.set_rarefaction([EDGE])
        acc.add_rows_hits_pairs(0, [9, 9, 1], [3, 4, 2], [0, 1, 2])
        acc.add_pairs(0, 3)
        acc.set_rarefaction([EDGE, 0])                         # between targets: what was classified is gone, the depth counters stay
        acc.add_rows_hits_pairs(1, [0, 0], [3, 2], [EDGE, EDGE])
        acc.add_pairs(EDGE, 1)
        pairs, uq, tot = acc.finish_target_rarefaction()
        assert pairs.tolist() == [1, 0] and uq.tolist() == [[0, 0], [1, 0]] and tot.tolist() == [[0, 0], [1, 0]]
        assert [x.tolist() for x in acc.finish_target()] == [[1, 1], [2, 1]]
        with pytest.raises(sk.SKError) as e:
            acc.add_rows_hits_pairs(1, [300], [3], [0])        # a row the member does not have
        assert e.value.code == SK_E_ARG
        acc.set_rarefaction([])
        with pytest.raises(sk.SKError):
            acc.finish_target_rarefaction()


# ---------------------------------------------------------------------------------------------------------------------------------
# real launches (the world of test_coverage_regions_gpu.py)
# ---------------------------------------------------------------------------------------------------------------------------------
T_REAL = "1,0.6,0.3,0.12,0.05"
T_SINGLE = "1,0.5,0.2"                                        # one strain's lines are fewer: a list that keeps the premises


BASES = [0, EDGE - 3]


def _lines(ns, is_union, sides, npairs):
    """sides: (recs, hits, starts, r0, step) per mate -> per member the hit lines (pair of the run, row, the pair's total)"""
    tot = np.zeros((npairs, ns), dtype=np.int64)
    for recs, _, _, r0, step in sides:
        for key, al, _ in recs.tolist():
            j = _pair(key // ns, r0, step, npairs)
            if j is not None:
                tot[j, key % ns] += al
    out = [[] for _ in range(ns)]
    for _, hits, starts, r0, step in sides:
        rec_of = np.searchsorted(starts, hits[:, 0], side="right") - 1
        for (pos, row), rec in zip(hits.tolist(), rec_of.tolist()):
            m, row = (row >> ROW_BITS, row & ((1 << ROW_BITS) - 1)) if is_union else (0, row)
            j = _pair(rec, r0, step, npairs)
            if j is not None:
                out[m].append((j, row, int(tot[j, m])))
    return out


def _check_real(acc, nrows, ns, is_union, sides, npairs, primary, base, T, seed):
    """the rarefaction table against the model, its premises on the model alone, then the main counters"""
    pairs, uq, tot = acc.finish_target_rarefaction()
    ords = np.arange(npairs, dtype=np.uint64) + np.uint64(base)
    lines = _lines(ns, is_union, sides, npairs)
    sums = np.zeros(len(T), dtype=np.int64)
    for m in range(ns):
        wp, wu, wt = rm.table([(base + j, row, t) for j, row, t in lines[m]], T, seed, primary, ords)
        assert pairs.tolist() == wp
        assert uq[m].tolist() == wu and tot[m].tolist() == wt, ("member", m)
        sums += np.array(wu)
    if primary < 1000:                                         # premises: every subsample counts a line, adjacent ones differ
        assert sums[-1] > 0 and all(a > b for a, b in zip(sums, sums[1:])), sums
    want = model(nrows, ns, is_union, sides, npairs, primary)
    d = acc.finish_target()
    assert d[0].tolist() == [int(np.count_nonzero(x)) for x in want] and d[1].tolist() == [int(x.sum()) for x in want]
    assert uq[:, 0].tolist() == d[0].tolist() and tot[:, 0].tolist() == d[1].tolist() and int(pairs[0]) == npairs     # f0 = 1
    assert not any(x.any() for x in acc.finish_target_rarefaction())


@pytest.mark.parametrize("base", BASES)
@pytest.mark.parametrize("primary", [0, 5, 1000])
def test_union_of_three(world, primary, base):  # noqa: F811
    w, u = world, world.union
    T, _ = rm.parse_list(T_REAL)
    r1, h1 = w.uni[0]
    with sk.CoverageAcc(w.ctxs[0], w.nrows, primary) as acc:
        acc.set_rarefaction(T, 11)
        u.tally_launch(w.b1, results_stay=True)
        u.tally_collect_counts()
        acc.set_pair_base(base)
        acc.add(u, 0, 1, w.b1.nrec)
        _check_real(acc, w.nrows, 3, True, [(r1, h1, w.st1, 0, 1)], w.b1.nrec, primary, base, T, 11)


@pytest.mark.parametrize("base", BASES)
def test_single_reads_interleaved_pairs_and_pairs_over_two_batches(world, base):  # noqa: F811
    w, primary = world, 5
    T, _ = rm.parse_list(T_SINGLE)
    (r1, h1), (r2, h2) = w.single
    c = w.ctxs[1]
    np_ = w.b1.nrec // 2
    with sk.CoverageAcc(c, [w.nrows[1]], primary) as acc:
        acc.set_rarefaction(T, 0)
        acc.set_pair_base(base)                                # (kept from one add to the next)
        c.tally_launch(w.b1)
        c.tally_collect_counts()
        acc.add(c, 0, 1, w.b1.nrec)
        _check_real(acc, [w.nrows[1]], 1, False, [(r1, h1, w.st1, 0, 1)], w.b1.nrec, primary, base, T, 0)
        c.tally_launch(w.b1)
        c.tally_collect_counts()
        acc.add(c, 0, 2, np_, mate=("same", 1, 2))             # interleaved pairs from record 0 ...
        _check_real(acc, [w.nrows[1]], 1, False, [(r1, h1, w.st1, 0, 2), (r1, h1, w.st1, 1, 2)], np_, primary, base, T, 0)
        c.tally_launch(w.b1)
        c.tally_collect_counts()
        acc.add(c, 1, 2, np_ - 1, mate=("same", 2, 2))         # ... and from record 1
        _check_real(acc, [w.nrows[1]], 1, False, [(r1, h1, w.st1, 1, 2), (r1, h1, w.st1, 2, 2)], np_ - 1, primary, base, T, 0)
        c.tally_launch(w.b1)
        c.tally_collect_counts()
        acc.hold(c)
        c.tally_launch(w.b2)
        c.tally_collect_counts()
        acc.add(c, 4, 1, w.b1.nrec - 4, mate=("held", 2, 1))   # held mates
        _check_real(acc, [w.nrows[1]], 1, False, [(r2, h2, w.st2, 4, 1), (r1, h1, w.st1, 2, 1)], w.b1.nrec - 4, primary, base, T, 0)


def test_two_runs_of_one_target_and_a_replayed_run_between_them(world):  # noqa: F811
    """a target of three runs: pairs 0 .. n - 1 folded, then 5 replayed pairs, then a folded run again: every pair counted once"""
    w, c, primary = world, world.ctxs[1], 1
    T, _ = rm.parse_list("0.8,0.4")                            # a list without 1
    (r1, h1), (r2, h2) = w.single
    n1, base = w.b1.nrec, EDGE - 400
    lines = [(base + j, row, t) for j, row, t in _lines(1, False, [(r1, h1, w.st1, 0, 1)], n1)[0]]
    replay = [(base + n1 + k, (37 * k) % w.nrows[1], k) for k in range(5)]
    lines += replay
    lines += [(base + n1 + 5 + j, row, t) for j, row, t in _lines(1, False, [(r2, h2, w.st2, 0, 1)], n1)[0]]
    with sk.CoverageAcc(c, [w.nrows[1]], primary) as acc:
        acc.set_rarefaction(T, 5)
        c.tally_launch(w.b1)
        c.tally_collect_counts()
        acc.set_pair_base(base)
        acc.add(c, 0, 1, n1)
        acc.add_rows_hits_pairs(0, [r for _, r, _ in replay], [t for _, _, t in replay], [o for o, _, _ in replay])
        acc.add_pairs(base + n1, 5)
        c.tally_launch(w.b2)
        c.tally_collect_counts()
        acc.set_pair_base(base + n1 + 5)
        acc.add(c, 0, 1, n1)
        pairs, uq, tot = acc.finish_target_rarefaction()
        wp, wu, wt = rm.table(lines, T, 5, primary, np.arange(2 * n1 + 5, dtype=np.uint64) + np.uint64(base))
        assert (pairs.tolist(), uq[0].tolist(), tot[0].tolist()) == (wp, wu, wt)
        assert 0 < wp[1] < wp[0] < 2 * n1 + 5 and 0 < wu[1] < wu[0]
        acc.finish_target()


@pytest.mark.parametrize("is_union", [True, False], ids=["union", "single"])
def test_beside_thresholds_and_support_all_three_tables_equal_their_models(world, is_union):  # noqa: F811
    w, primary, base = world, 5, EDGE - 3
    T, _ = rm.parse_list(T_REAL if is_union else T_SINGLE)
    lst = [0, 3, 10, 100]
    src = w.union if is_union else w.ctxs[1]
    ns = 3 if is_union else 1
    nrows = w.nrows if is_union else [w.nrows[1]]
    (r1, h1), (r2, h2) = w.uni if is_union else w.single
    sides = [(r2, h2, w.st2, 4, 1), (r1, h1, w.st1, 2, 1)]
    npairs = w.b1.nrec - 4
    got = {}
    for rar in (False, True):
        with sk.CoverageAcc(w.ctxs[0] if is_union else src, nrows, primary) as acc:
            acc.set_thresholds(lst)
            acc.set_support(True)
            if rar:
                acc.set_rarefaction(T, 2)
                acc.set_pair_base(base)
            for i, b in enumerate((w.b1, w.b2)):
                if is_union:
                    src.tally_launch(b, results_stay=True)
                else:
                    src.tally_launch(b)
                src.tally_collect_counts()
                if i == 0:
                    acc.hold(src)
            acc.add(src, 4, 1, npairs, mate=("held", 2, 1))
            thr = acc.finish_target_thresholds()
            sup = acc.finish_target_support()
            if rar:
                _check_real(acc, nrows, ns, is_union, sides, npairs, primary, base, T, 2)
            else:
                acc.finish_target()
            got[rar] = (thr, sup)
    for rar in (False, True):
        thr, sup = got[rar]
        for q, t in enumerate(lst):
            want = model(nrows, ns, is_union, sides, npairs, t)
            assert thr[0][:, q].tolist() == [int(np.count_nonzero(d)) for d in want], t
            assert thr[1][:, q].tolist() == [int(d.sum()) for d in want], t
        em = sm.from_records(0, ns, [(r2, 4, 1), (r1, 2, 1)], npairs)
        S = sm.tables([(0, j, s, L, parts, tot, None) for _, j, s, L, parts, tot, _ in em], 1, ns, primary, group=ns)
        assert sup[0].tolist() == S.pairs[0].tolist() and sup[1].tolist() == S.lines[0].tolist() and sup[2].tolist() == S.both[0].tolist()
        assert np.array_equal(sup[3], S.shared[0]) and np.array_equal(sup[4], S.lines_a[0]) and int(sup[0].sum()) > 0


# ---------------------------------------------------------------------------------------------------------------------------------
# the programs: every row against a plain --coverage-only run of the same binary on the subsample's file
# ---------------------------------------------------------------------------------------------------------------------------------
import gzip  # noqa: E402
import os  # noqa: E402
import random  # noqa: E402
import re  # noqa: E402

import _synth  # noqa: E402
from _thresholds_model import main_table  # noqa: E402
from test_coverage_only_gpu import NAME, WENT, _fa, job  # noqa: E402,F401  (job: the fixture)
from test_coverage_regions_gpu import _base, _run_sd  # noqa: E402

P_LIST, P_SEED = "1,0.5,0.2", 3
TINY = {"SK_SD_CHUNK_BYTES": "600", "SK_SD_RESULT_BYTES": "1"}       # chunks of about six reads: a target spans a hundred of them


def _targets(job):  # noqa: F811
    """Targets that force the replay between chunks the device counts.  A record shorter than k, and a read whose mate is missing,
    re-use what the record before them left (the reference's read loop), and in a subsample's file that is another record; so
    that the table's definition -- a rerun on the subsample's file -- holds exactly, the short record stands among records that hit no
    strain (nothing is carried into it in any subsample) and the unpaired last record hits no strain (it prints no line whatever its
    mate's stale tallies are).  Every other record has k bases or more."""
    rng, r = random.Random(77), job.reads
    junk = lambda n, ln=None: [_synth.rand_dna(rng, ln or rng.choice([31, 60, 100, 150])) for _ in range(n)]  # noqa: E731
    hits = [job.hit, _synth.revcomp(job.hit), job.hit[3:97], job.hit[10:100]]
    body = r(600, 51)
    for i in range(5, 600, 7):
        body[i] = hits[i % 4]
    same = [x[:100].ljust(100, b"A") for x in r(500, 53)]      # reads of one length: the two files' chunks line up
    for i in range(3, 500, 5):
        same[i] = hits[i % 4][:100].ljust(100, b"C")
    return {
        "pei_short_read_and_missing_last_mate": ("PEI", [junk(61) + [b"ACGTACGTAC"] + junk(60) + body + junk(1)]),       # 723 records
        "se_short_read": ("SE", [junk(45) + [b"ACGT"] + junk(45) + body]),
        "pe_lined_up": ("PE", [junk(40, 100) + same, junk(40, 100) + [_synth.revcomp(x) for x in same]]),
        "pe_not_lined_up": ("PE", [junk(37) + [b"ACGTACGTACGT"] + junk(37) + body[:500], junk(75) + r(500, 54)]),
    }


def _rtable(path, named=False):
    """-> {metagenome: [(fraction text, pairs, unique, total)]}; with `named` {(strain, metagenome): ...}"""
    lines = open(path, "rb").read().split(b"\n")
    assert lines[0] + b"\n" == (b"strain_name\t" if named else b"") + rm.HEADER and lines[-1] == b""
    out = {}
    for ln in lines[1:-1]:
        f = ln.split(b"\t")
        key = (f[0], f[1]) if named else f[0]
        f = f[1:] if named else f
        out.setdefault(key, []).append((f[1].decode(), int(f[2]), int(f[3]), int(f[4])))
    return out


def _argv(job, d, tag, mode, paths, strain=1):  # noqa: F811
    (d / tag).mkdir(exist_ok=True)
    return ["-r", str(job.d / f"s{strain}.fa"), "-a", str(job.d / f"s{strain}.inf.gz"), "-b", str(paths[0]), "-t", mode] + \
           (["-c", str(paths[1])] if mode == "PE" else []) + ["-o", str(d / tag / (NAME % strain))]


def _write(d, stem, files, gz=False):
    paths = []
    for i, recs in enumerate(files):
        paths.append(d / (f"{stem}_{i}.fa" + (".gz" if gz else "")))
        data = _fa(recs)
        paths[-1].write_bytes(gzip.compress(data, 1) if gz else data)
    return paths


def _reruns(job, d, mode, files, T, strain=1):  # noqa: F811
    """the expected rows: per q the subsample's file(s), a plain --coverage-only run on them, its pair count and two numbers"""
    want = []
    for q, t in enumerate(T):
        sub = rm.subsample(files, mode, t, P_SEED)
        paths = _write(d, f"sub{q}", sub)
        tag = f"rerun{q}_s{strain}"
        rc, err, _ = _run_sd(_argv(job, d, tag, mode, paths, strain) + ["--coverage-only"], {}, d, tag)
        assert rc == 0, err.decode()[-600:]
        tab = main_table(open(_base(d / tag / (NAME % strain)) + ".coverage_depth", "rb").read())
        u, tot = tab.get(paths[0].name.encode(), (0, 0))
        want.append((rm.npairs(sub, mode), u, tot))
    return want


@pytest.mark.parametrize("case", ["pei_short_read_and_missing_last_mate", "se_short_read", "pe_lined_up", "pe_not_lined_up"])
def test_program_rows_equal_reruns_on_the_subsamples_files(job, case):  # noqa: F811
    mode, files = _targets(job)[case]
    d = job.d / ("rar_" + case)
    d.mkdir()
    paths = _write(d, "in", files)
    T, fields = rm.parse_list(P_LIST)
    want = _reruns(job, d, mode, files, T)
    assert want[0][0] == rm.npairs(files, mode) > want[1][0] > want[2][0] > 0
    assert want[0][1] > want[1][1] > want[2][1] > 0 and want[2][2] > 0      # premises: the subsamples differ, the smallest counts a line
    outs = {}
    for tag, flags in (("only_on", ["--coverage-only", "--coverage-rarefaction"]), ("only_off", ["--coverage-only"]),
                       ("depth_on", ["--coverage-depth", "--coverage-rarefaction"]), ("depth_off", ["--coverage-depth"])):
        extra = ["--rarefaction-list", P_LIST, "--rarefaction-seed", str(P_SEED)] if tag.endswith("_on") else []
        rc, err, stats = _run_sd(_argv(job, d, tag, mode, paths) + flags + extra, dict(TINY, SK_SD_CO_FLUSH_ROWS="1"), d, tag)
        assert rc == 0, err.decode()[-600:]
        b = _base(d / tag / (NAME % 1))
        outs[tag] = (err, open(d / (tag + ".out"), "rb").read(), open(b + ".coverage_depth", "rb").read(),
                     open(b + ".kmer_hits.gz", "rb").read() if tag.startswith("depth") else None, stats)
        assert os.path.exists(b + ".coverage_rarefaction") == tag.endswith("_on")
        if tag.endswith("_on"):
            got = _rtable(b + ".coverage_rarefaction")
            assert got == {paths[0].name.encode(): [(f,) + w for f, w in zip(fields, want)]}, tag
    for kind in ("only", "depth"):                             # stdout, stderr, the main table and -o: the same bytes, flag on or off
        assert outs[kind + "_on"][:4] == outs[kind + "_off"][:4], kind
    dev, replayed = (int(x) for x in WENT.search(outs["only_on"][0]).groups())
    if case == "pe_not_lined_up":
        assert replayed >= 10
    else:
        assert dev >= 10 and (replayed >= 1 or case == "pe_lined_up"), (dev, replayed)


def test_program_forms_gz_many_strains_two_unions_two_devices_the_cache_and_the_other_tables(job):  # noqa: F811
    mode, files = _targets(job)["pei_short_read_and_missing_last_mate"]
    d = job.d / "rar_forms"
    d.mkdir()
    paths = _write(d, "in", files, gz=True)
    T, fields = rm.parse_list(P_LIST)
    strains = (0, 1, 2, 3)
    want = {}
    for s in strains:
        w = _reruns(job, d, mode, files, T, s)
        want[s] = [(f,) + (x[0], x[1], x[2]) for f, x in zip(fields, w)]
    assert sum(w[2][3] for w in want.values()) > 0
    cache = d / "cache"
    cache.mkdir()
    others = ["--coverage-regions", "--coverage-spectrum", "--coverage-thresholds", "--coverage-support", "--coverage-recurrence"]
    forms = [("S", "--coverage-only", {}, []), ("two_unions", "--coverage-only", {"SK_SD_GROUP": "2"}, []),
             ("dev2", "--coverage-only", {"SK_DEVICES": "0,0", "SK_SD_GROUP": "2"}, []), ("nounion", "--coverage-only", {"SK_SD_NO_UNION": "1"}, []),
             ("depth", "--coverage-depth", {}, []), ("beside", "--coverage-only", {}, others),
             ("pack", "--coverage-only", {"SK_SD_PACK": "1"}, []),
             ("cache_fill", "--coverage-only", {}, ["--target-cache", str(cache)]), ("cache_served", "--coverage-only", {}, ["--target-cache", str(cache)])]
    for tag, flag, env, extra in forms:
        (d / tag).mkdir()
        (d / (tag + ".S")).write_text("".join(f"{job.d}/s{s}.fa\t{job.d}/s{s}.inf.gz\t{d}/{tag}/{NAME % s}\n" for s in strains))
        argv = ["-S", str(d / (tag + ".S")), "-b", str(paths[0]), "-t", mode, flag, "--coverage-rarefaction", "--rarefaction-list", P_LIST,
                "--rarefaction-seed", str(P_SEED)] + extra
        rc, err, _ = _run_sd(argv, dict(TINY, **env), d, tag)
        assert rc == 0, (tag, err.decode()[-600:])
        for s in strains:
            got = _rtable(_base(d / tag / (NAME % s)) + ".coverage_rarefaction", named=True)
            assert got == {((NAME % s)[: -len(".kmer_hits.gz")].encode(), paths[0].name.encode()): want[s]}, (tag, s)


def test_program_plain_text_parsed_on_the_device_two_targets_and_a_file_of_its_own(job):  # noqa: F811
    """SK_DEVICE_PARSE=1 on a plain file, two targets in one run (one row block per target, in order), --coverage-rarefaction=FILE"""
    t = _targets(job)
    d = job.d / "rar_two"
    d.mkdir()
    T, fields = rm.parse_list(P_LIST)
    rows, lines = {}, []
    for k, case in enumerate(("se_short_read", "pei_short_read_and_missing_last_mate")):
        mode, files = t[case]
        sub = d / f"t{k}"
        sub.mkdir()
        p = _write(sub, f"in{k}", files)
        rows[p[0].name.encode()] = [(f,) + w for f, w in zip(fields, _reruns(job, sub, mode, files, T))]
        lines.append(f"{mode}\t{p[0]}\n")
    (d / "T.txt").write_text("".join(lines))
    for tag, env in (("host_parse", TINY), ("device_parse", dict(TINY, SK_DEVICE_PARSE="1"))):
        (d / tag).mkdir()
        out = d / (tag + ".table")
        argv = ["-r", str(job.d / "s1.fa"), "-a", str(job.d / "s1.inf.gz"), "-B", str(d / "T.txt"), "-o", str(d / tag / (NAME % 1)),
                "--coverage-only", f"--coverage-rarefaction={out}", f"--rarefaction-list={P_LIST}", f"--rarefaction-seed={P_SEED}"]
        rc, err, _ = _run_sd(argv, env, d, tag)
        assert rc == 0, err.decode()[-600:]
        got = _rtable(out)
        assert got == rows and list(got) == list(rows), tag


def test_program_refusals_before_anything_is_read(job):  # noqa: F811
    d = job.d / "rar_refused"
    d.mkdir()
    base = ["-r", str(job.d / "s1.fa"), "-a", str(job.d / "s1.inf.gz"), "-b", str(d / "no_such_file.fa"), "-t", "SE", "-o", str(d / (NAME % 1))]
    for k, extra in enumerate((["--coverage-only", "--coverage-rarefaction", "--rarefaction-list", "0.5,0.5"],
                               ["--coverage-only", "--coverage-rarefaction", "--rarefaction-list", "0.25,0.5"],
                               ["--coverage-only", "--coverage-rarefaction", "--rarefaction-list", "1.5"],
                               ["--coverage-only", "--coverage-rarefaction", "--rarefaction-seed", "4294967296"],
                               ["--coverage-only", "--coverage-rarefaction", "--rarefaction-seed", "-1"],
                               ["--coverage-only", "--rarefaction-list", "1,0.5"],
                               ["--coverage-rarefaction"])):
        rc, err, _ = _run_sd(base + extra, {}, d, f"r{k}")
        assert rc != 0 and b"rarefaction" in err and b"no_such_file" not in err, (extra, err)


@pytest.mark.parametrize("flag", ["--coverage-only", "--coverage-depth"])
def test_program_a_short_record_that_repeats_its_neighbours_lines_counts_them_for_its_own_pair(job, flag):  # noqa: F811
    """The documented behaviour where a rerun cannot be the yardstick: a record shorter than k behind a read with informative hits prints
    that read's lines again (the reference's read loop), and the table counts them for the SHORT record's pair.  The leading reads hit
    no strain, and their number is chosen so that exactly one of the two pairs is in the subsample at 0.5."""
    rng = random.Random(5)
    T, fields = rm.parse_list("1,0.5")
    n = next(k for k in range(10, 200) if rm.keep(k, T[1], P_SEED) != rm.keep(k + 1, T[1], P_SEED))
    junk = [_synth.rand_dna(rng, 80) for _ in range(n + 30)]
    files = [junk[:n] + [job.hit, b"ACGTACGT"] + junk[n:]]
    d = job.d / ("rar_short_" + flag.strip("-"))
    d.mkdir()
    alone = _write(d, "alone", [[job.hit]])
    rc, err, _ = _run_sd(_argv(job, d, "alone", "SE", alone) + ["--coverage-only"], {}, d, "alone")
    assert rc == 0, err.decode()[-600:]
    u, t = main_table(open(_base(d / "alone" / (NAME % 1)) + ".coverage_depth", "rb").read())[alone[0].name.encode()]
    assert u > 0 and t >= u
    paths = _write(d, "in", files)
    rc, err, _ = _run_sd(_argv(job, d, "run", "SE", paths) + [flag, "--coverage-rarefaction", "--rarefaction-list", "1,0.5", "--rarefaction-seed", str(P_SEED)],
                         TINY, d, "run")
    assert rc == 0, err.decode()[-600:]
    b = _base(d / "run" / (NAME % 1))
    assert main_table(open(b + ".coverage_depth", "rb").read())[paths[0].name.encode()] == (u, 2 * t)       # the lines were printed twice
    pairs = [sum(rm.keep(k, tq, P_SEED) for k in range(len(files[0]))) for tq in T]
    assert _rtable(b + ".coverage_rarefaction") == {paths[0].name.encode(): [(fields[0], pairs[0], u, 2 * t), (fields[1], pairs[1], u, t)]}


def test_program_two_ranks_each_writes_its_own_strains_tables(job):  # noqa: F811
    mode, files = _targets(job)["pei_short_read_and_missing_last_mate"]
    d = job.d / "rar_ranks"
    d.mkdir()
    paths = _write(d, "in", files)
    T, fields = rm.parse_list(P_LIST)
    strains = (0, 1, 2, 3)
    want = {s: [(f,) + w for f, w in zip(fields, _reruns(job, d, mode, files, T, s))] for s in strains}
    for rank in (0, 1):
        r = d / f"rank{rank}"
        r.mkdir()
        (r / "S.txt").write_text("".join(f"{job.d}/s{s}.fa\t{job.d}/s{s}.inf.gz\t{r}/{NAME % s}\n" for s in strains))
        argv = ["-S", str(r / "S.txt"), "-b", str(paths[0]), "-t", mode, "--coverage-only", "--coverage-rarefaction", "--rarefaction-list", P_LIST,
                "--rarefaction-seed", str(P_SEED)]
        rc, err, _ = _run_sd(argv, dict(TINY, WORLD_SIZE="2", RANK=str(rank)), d, f"rank{rank}")
        assert rc == 0, err.decode()[-600:]
        for i, s in enumerate(strains):
            p = _base(r / (NAME % s)) + ".coverage_rarefaction"
            assert os.path.exists(p) == (i % 2 == rank), (rank, s)
            if i % 2 == rank:
                assert _rtable(p, named=True) == {((NAME % s)[: -len(".kmer_hits.gz")].encode(), paths[0].name.encode()): want[s]}
