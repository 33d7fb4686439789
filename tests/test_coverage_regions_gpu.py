"""strain_detect --coverage-regions on the device (include/strainer_kmer.h has the rule): sk_table_first_pos against the host
builder's first positions, the fold by region (sk_covacc_set_regions / _region_rows / _finish_target_regions) against a model built
from the existing collections exactly as test_coverage_only_gpu.py's model() builds its own, plus row -> region, and the program in
all the forms it runs in against a table computed in Python from the hit list --coverage-depth writes (tests/_regions_model.py).

World of the library-level tests: three strains of about 3 kbp --
  A  one record, rows in strain order, one region (W = 0);
  B  records of 1000, 31, 29 (skipped) and 1969 bases, rows in the reference's slot order, W = 64: 48 regions, the few-bins path;
     informative 31-mers start at offsets W - 1 and W of two records, in the last window of a record, at a record's last possible
     start, and the record of exactly 31 bases is one;
  C  two records of 1500 bases, reference order, W = 2: 1500 regions, more than a workgroup keeps in LDS: the many-bins path --
and reads of 31 to 150 bases, 700 a batch."""
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
from _regions_model import NO_POS, StrainModel, expected_table, model_regions, region_of_pos
from strainer2_amd import native
from test_coverage_only_gpu import NAME, WENT, _canon, _fa, _fq, _mutate, _union_collect, model

pytestmark = pytest.mark.gpu

STRAIN_ORDER = 0xFFFFFFFF
WB = 64


def _stream(recs):
    return b"\n".join(recs) + b"\n", np.cumsum([0] + [len(r) + 1 for r in recs[:-1]]).astype(np.uint32)


class World:
    pass


def _reads(rng, strains, special, n):
    out = list(special)
    while len(out) < n:
        ln = rng.choice([31, 31, 32, 47, 64, 100, 150])
        if rng.random() < 0.6:
            g = rng.choice([r for s in strains for r in s if len(r) > ln])
            a = rng.randrange(len(g) - ln)
            seq = g[a:a + ln]
            out.append(_synth.revcomp(seq) if rng.random() < 0.5 else seq)
        else:
            out.append(_synth.rand_dna(rng, ln))
    rng.shuffle(out)
    return out


@pytest.fixture(scope="module")
def world():
    rng = random.Random(31337)
    d = _synth.rand_dna
    w = World()
    w.strains = [[d(rng, 3000)], [d(rng, 1000), d(rng, 31), d(rng, 29), d(rng, 1969)], [d(rng, 1500), d(rng, 1500)]]
    w.window = [0, WB, 2]
    order = [STRAIN_ORDER, native.SK_REF_TABLE_SLOTS, native.SK_REF_TABLE_SLOTS]
    b0, b1, b3 = w.strains[1][0], w.strains[1][1], w.strains[1][3]
    # text positions of strain B's placed informative 31-mers: record 1 at W - 1, W, in its last window and at its last start;
    # the 31-base record; record 4 (text offset 1031) at W - 1 and W
    w.placed = [WB - 1, WB, 965, 969, 1000, 1031 + WB - 1, 1031 + WB]
    special = [b0[30:130], _synth.revcomp(b0[40:140]), b0[900:1000], _synth.revcomp(b0[930:1000]), b0[969:1000], b1, _synth.revcomp(b1),
               b3[20:120], _synth.revcomp(b3[33:133]), b3[WB:WB + 31]]
    w.ctxs, w.sets, w.fp, w.starts, w.typ = [], [], [], [], []
    for i, recs in enumerate(w.strains):
        ks = sk.Keyset.from_stream(b"\n".join(recs) + b"\n", initial_slots=order[i], default_val=1, incr=0)
        c = sk.KmerContext(0)
        c.load_keyset(ks, 6)
        fp = ks.first_pos()
        typ = np.full(ks.nrows, 1, dtype=np.uint32)
        typ[np.array(rng.sample(range(ks.nrows), ks.nrows // 60))] = 2
        if i == 1:
            for p in w.placed:
                assert (fp == p).sum() == 1
                typ[fp == p] = 2
        c.set_counts(0, typ)
        regs, n = model_regions([(b"r%d" % j, r) for j, r in enumerate(recs)], w.window[i])
        assert n == sum(len(r) for r in recs if len(r) >= 30)
        w.ctxs.append(c)
        w.sets.append(ks)
        w.fp.append(fp)
        w.typ.append(typ)
        w.starts.append(np.array([r[0] for r in regs], dtype=np.uint32))
    assert [len(s) for s in w.starts] == [1, 16 + 1 + 31, 1500]
    w.nrows = [k.nrows for k in w.sets]
    w.recs1 = _reads(rng, w.strains, special, 700)
    w.recs2 = _reads(rng, w.strains, [_synth.revcomp(x) for x in special], 700)
    w.s1, w.st1 = _stream(w.recs1)
    w.s2, w.st2 = _stream(w.recs2)
    w.b1, w.b2 = native.TallyBatch(w.ctxs[1]), native.TallyBatch(w.ctxs[1])
    w.b1.fill(w.s1, w.st1)
    w.b2.fill(w.s2, w.st2)
    w.union = sk.KmerUnion(w.ctxs, 0, 2)
    w.single, w.uni = [], []
    for b in (w.b1, w.b2):                                   # the reference results, once: what the existing collections return
        w.ctxs[1].tally_launch(b)
        recs, hits, nh = w.ctxs[1].tally_collect_sparse()
        assert nh == len(hits)
        w.single.append((recs.copy(), hits.copy()))
        w.union.tally_launch(b)
        w.uni.append(_union_collect(w.union, b))
    for v in w.single + w.uni:
        v[0].setflags(write=False)
        v[1].setflags(write=False)
    yield w
    w.union.close()
    w.b1.close()
    w.b2.close()
    for c in w.ctxs:
        c.close()
    for k in w.sets:
        k.close()


def fold(depth, fp, starts):
    """(unique, total) per region, the unplaced rows' last: the model's row -> region"""
    reg = region_of_pos(fp, starts)
    nb = len(starts) + 1
    return (np.bincount(reg[depth > 0], minlength=nb).astype(np.uint64),
            np.bincount(reg, weights=depth.astype(np.float64), minlength=nb).astype(np.uint64))


def _check(w, acc, members, want, again):
    """acc holds a fold of `want` (per-member depth arrays of the world's strains `members`): the region pairs are the model's,
    their sums what finish_target returns for the same launch (`again` folds it once more), everything is zero afterwards"""
    for m, d in enumerate(want):
        assert np.array_equal(acc.rows(m), d), ("rows of member", m)
    uq, tot, per = acc.finish_target_regions()
    for m, d in enumerate(want):
        u, t = fold(d, w.fp[members[m]], w.starts[members[m]])
        assert np.array_equal(per[m][0], u) and np.array_equal(per[m][1], t), ("regions of member", m)
        assert (int(uq[m]), int(tot[m])) == (int(per[m][0].sum()), int(per[m][1].sum())) == (int(np.count_nonzero(d)), int(d.sum()))
    uq2, tot2, per2 = acc.finish_target_regions()            # a second finish: everything was cleared
    assert not uq2.any() and not tot2.any() and not any(p[0].any() or p[1].any() for p in per2)
    for m in range(len(want)):
        assert not acc.rows(m).any()
    again()
    uq3, tot3 = acc.finish_target()                          # the sweep without regions, same launch: the members' sums
    assert np.array_equal(uq3, uq) and np.array_equal(tot3, tot)
    return uq, tot, per


# ---------------------------------------------------------------------------------------------------------------------------------
# first positions
# ---------------------------------------------------------------------------------------------------------------------------------
def _strain_cases():
    rng = random.Random(808)
    d = _synth.rand_dna
    a, b = d(rng, 1400), d(rng, 1500)
    rep = a[200:231]
    return {
        "plain": [d(rng, 3000)],
        "n_run": [d(rng, 900) + b"N" * 40 + d(rng, 700) + b"n" + d(rng, 30) + b"N" + d(rng, 1300)],
        "repeat": [a, b[:500] + rep + b[500:900] + _synth.revcomp(a[700:731]) + b[900:], d(rng, 31), d(rng, 29), d(rng, 30)],
        "u": [d(rng, 800) + b"U" + d(rng, 700), d(rng, 600)],
    }


@pytest.mark.parametrize("case", ["plain", "n_run", "repeat", "u"])
def test_first_positions(case):
    recs = _strain_cases()[case]
    stream = b"\n".join(recs) + b"\n"
    sm = StrainModel(b"".join(b">r%d\n%s\n" % (i, r) for i, r in enumerate(recs)), 0)
    by_order = {}
    for order in (STRAIN_ORDER, native.SK_REF_TABLE_SLOTS):
        ks = sk.Keyset.from_stream(stream, initial_slots=order, default_val=1, incr=0)
        with sk.KmerContext(0) as c:
            c.load_keyset(ks, 2)
            got = c.first_pos()
        want = ks.first_pos()
        assert np.array_equal(got, want), (case, order)
        placed = want != NO_POS
        assert placed.sum() == len(sm.pos) and np.array_equal(np.sort(want[placed]), np.sort(sm.pos))      # (the model's, too)
        if case == "u":
            assert (~placed).sum() > 0 and ks.nwide > 0      # rows without a position
        else:
            assert placed.all()
        by_order[order] = want
        ks.close()
    assert not np.array_equal(by_order[STRAIN_ORDER], by_order[native.SK_REF_TABLE_SLOTS])           # (two row orders)
    if case == "repeat":                                     # the repeated 31-mers belong to the first record
        reg, _ = sm.regions_of([recs[0][200:231], recs[0][700:731], _synth.revcomp(recs[0][700:731])])
        assert reg.tolist() == [0, 0, 0]
    if case != "u":                                          # a table built on the device: rows in strain order
        with sk.KmerContext(0) as c:
            n = c.build_from_text(recs, 2, 1)
            got = c.first_pos()
        assert n == len(by_order[STRAIN_ORDER]) and np.array_equal(got, by_order[STRAIN_ORDER])
        assert (np.diff(got.astype(np.int64)) > 0).all()


def test_first_positions_without_a_table():
    with sk.KmerContext(0) as c:
        with pytest.raises(sk.SKError):
            c.first_pos()


# ---------------------------------------------------------------------------------------------------------------------------------
# the fold
# ---------------------------------------------------------------------------------------------------------------------------------
def test_world_has_the_cases_it_claims(world):
    w = world
    recs, hits = w.single[0]
    d = model([w.nrows[1]], 1, False, [(recs, hits, w.st1, 0, 1)], len(w.st1), 0)[0]
    for p in w.placed:
        assert d[w.fp[1] == p][0] >= 1, p                    # every placed informative 31-mer is hit
    reg = region_of_pos(w.placed, w.starts[1])
    assert reg.tolist() == [0, 1, 15, 15, 16, 17, 18]        # W - 1 and W fall into two windows; the 31-base record is region 16
    urecs, uhits = w.uni[0]
    for m in range(3):
        assert ((uhits[:, 1] >> 27) == m).sum() > 0


@pytest.mark.parametrize("min_hits", [0, 1, 5])
def test_region_rows_and_single_reads(world, min_hits):
    w = world
    recs, hits = w.single[0]
    c = w.ctxs[1]
    with sk.CoverageAcc(c, [w.nrows[1]], min_hits) as acc:
        acc.set_regions(0, c, w.starts[1])
        rows, inf = acc.region_rows(0, c, 0, 2)
        reg = region_of_pos(w.fp[1], w.starts[1])
        assert np.array_equal(rows, np.bincount(reg, minlength=len(w.starts[1]) + 1))
        assert np.array_equal(inf, np.bincount(reg[w.typ[1] == 2], minlength=len(w.starts[1]) + 1))
        assert int(rows.sum()) == w.nrows[1] and int(rows[16]) == 1 and int(inf[16]) == 1

        def launch():
            c.tally_launch(w.b1)
            c.tally_collect_counts()
            acc.add(c, 0, 1, w.b1.nrec)
        launch()
        want = model([w.nrows[1]], 1, False, [(recs, hits, w.st1, 0, 1)], w.b1.nrec, min_hits)
        uq, tot, per = _check(w, acc, [1], want, launch)
        assert int(tot[0]) >= int(uq[0]) > 0 and int(per[0][0][-1]) == 0
        if min_hits == 0:                                    # (the read that is the 31-base record has one hit in all)
            assert int(per[0][0][16]) == 1


@pytest.mark.parametrize("min_hits", [0, 5])
def test_interleaved_pairs_and_pairs_over_two_batches(world, min_hits):
    w = world
    (r1, h1), (r2, h2) = w.single
    c = w.ctxs[1]
    np_ = w.b1.nrec // 2
    with sk.CoverageAcc(c, [w.nrows[1]], min_hits) as acc:
        acc.set_regions(0, c, w.starts[1])

        def pei():
            c.tally_launch(w.b1)
            c.tally_collect_counts()
            acc.add(c, 0, 2, np_, mate=("same", 1, 2))
        pei()
        _check(w, acc, [1], model([w.nrows[1]], 1, False, [(r1, h1, w.st1, 0, 2), (r1, h1, w.st1, 1, 2)], np_, min_hits), pei)

        def pe():
            c.tally_launch(w.b1)
            c.tally_collect_counts()
            acc.hold(c)
            c.tally_launch(w.b2)
            c.tally_collect_counts()
            acc.add(c, 4, 1, w.b1.nrec - 4, mate=("held", 2, 1))
        pe()
        _check(w, acc, [1], model([w.nrows[1]], 1, False, [(r2, h2, w.st2, 4, 1), (r1, h1, w.st1, 2, 1)], w.b1.nrec - 4, min_hits), pe)


@pytest.mark.parametrize("min_hits", [0, 1, 5])
def test_union_of_three_with_1_48_and_1500_regions(world, min_hits):
    w = world
    u = w.union
    r1, h1 = w.uni[0]
    with sk.CoverageAcc(w.ctxs[0], w.nrows, min_hits) as acc:
        for m in range(3):
            acc.set_regions(m, w.ctxs[m], w.starts[m])
            rows, inf = acc.region_rows(m, w.ctxs[m], 0, 2)
            reg = region_of_pos(w.fp[m], w.starts[m])
            assert np.array_equal(rows, np.bincount(reg, minlength=len(w.starts[m]) + 1)), m
            assert np.array_equal(inf, np.bincount(reg[w.typ[m] == 2], minlength=len(w.starts[m]) + 1)), m

        def launch():
            u.tally_launch(w.b1, results_stay=True)
            u.tally_collect_counts()
            acc.add(u, 0, 1, w.b1.nrec)
        launch()
        want = model(w.nrows, 3, True, [(r1, h1, w.st1, 0, 1)], w.b1.nrec, min_hits)
        uq, tot, per = _check(w, acc, [0, 1, 2], want, launch)
        assert [len(p[0]) for p in per] == [2, 49, 1501]
        assert all(int(t) > 0 for t in tot) and np.count_nonzero(per[2][0]) > 0


def test_a_member_whose_regions_were_never_set_is_all_unplaced(world):
    w = world
    c = w.ctxs[1]
    with sk.CoverageAcc(c, [w.nrows[1], w.nrows[2]], 0) as acc:
        acc.set_regions(1, w.ctxs[2], w.starts[2])
        acc.add_rows(0, [3, 3, 9])
        acc.add_rows(1, [0, 5])
        uq, tot, per = acc.finish_target_regions()
        assert uq.tolist() == [2, 2] and tot.tolist() == [3, 2]
        assert per[0][0].tolist() == [2] and per[0][1].tolist() == [3] and int(per[1][0].sum()) == 2


def test_rows_from_the_host_unplaced_rows_and_bad_calls():
    """a strain with a U: byte-string keys have no text position and go to the extra region; rows come in through add_rows"""
    recs = _strain_cases()["u"]
    ks = sk.Keyset.from_stream(b"\n".join(recs) + b"\n", default_val=1, incr=0)
    fp = ks.first_pos()
    regs, _ = model_regions([(b"x", r) for r in recs], 100)
    starts = np.array([r[0] for r in regs], dtype=np.uint32)
    with sk.KmerContext(0) as c:
        c.load_keyset(ks, 2)
        typ = np.full(ks.nrows, 1, dtype=np.uint32)
        typ[::50] = 2
        un = np.nonzero(fp == NO_POS)[0]
        typ[un[:3]] = 2
        c.set_counts(0, typ)
        with sk.CoverageAcc(c, [ks.nrows], 0) as acc:
            acc.set_regions(0, c, starts)
            reg = region_of_pos(fp, starts)
            rows, inf = acc.region_rows(0, c, 0, 2)
            assert np.array_equal(rows, np.bincount(reg, minlength=len(starts) + 1)) and int(rows[-1]) == len(un) > 0
            assert np.array_equal(inf, np.bincount(reg[typ == 2], minlength=len(starts) + 1)) and int(inf[-1]) >= 3
            given = [int(un[0]), int(un[0]), int(un[2]), 0, 1, 1, 1, ks.nrows - 1]
            acc.add_rows(0, given)
            depth = np.bincount(given, minlength=ks.nrows).astype(np.uint32)
            uq, tot, per = acc.finish_target_regions()
            u, t = fold(depth, fp, starts)
            assert np.array_equal(per[0][0], u) and np.array_equal(per[0][1], t)
            assert (int(per[0][0][-1]), int(per[0][1][-1])) == (2, 3) and (int(uq[0]), int(tot[0])) == (5, 8)
            assert not acc.rows(0).any()
            with pytest.raises(sk.SKError):
                acc.set_regions(1, c, starts)                # no such member
            with pytest.raises(sk.SKError):
                acc.set_regions(0, c, starts[::-1].copy())   # starts must ascend
        with sk.CoverageAcc(c, [ks.nrows + 1], 0) as acc:
            with pytest.raises(sk.SKError):
                acc.set_regions(0, c, starts)                # another table's row count
    ks.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# the program
# ---------------------------------------------------------------------------------------------------------------------------------
class Job:
    pass


def _wrap(seq, n):
    return b"\n".join(seq[i:i + n] for i in range(0, len(seq), n))


@pytest.fixture(scope="module")
def job(tmp_path_factory):
    """four strains of about 3 kbp in several records (1 and 2 related), wrapped lines and header comments, a record of 29 bases that
    is skipped but numbered and one of 31 bases; every 97th k-mer informative, a block of them near text position 1000, and the ones
    that start at offsets 499 and 500 of a record (W = 500), in a record's last window and in the 31-base record"""
    d = tmp_path_factory.mktemp("covregions")
    rng = random.Random(60606)
    j = Job()
    j.d = d
    g1 = [_synth.rand_dna(rng, n) for n in (1300, 31, 29, 1700)]
    j.strains = [[_synth.rand_dna(rng, n) for n in (2000, 1100)], g1, [_mutate(rng, r, 0.02, (0, 0)) for r in g1],
                 [_synth.rand_dna(rng, 2900)]]
    for s, recs in enumerate(j.strains):
        (d / f"s{s}.fa").write_bytes(b"".join(b">s%d_rec%d len=%d\n%s\n" % (s, i, len(r), _wrap(r, 70)) for i, r in enumerate(recs)))
        kms = set()
        for r in recs:
            kms |= {_canon(r[i:i + 31]) for i in range(s, len(r) - 30, 97)}
            if len(r) == 31:
                kms.add(_canon(r))
            if len(r) > 1100:
                kms |= {_canon(r[i:i + 31]) for i in (499, 500, 1000, 1010, 1020, len(r) - 31)}
        with gzip.open(d / f"s{s}.inf.gz", "wb") as f:
            f.write(b"#informative\n" + b"\n".join(sorted(kms)) + b"\n")

    def reads(n, seed):
        r = random.Random(seed)
        out = []
        for _ in range(n):
            ln = r.choice([31, 31, 75, 100, 150, r.randrange(31, 151)])
            if r.random() < 0.4:
                g = r.choice([x for x in j.strains[r.randrange(4)] if len(x) >= 31])
                if len(g) <= ln:
                    rd = g
                else:
                    a = r.randrange(440, 560) if r.random() < 0.3 and len(g) > 700 else r.randrange(0, len(g) - ln)
                    rd = g[a:a + ln]
                rd = _synth.revcomp(rd) if r.random() < 0.5 else rd
            else:
                rd = _synth.rand_dna(r, ln)
            out.append(rd)
        return out

    j.reads = reads
    j.hit = j.strains[1][0][450:550]                         # a read with informative hits on strains 1 and 2 (offsets 499 and 500)
    se, p1, p2, il = reads(1200, 1), reads(700, 2), reads(700, 3), reads(800, 4)
    assert all(len(x) >= 31 for x in se + p1 + p2 + il)
    with gzip.open(d / "se.fq.gz", "wb", compresslevel=1) as f:
        f.write(_fq(se))
    (d / "pe_1.fa").write_bytes(_fa(p1))
    (d / "pe_2.fa").write_bytes(_fa(p2))
    (d / "il.fq").write_bytes(_fq(il))
    (d / "none.fa").write_bytes(_fa([_synth.rand_dna(rng, 80) for _ in range(50)]))          # a target without any hit
    (d / "clean.txt").write_text(f"SE\t{d}/se.fq.gz\nPE\t{d}/pe_1.fa\t{d}/pe_2.fa\nSE\t{d}/none.fa\nPEI\t{d}/il.fq\n")
    return j


def _run_sd(argv, env, out_dir, tag):
    """strain_detect in this process, `env` set for the length of the run: (status, stderr, the run's coverage_only_stats)"""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        native.coverage_only_stats(reset=True)
        rc = native.run_strain_detect_inprocess(argv, str(out_dir / (tag + ".out")), str(out_dir / (tag + ".err")))
        stats = native.coverage_only_stats(reset=True)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return rc, open(out_dir / (tag + ".err"), "rb").read(), stats


def _base(p):
    return str(p)[: -len(".kmer_hits.gz")]


def _case(job, tag, targets, strains=(1,), env=None, window=("--region-window", "500"), min_hits=None, clean=False):
    """the four runs of one case: --coverage-depth and --coverage-only, each with and without --coverage-regions.  Both region
    tables equal the model computed from the hit list --coverage-depth wrote, and each other byte for byte; without the flag the
    coverage table and the hit list are the same bytes.  Returns ({strain: region table}, stats of the --coverage-only run with the
    flag, its stderr)."""
    d = job.d / tag
    d.mkdir()
    env = dict(env or {}, SK_SD_RESULT_BYTES="1")
    extra = list(targets) + (["--min-kmer-hits", str(min_hits)] if min_hits is not None else [])
    w = int(window[1]) if window else 100000
    outs, keep = {}, {}
    for run, flags in (("depth_rg", ["--coverage-depth", "--coverage-regions"] + list(window or ())), ("depth", ["--coverage-depth"]),
                       ("only_rg", ["--coverage-only", "--coverage-regions"] + list(window or ())), ("only", ["--coverage-only"])):
        (d / run).mkdir()
        if len(strains) > 1:
            (d / (run + ".S")).write_text("".join(f"{job.d}/s{s}.fa\t{job.d}/s{s}.inf.gz\t{d}/{run}/{NAME % s}\n" for s in strains))
            argv = ["-S", str(d / (run + ".S"))]
        else:
            s = strains[0]
            argv = ["-r", str(job.d / f"s{s}.fa"), "-a", str(job.d / f"s{s}.inf.gz"), "-o", str(d / run / (NAME % s))]
        rc, err, stats = _run_sd(argv + extra + flags, env, d, run)
        assert rc == 0, err.decode()[-600:]
        keep[run] = (stats, err)
        outs[run] = {}
        for s in strains:
            b = _base(d / run / (NAME % s))
            o = {"table": open(b + ".coverage_depth", "rb").read()}
            if run.startswith("depth"):
                o["hits"] = gzip.open(b + ".kmer_hits.gz", "rb").read()
            assert os.path.exists(b + ".coverage_regions") == run.endswith("_rg"), (run, s)
            if run.endswith("_rg"):
                o["regions"] = open(b + ".coverage_regions", "rb").read()
            outs[run][s] = o
    tables = {}
    for s in strains:
        assert outs["depth_rg"][s]["table"] == outs["depth"][s]["table"] == outs["only_rg"][s]["table"] == outs["only"][s]["table"]
        assert outs["depth_rg"][s]["hits"] == outs["depth"][s]["hits"]
        want = expected_table(str(job.d / f"s{s}.fa"), str(job.d / f"s{s}.inf.gz"), _base(d / "depth_rg" / (NAME % s)) + ".kmer_hits.gz",
                              outs["depth"][s]["table"], w, 1 if min_hits is None else min_hits)
        assert outs["depth_rg"][s]["regions"] == want, ("--coverage-depth", s)
        assert outs["only_rg"][s]["regions"] == want, ("--coverage-only", s)
        tables[s] = want
    stats, err = keep["only_rg"]
    went = WENT.search(err)
    assert went and (int(went.group(1)), int(went.group(2))) == stats[:2]
    if clean:                                                # counted on the device: no host fallback stands in for the kernel
        assert stats[0] >= 1 and stats[1] == 0 and stats[2] == 0, stats
    return tables, stats, err


def _rows(table):
    return [ln.split(b"\t") for ln in table.splitlines()[1:]]


@pytest.mark.parametrize("min_hits", [None, 0, 40])
def test_program_clean_targets(job, min_hits):
    """SE (.gz FASTQ), PE over two files, a target without a hit and PEI, reads of 31 bases or more: all counted on the device"""
    t, stats, _ = _case(job, f"clean{min_hits}", ["-B", str(job.d / "clean.txt")], min_hits=min_hits, clean=True)
    rows = _rows(t[1])
    regions = [r[2] for r in rows if r[1] == b"se.fq.gz"]
    assert regions == [b"1:0-500", b"1:500-1000", b"1:1000-1300", b"2:0-31", b"4:0-500", b"4:500-1000", b"4:1000-1500", b"4:1500-1700"]
    assert [r[3] for r in rows[:4]] == [b"s1_rec0", b"s1_rec0", b"s1_rec0", b"s1_rec1"]
    assert sorted(r[1] for r in rows[::8]) == [b"il.fq", b"none.fa", b"pe_1.fa", b"se.fq.gz"] and len(rows) == 32
    assert all(r[5:] == [b"0", b"0", b"0.0", b"0.0"] for r in rows if r[1] == b"none.fa")
    if min_hits != 40:
        assert [r[1] for r in rows[::8]] == [b"se.fq.gz", b"pe_1.fa", b"il.fq", b"none.fa"]   # (the coverage table's order: no hit, last)
        assert all(sum(int(r[6]) for r in rows if r[1] == m) > 0 for m in (b"se.fq.gz", b"pe_1.fa", b"il.fq"))
        assert stats[0] >= 4


@pytest.mark.parametrize("window", [None, ("--region-window", "0"), ("--region-window", "64"), ("--region-window", "1")])
def test_program_windows(job, window):
    """the default window (one region per record here), W = 0, and windows small enough for more regions than a workgroup keeps in
    LDS (W = 1: 3031 regions)"""
    t, _, _ = _case(job, "win" + (window[1] if window else "default"), ["-b", str(job.d / "se.fq.gz")], window=window, clean=True)
    rows = _rows(t[1])
    if window is None or window[1] == "0":
        assert [r[2] for r in rows] == [b"1:0-1300", b"2:0-31", b"4:0-1700"]
    if window and window[1] == "64":
        byreg = {r[2]: r for r in rows}
        assert int(byreg[b"1:448-512"][4]) >= 2                # offsets 499 and 500 of record 1 lie in one window of 64 ...
    if window and window[1] == "1":
        byreg = {r[2]: r for r in rows}
        assert b"1:499-500" in byreg and b"1:500-501" in byreg  # ... and in two of one base


@pytest.mark.parametrize("mode,files", [("PE", ["pe_1.fa", "pe_2.fa"]), ("PEI", ["il.fq"])])
def test_program_single_targets(job, mode, files):
    argv = ["-b", str(job.d / files[0]), "-t", mode] + (["-c", str(job.d / files[1])] if mode == "PE" else [])
    _, stats, _ = _case(job, "one" + mode, argv, clean=True)
    assert stats[0] == 1


def _short_cases(job):
    h, r = job.hit, job.reads
    a, b = r(40, 11), r(40, 12)
    stale = a[:20] + [h, h[:12], h[10:80]] + a[20:]                    # a short read between two hit reads
    pe1 = a[:10] + [h, h[5:90]] + a[10:]
    pe2 = b[:10] + [_synth.revcomp(h), h[:9]] + b[10:]                 # a short PE2 mate behind a hit pair
    odd = a[:11] + [h, _synth.revcomp(h), h[20:100]]
    return {"stale": ("SE", [_fa(stale)]), "short_mate": ("PE", [_fa(pe1), _fa(pe2)]), "pei_odd": ("PEI", [_fa(odd if len(odd) % 2 else odd + [h])])}


@pytest.mark.parametrize("case", ["stale", "short_mate", "pei_odd"])
def test_program_fallback_inputs(job, case):
    """reads shorter than 31 bases: runs are replayed on the host and reach the counters through add_rows"""
    mode, files = _short_cases(job)[case]
    paths = []
    for i, data in enumerate(files):
        paths.append(job.d / f"{case}_{i}.fx")
        paths[-1].write_bytes(data)
    argv = ["-b", str(paths[0]), "-t", mode] + (["-c", str(paths[1])] if mode == "PE" else [])
    t, stats, _ = _case(job, "fb_" + case, argv)
    assert stats[1] > 0 and stats[2] == 0
    assert sum(int(r[6]) for r in _rows(t[1])) > 0


def test_program_two_targets_with_one_basename(job):
    r = job.reads
    for sub, seed in (("x", 31), ("y", 32)):
        (job.d / sub).mkdir()
        (job.d / sub / "same.fa").write_bytes(_fa(r(60, seed) + [job.hit, _synth.revcomp(job.hit)]))
    (job.d / "dup.txt").write_text(f"SE\t{job.d}/x/same.fa\nSE\t{job.d}/y/same.fa\n")
    t, stats, err = _case(job, "dup", ["-B", str(job.d / "dup.txt")])
    assert stats[2] == 2 and stats[0] == 0 and err.count(b"share a file name") == 1
    rows = _rows(t[1])
    assert {r[1] for r in rows} == {b"same.fa"} and len(rows) == 8 and sum(int(r[6]) for r in rows) >= 4       # one sample


def test_program_many_small_chunks(job):
    """chunks of about fifteen reads, a strain's replayed rows going to the device one at a time: runs counted on the device and
    runs replayed between them feed one set of counters"""
    h, r = job.hit, job.reads
    hits = [h, _synth.revcomp(h), h[3:97], h[10:100]]
    se = []
    for i, x in enumerate(r(900, 42)):
        se.append(x[:100].ljust(100, b"G"))
        if i % 23 == 22:
            se += [hits[i % 4], h[:7 + i % 20]]              # a hit read and a short read behind it
    (job.d / "chunks.fa").write_bytes(_fa(se))
    t, stats, _ = _case(job, "chunks", ["-b", str(job.d / "chunks.fa")], env={"SK_SD_CHUNK_BYTES": "1500", "SK_SD_CO_FLUSH_ROWS": "1"})
    assert stats[0] >= 10 and stats[1] >= 3, stats
    assert sum(int(x[6]) for x in _rows(t[1])) > 50


@pytest.mark.parametrize("env", [{}, {"SK_DEVICES": "0,0", "SK_SD_GROUP": "2"}, {"SK_SD_NO_UNION": "1"}])
def test_program_many_strains(job, env):
    """-S with three strains (1 and 2 related): one union table, two logical devices, and strain by strain"""
    t, stats, _ = _case(job, "many" + "".join(env), ["-B", str(job.d / "clean.txt")], strains=(0, 1, 2), env=env, clean=True)
    assert len({t[s] for s in t}) == 3
    for s in (1, 2):
        assert sum(int(r[6]) for r in _rows(t[s])) > 0


@pytest.mark.parametrize("env", [{"SK_SD_HOST_KEYSET": "1"}, {"SK_SD_HOST_KEYSET": "1", "SK_SD_REF_ROW_ORDER": "1"}])
def test_program_host_built_key_sets(job, env):
    """key sets built on the host, rows in strain order and in the reference's slot order (the tables --detect adopts)"""
    t, _, _ = _case(job, "hostks" + str(len(env)), ["-B", str(job.d / "clean.txt")], env=env, clean=True)
    assert sum(int(r[6]) for r in _rows(t[1])) > 0


def test_program_bundled_step_3_against_the_reference_hit_list(golden, job):
    """the bundled step 3 with --coverage-only --coverage-regions: the model fed with the REFERENCE's hit list (tests/golden/
    bundled/step3_expected.hits); 561 records, the default window; no run is replayed"""
    from test_sanitizers import COV_CASES
    b = os.path.join(golden, "bundled")
    facts = json.load(open(os.path.join(b, "step3_facts.json")))
    nm = "Bacteroides_ovatus_1001283st1_B8_1001283B150210_160208.kmer_hits.gz"
    d = job.d / "bundled"
    d.mkdir()
    argv = [os.path.join(b, a) if os.path.exists(os.path.join(b, a)) else a for a in facts["argv"]]
    argv[argv.index("-o") + 1] = str(d / nm)
    lst = d / "targets.txt"
    lst.write_text("".join("\t".join([f[0]] + [os.path.join(b, x) for x in f[1:]]) + "\n"
                           for f in (ln.split("\t") for ln in open(os.path.join(b, "target_metagenomes.txt")).read().splitlines())))
    argv[argv.index("-B") + 1] = str(lst)
    rc, err, stats = _run_sd(argv + ["--coverage-only", "--coverage-regions"], {}, d, "b")
    assert rc == 0, err.decode()[-500:]
    table = open(_base(d / nm) + ".coverage_depth", "rb").read()
    assert table == open(os.path.join(COV_CASES, "bundled_step4", "expected.stdout"), "rb").read()
    want = expected_table(argv[argv.index("-r") + 1], argv[argv.index("-a") + 1], os.path.join(b, "step3_expected.hits"), table, 100000)
    assert open(_base(d / nm) + ".coverage_regions", "rb").read() == want
    assert want.count(b"\n") > 100 and stats[0] >= 2 and stats[1] == 0 and stats[2] == 0 and not (d / nm).exists()


def test_program_fused_with_the_scrub(golden, job):
    """kmer_scrub_count -S .. --scrub .. --detect .. --coverage-regions on the bundled pair: the tables adopted from step 1 are in
    the reference's slot order; both modes write the model's table, computed from the hit lists --coverage-depth writes; the
    coverage tables are the reference chain's"""
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
    regs = {}
    for flag in ("--coverage-depth", "--coverage-only"):
        t = job.d / ("pair" + flag)
        t.mkdir()
        base = {n: str(t / os.path.basename(g)[: -len(".fna.gz")]) for n, g in facts["strains"].items()}
        with open(t / "S.txt", "w") as f:
            for n, g in facts["strains"].items():
                f.write("\t".join((g, base[n] + ".scrubbed_kmers", base[n] + ".kmer_hits.gz")) + "\n")
        argv = (["-S", str(t / "S.txt"), "-A", "genomes_to_scrub.txt", "-B", "metagenomes_to_scrub.txt"] + c["kmer_scrub_count"] +
                ["--scrub", facts["min_fraction"], "--detect"] + facts["detect_args"] + [flag, "--coverage-regions", "--region-window", "250000"])
        p = subprocess.run([sk.cli_path()] + argv, cwd=str(b), capture_output=True, env=dict(os.environ, SK_SD_RESULT_BYTES="1"))
        assert p.returncode == 0, p.stderr.decode()[-800:]
        for n in base:
            assert hashlib.md5(open(base[n] + ".coverage_depth", "rb").read()).hexdigest() == c["strains"][n]["coverage_md5"], (flag, n)
        regs[flag] = {n: open(base[n] + ".coverage_regions", "rb").read() for n in base}
        if flag == "--coverage-depth":
            for n, g in facts["strains"].items():
                want = expected_table(str(b / g), base[n] + ".scrubbed_kmers", base[n] + ".kmer_hits.gz",
                                      open(base[n] + ".coverage_depth", "rb").read(), 250000)
                assert regs[flag][n] == want and want.count(b"\n") > 20, n
        else:
            went = WENT.search(p.stderr)
            assert went and int(went.group(1)) >= 2 and int(went.group(2)) == 0
    assert regs["--coverage-depth"] == regs["--coverage-only"]
