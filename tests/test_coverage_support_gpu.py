"""Support: the read pairs behind step 4's numbers (sk_covacc_set_support / sk_covacc_finish_target_support, CoverageAcc.set_support;
include/strainer_kmer.h has the rule) against tests/_support_model.py.

Library level: tallies are launched in the world of test_coverage_only_gpu.py; the expected numbers come from the sparse records the
ORDINARY collections return for the same launches (as model() there does), fed to the model's emission rule for folded runs: an
emission of (pair, member) is tot > min_kmer_hits with a non-zero informative tally, its lines the informative tallies of both mates."""
import random

import numpy as np
import pytest

import _support_model as sm
import _synth
import strainer2_amd as sk
from strainer2_amd import native
from test_coverage_only_gpu import _stream, _union_collect, model, world  # noqa: F401  (world: the fixture)
from test_coverage_regions_gpu import STRAIN_ORDER

pytestmark = pytest.mark.gpu

MINS = [0, 5, 1000]


class Extra:
    pass


@pytest.fixture(scope="module")
def extra(world):  # noqa: F811
    """Interleaved pairs made by hand around W, the informative 31-mer strains 0 and 1 share at 1500 of a stretch (1400..1600) in
    which they are identical, so every k-mer below is a key of both:
      pair 0   A = 33 bases from 1498 (3 k-mers, W among them), B = 34 bases from 1497 (4 k-mers, W among them): at min 5 neither mate
               passes alone (3, 4 <= 5) and the pair passes on the sum (7 > 5); both mates print
      pair 1   A = 80 bases around W, B random: supported through PE1 only
      pair 2   A random, B = the other strand of those 80 bases: supported through PE2 only
      pair 3   A = 32 bases from 1499 (2 k-mers, W among them), B random: an informative hit, and a total of 2 -- an emission at
               min 0 and none at min 5
      pair 4   both random"""
    w = world
    g, rng = w.strains[0], random.Random(99)
    assert w.strains[1][1400:1600] == g[1400:1600]
    e = Extra()
    e.reads = [g[1498:1531], g[1497:1531], g[1480:1560], _synth.rand_dna(rng, 60), _synth.rand_dna(rng, 45), _synth.revcomp(g[1480:1560]),
               g[1499:1531], _synth.rand_dna(rng, 31), _synth.rand_dna(rng, 100), _synth.rand_dna(rng, 100)]
    e.s, e.st = _stream(e.reads)
    e.b = native.TallyBatch(w.ctxs[0])
    e.b.fill(e.s, e.st)
    w.union.tally_launch(e.b)
    e.uni = _union_collect(w.union, e.b)
    w.ctxs[0].tally_launch(e.b)
    recs, hits, _ = w.ctxs[0].tally_collect_sparse()
    e.single = (recs.copy(), hits.copy())
    yield e
    e.b.close()


def _expect(em, nm, member0, mh):
    """the model's tables of one target whose launches' members are members member0.. of an accumulator of nm"""
    return sm.tables([(0, j, s + member0, L, parts, tot, None) for _, j, s, L, parts, tot, _ in em], 1, nm, mh, group=nm)


def _check(acc, em, member0=0, mh=0):
    nm = len(acc.nrows)
    T = _expect(em, nm, member0, mh)
    pairs, lines, both, shared, lines_a = acc.finish_target_support()
    assert pairs.tolist() == T.pairs[0].tolist()
    assert lines.tolist() == T.lines[0].tolist()
    assert both.tolist() == T.both[0].tolist()
    assert np.array_equal(shared, T.shared[0]) and np.array_equal(lines_a, T.lines_a[0])
    assert np.array_equal(shared, shared.T)
    for a in range(nm):                                        # the rule's invariants
        assert shared[a, a] <= pairs[a] <= lines[a] and both[a] <= pairs[a] and lines_a[a].max() <= lines[a]
        for b in range(nm):
            assert shared[a, b] <= min(pairs[a], pairs[b])
    again = acc.finish_target_support()                        # a second finish: everything was cleared
    assert not any(x.any() for x in again)
    return T


def _geometries(w, e, src, results, eres):
    """(name, launches to make, the add, the model's sides) for a context or the union: SE, PEI from record 0 and from record 1, pairs
    over two batches through hold, and the hand-made pairs"""
    (r1, _), (r2, _) = results
    n1 = w.b1.nrec
    return [
        ("se", [w.b1], dict(a0=0, astep=1, npairs=n1), [(r1, 0, 1)]),
        ("pei0", [w.b1], dict(a0=0, astep=2, npairs=n1 // 2, mate=("same", 1, 2)), [(r1, 0, 2), (r1, 1, 2)]),
        ("pei1", [w.b1], dict(a0=1, astep=2, npairs=(n1 - 1) // 2, mate=("same", 2, 2)), [(r1, 1, 2), (r1, 2, 2)]),
        ("hold", [w.b1, w.b2], dict(a0=4, astep=1, npairs=n1 - 4, mate=("held", 2, 1)), [(r2, 4, 1), (r1, 2, 1)]),
        ("made", [e.b], dict(a0=0, astep=2, npairs=e.b.nrec // 2, mate=("same", 1, 2)), [(eres[0], 0, 2), (eres[0], 1, 2)]),
    ]


def _launch(src, batches, acc):
    is_union = isinstance(src, sk.KmerUnion)
    for i, b in enumerate(batches):
        if is_union:
            src.tally_launch(b, results_stay=True)
        else:
            src.tally_launch(b)
        src.tally_collect_counts()
        if i + 1 < len(batches):
            acc.hold(src)


def _fold(src, acc, geo, member0=0):
    _, batches, add, _ = geo
    _launch(src, batches, acc)
    acc.add(src, add["a0"], add["astep"], add["npairs"], mate=add.get("mate"), member0=member0)


@pytest.mark.parametrize("mh", MINS)
def test_union_of_three(world, extra, mh):  # noqa: F811
    w, u = world, world.union
    nrows = [7] + w.nrows + [9]                                # the union's members are members 1..3 of five
    with sk.CoverageAcc(w.ctxs[0], nrows, mh) as acc:
        acc.set_support(True)
        for geo in _geometries(w, extra, u, w.uni, extra.uni):
            _fold(u, acc, geo, member0=1)
            em = sm.from_records(0, 3, geo[3], geo[2]["npairs"])
            T = _check(acc, em, member0=1, mh=mh)
            assert not T.pairs[0, 0] and not T.pairs[0, 4] and not T.shared[0, 0].any() and not T.shared[0, :, 4].any()
            acc.finish_target()
            if mh == 1000:
                assert not T.pairs.any()
            elif geo[0] != "made":
                assert T.pairs[0, 1] > 0 and T.pairs[0, 3] > 0 and T.lines[0, 1] > T.pairs[0, 1]
            if geo[0] == "made":                               # what the hand-made pairs are there for
                by = {(j, s): (L, parts, tot) for _, j, s, L, parts, tot, _ in em}
                assert by[(1, 0)][1] == 1 and by[(2, 0)][1] == 2 and by[(0, 0)][1] == 3          # through PE1 only, PE2 only, both
                assert by[(0, 0)][1:] == (3, 7) and by[(0, 1)][1:] == (3, 7) and by[(3, 0)][1:] == (1, 2) and by[(0, 0)][0] >= 2
                if mh == 5:
                    assert T.pairs[0, 1] == 3 and T.both[0, 1] == 1                             # pair 0 passes on the sum alone, pair 3 does not pass
                    assert T.shared[0, 1, 2] == 3 and T.shared[0, 1, 1] == 0 < T.pairs[0, 1]    # every pair of strain 0 is strain 1's too
                if mh == 0:
                    assert T.pairs[0, 1] == 4


@pytest.mark.parametrize("mh", MINS)
def test_single_context(world, extra, mh):  # noqa: F811
    w, c = world, world.ctxs[0]
    with sk.CoverageAcc(c, w.nrows[:1], mh) as acc:
        acc.set_support(True)
        for geo in _geometries(w, extra, c, w.single, extra.single):
            _fold(c, acc, geo)
            em = sm.from_records(0, 1, geo[3], geo[2]["npairs"])
            T = _check(acc, em, mh=mh)
            assert T.shared[0, 0, 0] == T.pairs[0, 0] and ((T.pairs[0, 0] > 0) == (mh < 1000))   # alone in its group: every pair is exclusive
            acc.finish_target()


def test_two_runs_back_to_back_without_a_finish_between(world, extra):  # noqa: F811
    """the second fold finds the words and the informative cells zero again: the sums are the model's"""
    w, u, mh = world, world.union, 5
    geos = _geometries(w, extra, u, w.uni, extra.uni)
    with sk.CoverageAcc(w.ctxs[0], w.nrows, mh) as acc:
        acc.set_support(True)
        em = []
        for k, name in enumerate(("hold", "pei1", "se")):
            geo = [g for g in geos if g[0] == name][0]
            _fold(u, acc, geo)
            em += [(0, j + k * 100000, s, L, parts, tot, None) for _, j, s, L, parts, tot, _ in sm.from_records(0, 3, geo[3], geo[2]["npairs"])]
        _check(acc, em, mh=mh)
        acc.finish_target()


def test_support_off(world):  # noqa: F811
    w, c = world, world.ctxs[0]
    with sk.CoverageAcc(c, w.nrows[:1], 0) as acc:
        with pytest.raises(sk.SKError) as ei:
            acc.finish_target_support()
        assert ei.value.code == native.SK_E_STATE
        acc.set_support(True)
        assert not any(x.any() for x in acc.finish_target_support())
        acc.set_support(False)
        with pytest.raises(sk.SKError) as ei:
            acc.finish_target_support()
        assert ei.value.code == native.SK_E_STATE


def test_every_other_result_is_the_same_with_support_on(world, extra):  # noqa: F811
    """finish_target, _regions, _spectrum, _thresholds and rows() over the same feeds with support off and on: the arrays of the two
    states are identical, and (so that both are not wrong alike) the main numbers are the existing model's"""
    w, u, mh = world, world.union, 5
    geos = {g[0]: g for g in _geometries(w, extra, u, w.uni, extra.uni)}
    (r1, h1), (r2, h2) = w.uni
    lst = [0, 3, 5, 40]
    want = [a + b for a, b in zip(model(w.nrows, 3, True, [(r1, h1, w.st1, 0, 2), (r1, h1, w.st1, 1, 2)], w.b1.nrec // 2, mh),
                                  model(w.nrows, 3, True, [(r2, h2, w.st2, 4, 1), (r1, h1, w.st1, 2, 1)], w.b1.nrec - 4, mh))]
    seen = {}
    for on in (False, True):
        out = seen[on] = []
        with sk.CoverageAcc(w.ctxs[0], w.nrows, mh) as acc:
            acc.set_support(on)
            acc.set_spectrum(4)
            acc.set_thresholds(lst)
            for m in range(3):
                acc.set_regions(m, w.ctxs[m], [0, 700, 1500, 2200])
            for finish in ("plain", "regions", "spectrum", "spectrum_regions"):
                _fold(u, acc, geos["pei0"])
                _fold(u, acc, geos["hold"])
                out += [acc.rows(m) for m in range(3)]
                out += list(acc.finish_target_thresholds())
                got = (acc.finish_target() if finish == "plain" else acc.finish_target_regions() if finish == "regions" else
                       acc.finish_target_spectrum(regions=finish == "spectrum_regions"))
                assert got[0].tolist() == [int(np.count_nonzero(d)) for d in want] and got[1].tolist() == [int(d.sum()) for d in want]
                for x in got:
                    out += [y for pair in x for y in pair] if isinstance(x, list) else [x]
                if on:
                    assert acc.finish_target_support()[1].tolist() == got[1].tolist()      # lines = the main table's total
    assert len(seen[False]) == len(seen[True]) > 30
    for a, b in zip(seen[False], seen[True]):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    assert any(len(x) == 5 and np.count_nonzero(x) >= 2 for x in seen[True] if x.ndim == 1)       # region pairs over more than one region


def test_union_of_32_members():
    """SK_UNION_MAX members of a few hundred bases, every fifth row informative, and pairs made by joining a 35-base stretch (five
    k-mers: one of them informative) of every member -- PE1 of members 0..15, PE2 of 16..31: such a pair supports all 32 (32 x 31
    cells of the take's LDS tables each).  Others support member 31 alone (through both mates), and members 0 and 31.  More than 300 sparse records carry
    an informative tally, so more than one workgroup adds into the same cells."""
    rng = random.Random(323232)
    M = native.SK_UNION_MAX
    assert M == 32
    genomes = [_synth.rand_dna(rng, 300 + 7 * i) for i in range(M)]

    def piece(m, n=35):
        a = rng.randrange(len(genomes[m]) - n)
        s = genomes[m][a:a + n]
        return s if rng.random() < 0.5 else _synth.revcomp(s)

    reads = []
    for i in range(60):
        if i % 5 == 0:
            reads += [b"".join(piece(m) for m in range(16)), b"".join(piece(m) for m in range(16, 32))]
        elif i % 5 == 1:
            reads += [piece(31, 60), piece(31, 45)]
        elif i % 5 == 2:
            reads += [piece(0, 60), piece(31, 40)]
        elif i % 5 == 3:
            reads += [_synth.rand_dna(rng, 31), piece((i * 7) % M, 80)]
        else:
            reads += [piece(31, 32), piece(31, 32)]            # two k-mers a mate: a total of 4 does not pass min_kmer_hits = 4 ...
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
        s, st = _stream(reads)
        b = native.TallyBatch(ctxs[0])
        b.fill(s, st)
        u = sk.KmerUnion(ctxs, 0, 2)
        try:
            u.tally_launch(b)
            recs, _ = _union_collect(u, b)
            assert int((recs[:, 2] > 0).sum()) >= 300
            mh = 4
            with sk.CoverageAcc(ctxs[0], [k.nrows for k in sets], mh) as acc:
                acc.set_support(True)
                u.tally_launch(b, results_stay=True)
                u.tally_collect_counts()
                acc.add(u, 0, 2, b.nrec // 2, mate=("same", 1, 2))
                em = sm.from_records(0, M, [(recs, 0, 2), (recs, 1, 2)], b.nrec // 2)
                T = _check(acc, em, mh=mh)
                sh = T.shared[0]
                assert (sh + np.eye(M, dtype=np.uint64) * 100).min() >= 12 and sh[0, 31] >= 20 and sh[31, 31] >= 12 and sh[31, 31] < T.pairs[0, 31]
                assert T.both[0, 31] >= 12 and T.both[0, 0] < T.both[0, 31]
                assert any(tot <= mh for _, _, m, _, _, tot, _ in em if m == 31)      # ... and is no emission
                acc.finish_target()
        finally:
            u.close()
            b.close()
    finally:
        for c in ctxs:
            c.close()
        for k in sets:
            k.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# the program: strain_detect --coverage-support [--support-pairs=FILE] in the job of test_coverage_spectrum_gpu.py
# ---------------------------------------------------------------------------------------------------------------------------------
import gzip  # noqa: E402
import hashlib  # noqa: E402
import json  # noqa: E402
import os  # noqa: E402
import shutil  # noqa: E402
import subprocess  # noqa: E402

import _skt  # noqa: E402
from _sweep_model import class_file  # noqa: E402
from _thresholds_model import main_table  # noqa: E402
from test_coverage_only_gpu import NAME, WENT, _fa  # noqa: E402
from test_coverage_regions_gpu import _base, _run_sd  # noqa: E402
from test_coverage_spectrum_gpu import SMALL_CHUNKS, job  # noqa: E402,F401  (job: the fixture)

SUFFIXES = ("coverage_depth", "coverage_support", "coverage_spectrum", "coverage_regions", "coverage_recurrence", "coverage_recurrence_pairs",
            "coverage_thresholds", "coverage_scrub_sweep", "kmer_hits.gz")
SUP = ["--coverage-support"]
PANEL = (0, 1, 2)


@pytest.fixture(scope="module")
def sjob(job):  # noqa: F811
    """the job's targets (SE .gz with reads shorter than k, PE over two files, PEI), a target without a hit, an odd PEI tail, and a
    target of interleaved pairs that join the informative blocks (1000..1100) of two and of three of the job's strains -- strains 1
    and 2 are identical there, so a read of that block alone supports both; the model's emissions of every strain, computed once"""
    j, r = job, random.Random(78)
    h = j.hit
    some = [_synth.rand_dna(r, 80) for _ in range(30)]
    odd = some[:11] + [h, _synth.revcomp(h), h[20:100]] + some[11:]
    assert len(odd) % 2
    b0, b1, b3 = (j.strains[s][1000:1100] for s in (0, 1, 3))
    join = [b0 + b1, _synth.rand_dna(r, 50), _synth.rand_dna(r, 60), _synth.revcomp(b1 + b0), b0[:70], b1[10:90], b3 + b0, some[0], b1, b0[:20],
            _synth.revcomp(b0), b3[:25]] + some[1:9]
    assert len(join) % 2 == 0
    (j.d / "su_none.fa").write_bytes(_fa([_synth.rand_dna(r, 80) for _ in range(100)]))
    (j.d / "su_odd.fa").write_bytes(_fa(odd))
    (j.d / "su_join.fa").write_bytes(_fa(join))
    j.su_targets = [("SE", f"{j.d}/se.fq.gz"), ("SE", f"{j.d}/su_none.fa"), ("PE", f"{j.d}/pe_1.fa", f"{j.d}/pe_2.fa"), ("PEI", f"{j.d}/il.fq"),
                    ("PEI", f"{j.d}/su_odd.fa"), ("PEI", f"{j.d}/su_join.fa")]
    (j.d / "T6.txt").write_text("".join("\t".join(t) + "\n" for t in j.su_targets))
    for s in range(4):                                       # a class file of two fractions beside every -a list (--coverage-scrub-sweep)
        kms = [ln for ln in gzip.open(j.d / f"s{s}.inf.gz", "rb").read().split(b"\n") if ln and not ln.startswith(b"#")]
        (j.d / f"s{s}.inf.gz.classes").write_bytes(class_file(["0.5", "0.1"], [kms, kms[::2]]))
    j.su_dup = [("SE", f"{j.d}/x/same.fa"), ("SE", f"{j.d}/y/same.fa")]
    j.su_strains = {s: sm.Strain([j.strains[s]], sm.informative_list(str(j.d / f"s{s}.inf.gz"))) for s in range(4)}
    j.su_em = {}
    return j


def _emissions(j, targets, strains):
    """the model's emissions of these strains (numbered in this order) over these targets, each (target list, strain) walked once"""
    out = []
    for t, tg in enumerate(targets):
        for k, s in enumerate(strains):
            key = (tg, s)
            if key not in j.su_em:
                j.su_em[key] = sm.walk(j.su_strains[s], 0, 0, tg[0], *tg[1:])
            out += [(t, jj, k, L, parts, tot, rows) for _, jj, _, L, parts, tot, rows in j.su_em[key]]
    return out


def _sprog(j, tag, flags, strains=(1,), targets="T6.txt", env=None, pairs=False):
    d = j.d / ("sup_" + tag)
    d.mkdir()
    if len(strains) > 1:
        (d / "S.txt").write_text("".join(f"{j.d}/s{s}.fa\t{j.d}/s{s}.inf.gz\t{d}/{NAME % s}\n" for s in strains))
        argv = ["-S", str(d / "S.txt")]
    else:
        s = strains[0]
        argv = ["-r", str(j.d / f"s{s}.fa"), "-a", str(j.d / f"s{s}.inf.gz"), "-o", str(d / (NAME % s))]
    if pairs:
        flags = flags + ["--support-pairs=" + str(d / "pairs.tsv")]
    rc, err, stats = _run_sd(argv + ["-B", str(j.d / targets)] + flags, dict(SMALL_CHUNKS, SK_SD_RESULT_BYTES="1", **(env or {})), d, "run")
    assert rc == 0, err.decode()[-600:]
    out = {}
    for s in strains:
        b = _base(d / (NAME % s))
        out[s] = {x: open(b + "." + x, "rb").read() for x in SUFFIXES if os.path.exists(b + "." + x)}
    out["pairs"] = (d / "pairs.tsv").read_bytes() if (d / "pairs.tsv").exists() else None
    return out, stats, err, open(d / "run.out", "rb").read()


def _want(j, targets, strains, mh=1, group=32):
    em = _emissions(j, targets, strains)
    paths = [t[1] for t in targets]
    T = sm.tables(em, len(targets), len(strains), mh, group=group)
    names = [(NAME % s)[: -len(".kmer_hits.gz")] for s in strains]
    return em, T, {s: sm.support_file(T, paths, k) for k, s in enumerate(strains)}, sm.pairs_file(T, paths, names, group=group)


def _anchored(j, out, targets, strains):
    """the anchor: for every strain the lines the model emits are the hit list the --coverage-depth run wrote (less its '#' trailers)"""
    em, total = _emissions(j, targets, strains), 0
    for k, s in enumerate(strains):
        got = b"".join(ln + b"\n" for ln in gzip.decompress(out[s]["kmer_hits.gz"]).split(b"\n") if ln and not ln.startswith(b"#"))
        mine = b"".join(b"".join(rows) for t, _, kk, _, _, _, rows in sorted(em, key=lambda e: (e[0], e[2], e[1])) if kk == k)
        assert got == mine, s
        total += len(got)
    assert total > 1000


def _lines_are_the_main_tables_totals(out, strains):
    for s in strains:
        mt = main_table(out[s]["coverage_depth"])
        rows = [ln.split(b"\t") for ln in out[s]["coverage_support"].split(b"\n")[1:-1]]
        assert [r[0] for r in rows] == list(mt)                                    # the samples and their order are the main table's
        assert [int(r[3]) for r in rows] == [mt[r[0]][1] for r in rows], s
        assert all(int(r[2]) <= int(r[1]) <= int(r[3]) for r in rows)


def test_program_the_models_lines_are_the_hit_list_and_its_files_the_programs(sjob):
    j = sjob
    em, T, want, want_pairs = _want(j, j.su_targets, PANEL)
    # the anchor: for every strain the lines the model emits are the hit list a --coverage-depth run writes (less its '#' trailers)
    plain, _, perr, pout = _sprog(j, "S_plain_depth", ["--coverage-depth"], strains=PANEL)
    _anchored(j, plain, j.su_targets, PANEL)
    # what the inputs are there for
    by_pair = {}
    for t, jj, k, L, parts, tot, _ in em:
        if tot > 1:
            by_pair.setdefault((t, jj), set()).add(k)
    assert any(len(v) == 3 for v in by_pair.values()) and any(v == {1, 2} for v in by_pair.values()) and any(len(v) == 1 for v in by_pair.values())
    assert T.shared[:, 1, 2].sum() > 0 and T.shared[5, 0, 1] > 0 and T.both[3].sum() > 0 and T.both[0].sum() == 0
    assert T.pairs[1].sum() == 0 and (T.shared[:, 1, 1] < T.pairs[:, 1]).any()
    assert any(len(j.su_em[(tg, 1)]) for tg in j.su_targets[:1]) and want[1].count(b"\n") == 7
    # -S, both tables: the model's two files, byte for byte; lines = the main table's totals
    depth, _, derr, dout = _sprog(j, "S_depth", ["--coverage-depth"] + SUP, strains=PANEL, pairs=True)
    only, stats, oerr, oout = _sprog(j, "S_only", ["--coverage-only"] + SUP, strains=PANEL, pairs=True)
    assert WENT.search(oerr) and stats[0] > 0 and stats[1] > 0 and stats[2] == 0, stats        # folded on the device AND replayed
    for got in (depth, only):
        for s in PANEL:
            assert got[s]["coverage_support"] == want[s], s
            assert got[s]["coverage_depth"] == plain[s]["coverage_depth"]
        assert got["pairs"] == want_pairs
        _lines_are_the_main_tables_totals(got, PANEL)
    # with the flags on, stdout, stderr and the hit lists are the unflagged run's
    assert (dout, derr) == (pout, perr)
    for s in PANEL:
        assert gzip.decompress(depth[s]["kmer_hits.gz"]) == gzip.decompress(plain[s]["kmer_hits.gz"])
    ponly, _, poerr, poout = _sprog(j, "S_plain_only", ["--coverage-only"], strains=PANEL)
    assert (oout, oerr) == (poout, poerr) and all("coverage_support" not in ponly[s] for s in PANEL) and ponly["pairs"] is None
    # -r: one strain, both tables, the default path and an explicit file
    _, _, w1, _ = _want(j, j.su_targets, (1,))
    assert w1[1] == want[1]
    for table in ("--coverage-only", "--coverage-depth"):
        one, st, _, _ = _sprog(j, "r" + table, [table] + SUP)
        if table == "--coverage-depth":
            _anchored(j, one, j.su_targets, (1,))
        assert one[1]["coverage_support"] == want[1]
        _lines_are_the_main_tables_totals(one, (1,))
    expl, _, _, _ = _sprog(j, "r_explicit", ["--coverage-only", "--coverage-support=" + str(j.d / "sup_x.tsv")])
    assert (j.d / "sup_x.tsv").read_bytes() == want[1] and "coverage_support" not in expl[1]


@pytest.mark.parametrize("mh", [0, 30, 1000])
def test_program_min_kmer_hits(sjob, mh):
    j = sjob
    _, T, want, want_pairs = _want(j, j.su_targets, PANEL, mh=mh)
    for table in ("--coverage-only", "--coverage-depth"):
        got, _, _, _ = _sprog(j, "mh%d%s" % (mh, table), [table, "--min-kmer-hits", str(mh)] + SUP, strains=PANEL, pairs=True)
        if table == "--coverage-depth":                                             # (the hit list does not depend on --min-kmer-hits)
            _anchored(j, got, j.su_targets, PANEL)
        for s in PANEL:
            assert got[s]["coverage_support"] == want[s], (table, s)
        assert got["pairs"] == want_pairs
        _lines_are_the_main_tables_totals(got, PANEL)
    assert (T.pairs.sum() == 0) == (mh == 1000)


def test_program_groups_devices_no_union_the_cache_and_the_other_tables(sjob):
    j = sjob
    _, _, want, want_pairs = _want(j, j.su_targets, PANEL)
    _, _, want2, want_pairs2 = _want(j, j.su_targets, PANEL, group=2)
    assert want2 == want and want_pairs2 != want_pairs
    extra = ["--coverage-regions", "--region-window", "500", "--coverage-spectrum", "--spectrum-max", "3", "--coverage-recurrence",
             "--recurrence-pairs", "--coverage-thresholds", "--threshold-list", "0,5,30", "--coverage-scrub-sweep"]
    ref, _, _, _ = _sprog(j, "other", ["--coverage-only"] + extra + ["--panel-share=" + str(j.d / "sup_panel_ref.tsv")], strains=PANEL)
    cache = j.d / "sup_cache"
    cache.mkdir()
    forms = [("dev2", {"SK_DEVICES": "0,0", "SK_SD_GROUP": "2"}, [], want_pairs2), ("group2", {"SK_SD_GROUP": "2"}, [], want_pairs2),
             ("all", {}, extra + ["--panel-share=" + str(j.d / "sup_panel.tsv")], want_pairs), ("cache_fill", {"SK_SD_TIMING": "1"}, ["--target-cache", str(cache)], want_pairs),
             ("cache_served", {"SK_SD_TIMING": "1"}, ["--target-cache", str(cache)], want_pairs)]
    for form, env, flags, wp in forms:
        for table in ("--coverage-only", "--coverage-depth") if form in ("group2", "all") else ("--coverage-only",):
            got, st, err, _ = _sprog(j, form + table, [table] + SUP + flags, strains=PANEL, env=env, pairs=True)
            if table == "--coverage-depth":
                _anchored(j, got, j.su_targets, PANEL)
            if form.startswith("cache"):
                cs = _skt.stats(err)
                assert cs and (cs[1] > 0 and cs[0] == 0 if form == "cache_fill" else cs[0] > 0 and cs[1] == 0), (form, cs)
            for s in PANEL:
                assert got[s]["coverage_support"] == want[s], (form, table, s)
                if form == "all" and table == "--coverage-only":                    # the other tables beside it are what they are without it
                    for x in ("coverage_depth", "coverage_regions", "coverage_spectrum", "coverage_recurrence", "coverage_recurrence_pairs",
                              "coverage_thresholds", "coverage_scrub_sweep"):
                        assert got[s][x] == ref[s][x] and len(ref[s][x]) > 40, x
            if form == "all":
                assert (j.d / "sup_panel.tsv").read_bytes() == (j.d / "sup_panel_ref.tsv").read_bytes()
            assert got["pairs"] == wp, (form, table)
            if table == "--coverage-only":
                assert st[0] > 0 and st[2] == 0
    nou, _, _, _ = _sprog(j, "nounion", ["--coverage-only"] + SUP, strains=PANEL, env={"SK_SD_NO_UNION": "1"})
    for s in PANEL:
        assert nou[s]["coverage_support"] == want[s]


def test_program_two_targets_with_one_basename(sjob):
    """the host path: both targets are one sample, every run is replayed and merged on the host"""
    j = sjob
    _, T, want, want_pairs = _want(j, j.su_dup, PANEL)
    only, stats, err, _ = _sprog(j, "dup_only", ["--coverage-only"] + SUP, strains=PANEL, targets="dup.txt", pairs=True)
    depth, _, _, _ = _sprog(j, "dup_depth", ["--coverage-depth"] + SUP, strains=PANEL, targets="dup.txt", pairs=True)
    assert stats[2] == 2 and stats[0] == 0
    _anchored(j, depth, j.su_dup, PANEL)
    for got in (only, depth):
        for s in PANEL:
            assert got[s]["coverage_support"] == want[s]
        assert got["pairs"] == want_pairs
        _lines_are_the_main_tables_totals(got, PANEL)
    assert want[1].count(b"\n") == 2 and T.pairs[0, 1] > 0 and T.pairs[1, 1] > 0


def _from_hit_list(text, mh=1):
    """{sample: [pairs, both, lines]} of a hit list in which every read has k bases or more: an emission's lines follow each other
    and there are i1 + i2 of them (fields 3 and 5), so the list can be cut back into its emissions"""
    out, lines = {}, [ln.split(b"\t") for ln in text.split(b"\n") if ln and not ln.startswith(b"#")]
    at = 0
    while at < len(lines):
        f = lines[at]
        h1, i1, h2, i2 = (int(x) for x in f[1:5])
        n = i1 + i2
        assert n >= 1 and all(x[:5] == f[:5] for x in lines[at:at + n]) and at + n <= len(lines)
        if h1 + h2 > mh:
            r = out.setdefault(os.path.basename(f[0]), [0, 0, 0])
            r[0] += 1
            r[1] += 1 if i1 and i2 else 0
            r[2] += n
        at += n
    return out


def test_program_fused_with_the_scrub(golden, sjob):
    """kmer_scrub_count -S .. --scrub .. --detect .. --coverage-support --support-pairs=F on the bundled pair: --coverage-depth (every
    run replayed and merged on the host) and --coverage-only (folded on the device) write the same two files, and both are the
    model's.  The two genomes have 6.7 million k-mers each, so the model walks the targets' pairs with the informative lists the job
    itself wrote (67 000 k-mers a strain) -- that finds every emission, its pair, its parts and its lines' k-mers -- and takes each
    emission's h1 + h2 from the hit list --coverage-depth writes, which must hold exactly the walk's lines in the walk's order
    (join_totals).  The per-strain tables are also cut back out of the hit lists alone; the coverage tables are the reference chain's"""
    facts = json.load(open(os.path.join(golden, "pair_workflow_facts.json")))
    b = sjob.d / "sup_bundled_pair"
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
        t = sjob.d / ("sup_pair" + flag)
        t.mkdir()
        base = {n: str(t / os.path.basename(g)[: -len(".fna.gz")]) for n, g in facts["strains"].items()}
        with open(t / "S.txt", "w") as f:
            for n, g in facts["strains"].items():
                f.write("\t".join((g, base[n] + ".scrubbed_kmers", base[n] + ".kmer_hits.gz")) + "\n")
        argv = (["-S", str(t / "S.txt"), "-A", "genomes_to_scrub.txt", "-B", "metagenomes_to_scrub.txt"] + c["kmer_scrub_count"] +
                ["--scrub", facts["min_fraction"], "--detect"] + facts["detect_args"] + [flag, "--coverage-support", "--support-pairs=" + str(t / "pairs.tsv")])
        p = subprocess.run([sk.cli_path()] + argv, cwd=str(b), capture_output=True, env=dict(os.environ, SK_SD_RESULT_BYTES="1"))
        assert p.returncode == 0, p.stderr.decode()[-800:]
        for n in base:
            assert hashlib.md5(open(base[n] + ".coverage_depth", "rb").read()).hexdigest() == c["strains"][n]["coverage_md5"], (flag, n)
        got[flag] = ({n: open(base[n] + ".coverage_support", "rb").read() for n in base}, (t / "pairs.tsv").read_bytes())
        if flag == "--coverage-depth":
            for n in base:
                rows = {r[0]: [int(x) for x in r[1:]] for r in (ln.split(b"\t") for ln in got[flag][0][n].split(b"\n")[1:-1])}
                cut = _from_hit_list(gzip.open(base[n] + ".kmer_hits.gz", "rb").read())
                assert {k: v for k, v in rows.items() if v[0]} == cut and len(cut) >= 1, n
        else:
            went = WENT.search(p.stderr)
            assert went and int(went.group(1)) >= 2
    assert got["--coverage-depth"] == got["--coverage-only"]
    assert got["--coverage-only"][1].count(b"\n") >= 2 + 2 * 2
    targets = [ln.split("\t") for ln in open(b / "target_metagenomes.txt").read().split("\n") if ln]
    t = sjob.d / "sup_pair--coverage-depth"
    em = []
    for k, (n, g) in enumerate(facts["strains"].items()):
        base = str(t / os.path.basename(g)[: -len(".fna.gz")])
        io = sm.InformativeOnly(sm.informative_list(base + ".scrubbed_kmers"))
        mine = []
        for ti, tg in enumerate(targets):
            mine += sm.walk(io, k, ti, tg[0], *[str(b / f) for f in tg[1:]], name=tg[1])
        em += sm.join_totals(mine, gzip.open(base + ".kmer_hits.gz", "rb").read())
    T = sm.tables(em, len(targets), len(facts["strains"]), 1)
    paths = [tg[1] for tg in targets]
    names = [os.path.basename(g)[: -len(".fna.gz")] for g in facts["strains"].values()]
    for k, n in enumerate(facts["strains"]):
        assert got["--coverage-only"][0][n] == sm.support_file(T, paths, k), n
    assert got["--coverage-only"][1] == sm.pairs_file(T, paths, names)
    assert T.pairs.sum() > 100 and T.both.sum() > 0


def test_program_pairs_are_refused_when_a_strain_cannot_join_a_union_table(sjob):
    """a panel whose first strain has an IUPAC letter (byte-string keys: no union table can hold it): --support-pairs is refused after the
    strains are open and before any target is read -- a non-zero status, one line on stderr, no support table, no pairs file, no
    coverage table, no run folded or replayed, and hit lists (--coverage-depth has opened them by then) without a line of a target"""
    j = sjob
    g = j.strains[0]
    (j.d / "s_iupac.fa").write_bytes(b">s0\n%s\n" % (g[:1500] + b"R" + g[1501:]))
    for table in ("--coverage-only", "--coverage-depth"):
        d = j.d / ("sup_refused" + table)
        d.mkdir()
        (d / "S.txt").write_text(f"{j.d}/s_iupac.fa\t{j.d}/s0.inf.gz\t{d}/{NAME % 0}\n" +
                                 "".join(f"{j.d}/s{s}.fa\t{j.d}/s{s}.inf.gz\t{d}/{NAME % s}\n" for s in (1, 2)))
        rc, err, stats = _run_sd(["-S", str(d / "S.txt"), "-B", str(j.d / "T6.txt"), table, "--coverage-support", "--support-pairs=" + str(d / "pairs.tsv")],
                                 dict(SMALL_CHUNKS), d, "run")
        assert rc != 0 and (d / "run.out").read_bytes() == b""
        assert err.count(b"\n") == 1 and err.endswith(b"\n"), err
        assert b"--support-pairs: the strains cannot all be held in union tables" in err
        files = sorted(os.listdir(d))
        assert not [f for f in files if f == "pairs.tsv" or f.endswith((".coverage_support", ".coverage_depth"))], files
        assert tuple(stats) == (0, 0, 0)                                            # no target was read
        if table == "--coverage-only":
            assert files == ["S.txt", "run.err", "run.out"]
        else:
            assert files == sorted(["S.txt", "run.err", "run.out"] + [NAME % s for s in (0, 1, 2)])
            for s in (0, 1, 2):
                raw = (d / (NAME % s)).read_bytes()
                assert raw == b"" or gzip.decompress(raw) == b""
    # the same panel without --support-pairs runs, strain by strain: the per-strain tables of strains 1 and 2 are the model's
    _, _, want, _ = _want(j, j.su_targets, PANEL)
    d = j.d / "sup_iupac_ok"
    d.mkdir()
    (d / "S.txt").write_text(f"{j.d}/s_iupac.fa\t{j.d}/s0.inf.gz\t{d}/{NAME % 0}\n" +
                             "".join(f"{j.d}/s{s}.fa\t{j.d}/s{s}.inf.gz\t{d}/{NAME % s}\n" for s in (1, 2)))
    rc, err, _ = _run_sd(["-S", str(d / "S.txt"), "-B", str(j.d / "T6.txt"), "--coverage-only", "--coverage-support"], dict(SMALL_CHUNKS), d, "run")
    assert rc == 0, err.decode()[-600:]
    for s in (1, 2):
        assert open(_base(d / (NAME % s)) + ".coverage_support", "rb").read() == want[s]
