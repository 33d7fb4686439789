"""Recurrence on the device (include/strainer_kmer.h has the rule): the bit-plane engine (sk_recur_*), its feeder from the coverage
accumulator (sk_covacc_set_recurrence / sk_covacc_mark_target) and the hit-list form (sk_distinct_recurrence), all against
tests/_recurrence_model.py; every comparison is exact.

Engine: members of 0, 1, 63, 64, 65, 4097 and 70 001 bits sit in one object (word edges, a member that shares no word with its
neighbour, a member of more than one workgroup's words); T = 1, 2, 63, 64, 65, 256 with the pair table (64 and 65 cross the gram's
tile), 257 and 4096 with the histogram alone (at 4096 the patterns that set a bit in every plane use the counter's thirteenth carry
plane and bin T)."""
import gzip
import json
import os
import re

import numpy as np
import pytest

import _synth
import strainer2_amd as sk
from _recurrence_model import check_tables, recurrence
from _spectrum_model import read_hits
from strainer2_amd import native
from test_sanitizers import COV_CASES, prepare_cov_case

pytestmark = pytest.mark.gpu

SK_E_ARG = -3
NBITS = [0, 1, 63, 64, 65, 4097, 70001]
BASE = np.concatenate([[0], np.cumsum(NBITS)])
PATTERNS = ["nothing", "everything", "last_bit", "identical", "disjoint", "random_1", "random_50"]


@pytest.fixture(scope="module")
def ctx():
    with sk.KmerContext(0) as c:
        yield c


def _planes(pattern, T, rng):
    n = int(BASE[-1])
    if pattern == "nothing":
        return np.zeros((T, n), dtype=bool)
    if pattern == "everything":
        return np.ones((T, n), dtype=bool)
    if pattern == "last_bit":
        p = np.zeros((T, n), dtype=bool)
        p[T - 1, n - 1] = True
        return p
    if pattern == "identical":
        return np.repeat(rng.random(n)[None, :] < 0.1, T, axis=0)
    if pattern == "disjoint":                                  # column c belongs to plane c % T, and half of them are set
        p = np.zeros((T, n), dtype=bool)
        cols = np.nonzero(rng.random(n) < 0.5)[0]
        p[cols % T, cols] = True
        return p
    if pattern == "random_1":
        p = np.zeros(T * n, dtype=bool)
        p[rng.integers(0, T * n, T * n // 100)] = True
        return p.reshape(T, n)
    return np.unpackbits(np.frombuffer(rng.bytes((T * n + 7) // 8), dtype=np.uint8))[: T * n].astype(bool).reshape(T, n)


def _mark(r, planes):
    for m, nb in enumerate(NBITS):
        sub = planes[:, BASE[m]: BASE[m + 1]]
        for s in np.nonzero(sub.any(axis=1))[0]:
            r.mark_bits(m, int(s), np.nonzero(sub[s])[0])


def _compare(r, planes, pairs):
    got = r.finish(pairs=pairs)
    hist, shared = got if pairs else (got, None)
    for m, nb in enumerate(NBITS):
        wh, ws = recurrence(planes[:, BASE[m]: BASE[m + 1]], pairs)
        assert np.array_equal(hist[m], wh), ("histogram of member", m)
        assert int(hist[m].sum()) == nb
        if pairs:
            assert np.array_equal(shared[m], ws), ("pairs of member", m)
            check_tables(hist[m], shared[m], nb)
    return got


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("T", [1, 2, 63, 64, 65, 256, 257, 4096])
def test_engine_equals_the_model(ctx, T, pattern):
    rng = np.random.default_rng(1000 * T + PATTERNS.index(pattern))
    planes = _planes(pattern, T, rng)
    with sk.Recurrence(ctx, NBITS, T) as r:
        _mark(r, planes)
        hist = _compare(r, planes, T <= sk.SK_RECUR_PAIRS_MAX)
        if T == 4096 and pattern in ("everything", "identical"):
            assert hist[:, T].any()                               # the thirteenth carry plane and bin T


def test_engine_grid_stride_loops_turn(ctx):
    """one member of more words than the histogram's grid has lanes (1024 workgroups x 64), marked with more bits in one call
    than the mark's grid has threads (4096 x 256): both loops turn more than once"""
    rng = np.random.default_rng(9)
    nbits = 64 * (1024 * 64 + 1000) + 5
    planes = np.zeros((3, nbits), dtype=bool)
    with sk.Recurrence(ctx, [nbits], 3) as r:
        for s in range(3):
            bits = np.concatenate([rng.integers(0, nbits, 4096 * 256 + 5000), [nbits - 1, 0]])
            planes[s, bits] = True
            r.mark_bits(0, s, bits)
        hist, shared = r.finish(pairs=True)
    wh, ws = recurrence(planes)
    assert np.array_equal(hist[0], wh) and np.array_equal(shared[0], ws) and wh[3] > 0
    check_tables(hist[0], shared[0], nbits)


def test_engine_refusals(ctx):
    for T in (0, 4097):
        with pytest.raises(sk.SKError) as e:
            sk.Recurrence(ctx, NBITS, T)
        assert e.value.code == SK_E_ARG
    with sk.Recurrence(ctx, NBITS, 257) as r:
        r.mark_bits(5, 256, [7])
        with pytest.raises(sk.SKError) as e:
            r.finish(pairs=True)
        assert e.value.code == SK_E_ARG
        assert r.finish()[5, 1] == 1
    planes = np.zeros((3, int(BASE[-1])), dtype=bool)
    with sk.Recurrence(ctx, NBITS, 3) as r:
        r.mark_bits(6, 2, [0, 70000, 5, 5, 5])                 # duplicates are fine
        planes[2, BASE[6] + np.array([0, 70000, 5])] = True
        r.mark_bits(3, 0, [63])
        planes[0, BASE[3] + 63] = True
        for member, sample, bits in [(3, 0, [1, 64]), (6, 1, [3, 70001, 4]), (0, 0, [0]), (7, 0, [0]), (1, 3, [0]), (1, 0, [0xFFFFFFFF])]:
            with pytest.raises(sk.SKError) as e:
                r.mark_bits(member, sample, bits)              # nothing of a refused call is marked
            assert e.value.code == SK_E_ARG
        first = _compare(r, planes, True)
        r.mark_bits(6, 2, [0, 70000, 5])                       # marking twice changes nothing
        r.mark_bits(3, 0, [63])
        second = _compare(r, planes, True)
        third = r.finish(pairs=True)                           # ... and neither does a finish
        for a, b, c in zip(first, second, third):
            assert np.array_equal(a, b) and np.array_equal(b, c)
        r.mark_bits(1, 1, [0])                                 # more marks after a finish
        planes[1, BASE[1]] = True
        _compare(r, planes, True)


# ---------------------------------------------------------------------------------------------------------------------------------
# sk_covacc_set_recurrence / sk_covacc_mark_target
# ---------------------------------------------------------------------------------------------------------------------------------
class World:
    pass


@pytest.fixture(scope="module")
def world():
    import random
    rng = random.Random(4242)
    w = World()
    w.ctxs, w.sets, w.typ = [], [], []
    for i, n in enumerate([3000, 300, 70000, 40]):             # 70 000 rows: more than 256 blocks of 256, the scan's loop turns twice
        ks = sk.Keyset.from_stream(_synth.rand_dna(rng, n) + b"\n", initial_slots=native.SK_REF_TABLE_SLOTS, default_val=1, incr=0)
        c = sk.KmerContext(0)
        c.load_keyset(ks, 6)
        typ = np.full(ks.nrows, 1, dtype=np.uint32)
        if i != 3:                                             # the last strain has no informative row
            typ[np.array(rng.sample(range(ks.nrows), max(ks.nrows // 7, 1)))] = 2
        typ[0] = 2 if i == 0 else typ[0]
        typ[-1] = 2 if i == 2 else typ[-1]                     # the first and the last row of a member
        c.set_counts(0, typ)
        w.ctxs.append(c)
        w.sets.append(ks)
        w.typ.append(typ)
    w.nrows = [k.nrows for k in w.sets]
    w.inf = [np.nonzero(t == 2)[0] for t in w.typ]
    yield w
    for c in w.ctxs:
        c.close()
    for k in w.sets:
        k.close()


def _acc(w, min_hits=0):
    acc = sk.CoverageAcc(w.ctxs[0], w.nrows, min_hits)
    got = [acc.set_recurrence(m, w.ctxs[m], 0, 2) for m in range(len(w.nrows))]
    assert got == [len(x) for x in w.inf] and got[3] == 0
    return acc, got


def test_ranks_are_the_prefix_count_of_the_type_column(ctx, world):
    """a row's rank is read back through the planes: feeding row i alone sets bit cumsum(informative)[i] - 1"""
    w = world
    acc, nbits = _acc(w)
    T = 3
    with acc, sk.Recurrence(w.ctxs[0], nbits, T) as r:
        # target 0: every informative row of every member, depth 1 + (rank % 3)
        for m, rows in enumerate(w.inf):
            if len(rows):
                acc.add_rows(m, np.repeat(rows, 1 + np.arange(len(rows)) % 3))
        before = [acc.rows(m).copy() for m in range(4)]
        assert acc.mark_target(r, 0) == 0
        for m in range(4):
            assert np.array_equal(acc.rows(m), before[m])      # the counters are untouched by the mark
        uq, tot = acc.finish_target()
        assert uq.tolist() == nbits and tot.tolist() == [int(b.sum()) for b in before]
        hist = r.finish()
        assert [int(h[1]) for h in hist] == nbits and [int(h[0]) for h in hist] == [0, 0, 0, 0]
        # target 1: one informative row per member, chosen by rank; the plane holds exactly that rank
        pick = [len(x) // 2 for x in w.inf]
        for m, rows in enumerate(w.inf):
            if len(rows):
                acc.add_rows(m, [rows[pick[m]], rows[-1]])
        assert acc.mark_target(r, 1) == 0
        acc.finish_target()
        rank = [np.cumsum(t == 2) - 1 for t in w.typ]
        with sk.Recurrence(w.ctxs[0], nbits, T) as want:
            for m, rows in enumerate(w.inf):
                if len(rows):
                    want.mark_bits(m, 0, np.arange(nbits[m]))
                    want.mark_bits(m, 1, [rank[m][rows[pick[m]]], rank[m][rows[-1]]])
                    assert rank[m][rows[-1]] == nbits[m] - 1
            a, b = r.finish(pairs=True), want.finish(pairs=True)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_a_stray_row_is_counted_and_marks_nothing(world):
    w = world
    acc, nbits = _acc(w)
    with acc, sk.Recurrence(w.ctxs[0], nbits, 2) as r:
        other = np.nonzero(w.typ[2] != 2)[0]
        acc.add_rows(2, [other[0], other[0], other[-1], w.inf[2][3]])
        acc.add_rows(3, [0])                                   # a member without an informative row
        assert acc.mark_target(r, 1) == 3
        uq, tot = acc.finish_target()
        assert uq.tolist() == [0, 0, 3, 1] and tot.tolist() == [0, 0, 4, 1]
        hist, shared = r.finish(pairs=True)
        assert hist[2].tolist() == [nbits[2] - 1, 1, 0] and shared[2].tolist() == [[0, 0], [0, 1]]
        assert not hist[3].any() and not shared[3].any()
        assert acc.mark_target(r, 0) == 0                      # the sweep cleared the counters: nothing to mark
        assert np.array_equal(r.finish(), hist)


def test_three_targets_give_the_models_tables(world):
    w = world
    rng = np.random.default_rng(5)
    acc, nbits = _acc(w)
    T = 3
    planes = [np.zeros((T, n), dtype=bool) for n in nbits]
    with acc, sk.Recurrence(w.ctxs[0], nbits, T) as r:
        for t in range(T):
            want_uq = []
            for m, rows in enumerate(w.inf):
                seen = np.nonzero(rng.random(len(rows)) < [0.5, 0.9, 0.02][t])[0]
                if t == 2 and m == 1:
                    seen = seen[:0]                            # a target without a hit on this member
                planes[m][t, seen] = True
                want_uq.append(len(seen))
                if len(seen):
                    acc.add_rows(m, np.repeat(rows[seen], rng.integers(1, 4, len(seen))))
            assert acc.mark_target(r, t) == 0
            uq, _ = acc.finish_target()
            assert uq.tolist() == want_uq
        hist, shared = r.finish(pairs=True)
        for m in range(4):
            wh, ws = recurrence(planes[m])
            assert np.array_equal(hist[m], wh) and np.array_equal(shared[m], ws)
            check_tables(hist[m], shared[m], nbits[m])


def test_mark_target_refusals(world):
    w = world
    acc, nbits = _acc(w)
    with acc:
        with sk.Recurrence(w.ctxs[0], nbits[:3], 2) as r, pytest.raises(sk.SKError) as e:
            acc.mark_target(r, 0)                              # other members
        assert e.value.code == SK_E_ARG
        with sk.Recurrence(w.ctxs[0], [nbits[0] + 1] + nbits[1:], 2) as r, pytest.raises(sk.SKError) as e:
            acc.mark_target(r, 0)                              # another nbits than set_recurrence returned
        assert e.value.code == SK_E_ARG
        with sk.Recurrence(w.ctxs[0], nbits, 2) as r, pytest.raises(sk.SKError) as e:
            acc.mark_target(r, 2)                              # a sample the planes do not have
        assert e.value.code == SK_E_ARG
        with pytest.raises(sk.SKError) as e:
            acc.set_recurrence(1, w.ctxs[0], 0, 2)             # another table's rows
        assert e.value.code == SK_E_ARG


# ---------------------------------------------------------------------------------------------------------------------------------
# sk_distinct_recurrence
# ---------------------------------------------------------------------------------------------------------------------------------
def _distinct_model(keys, sample, T):
    keys, sample = np.asarray(keys, dtype=np.uint64), np.asarray(sample, dtype=np.int64)
    uniq, col = np.unique(keys, return_inverse=True)
    planes = np.zeros((T, len(uniq)), dtype=bool)
    planes[sample, col] = True
    hist, shared = recurrence(planes)
    hist[0] = 0
    return hist, shared


def _distinct_check(ctx, keys, sample, T, pairs=True):
    wh, ws = _distinct_model(keys, sample, T)
    if pairs:
        hist, shared = ctx.distinct_recurrence(keys, sample, T, pairs=True)
        assert np.array_equal(shared, ws)
        check_tables(hist, shared)
    hist = ctx.distinct_recurrence(keys, sample, T)
    assert np.array_equal(hist, wh)
    return hist


def test_distinct_recurrence(ctx):
    rng = np.random.default_rng(78)
    assert not ctx.distinct_recurrence([], [], 3).any()                                # n = 0
    _distinct_check(ctx, rng.integers(0, 40, 500), np.zeros(500), 1)                   # one sample
    T = 256
    keys = np.concatenate([np.full(T, 99, dtype=np.uint64), rng.integers(0, 3000, 20000).astype(np.uint64) + (1 << 40)])
    smp = np.concatenate([np.arange(T), rng.integers(0, T, 20000)])
    order = rng.permutation(len(keys))
    hist = _distinct_check(ctx, keys[order], smp[order], T)                            # one key appears in all of 256 samples
    assert hist[T] == 1
    smp = rng.integers(0, 300, 5000)
    _distinct_check(ctx, rng.integers(0, 2 ** 62, 5000, dtype=np.uint64) >> (smp % 50).astype(np.uint64), smp, 300, pairs=False)
    for bad in [dict(keys=[1], sample=[0], nsamples=0), dict(keys=[1], sample=[0], nsamples=4097), dict(keys=[1, 2], sample=[0, 3], nsamples=3),
                dict(keys=[2 ** 64 - 1], sample=[0], nsamples=1), dict(keys=[1], sample=[0], nsamples=257, pairs=True)]:
        with pytest.raises(sk.SKError) as e:
            ctx.distinct_recurrence(**bad)
        assert e.value.code == SK_E_ARG


@pytest.mark.parametrize("name", sorted(set(os.listdir(COV_CASES)) - {"general_text", "short_line", "zero_informative"}))
def test_distinct_recurrence_on_the_golden_hit_lists(ctx, name):
    d = os.path.join(COV_CASES, name)
    prepare_cov_case(name, d)
    argv = json.load(open(os.path.join(d, "case.json")))["argv"]
    m = 1
    for flag in ("-m", "--min_kmer_hits"):
        if flag in argv:
            m = int(argv[argv.index(flag) + 1])
    order, depth, _ = read_hits(gzip.open(os.path.join(d, argv[argv.index("-k") + 1]), "rb").read(), m)
    ids = {k: i for i, k in enumerate(sorted({k for s in depth for k in depth[s]}))}
    keys, smp = [], []
    for i, s in enumerate(order):
        for k, n in depth.get(s, {}).items():
            keys += [ids[k] * 7919 + 5] * n                     # every line of the list, as the program hands them in
            smp += [i] * n
    if not order:
        return
    _distinct_check(ctx, keys, smp, len(order))


# ---------------------------------------------------------------------------------------------------------------------------------
# the programs: the job of test_coverage_spectrum_gpu.py (SE .gz with reads shorter than k -- so runs are replayed on the host and
# reach the counters through add_rows --, PE over two files, PEI) and a fourth target without a hit
# ---------------------------------------------------------------------------------------------------------------------------------
import hashlib  # noqa: E402
import random  # noqa: E402
import shutil  # noqa: E402
import subprocess  # noqa: E402

from _recurrence_model import HIST_HEADER, PAIRS_HEADER, tables_from_hits  # noqa: E402
from _spectrum_model import main_table, table_from_hits  # noqa: E402
from test_coverage_only_gpu import NAME, WENT, _fa  # noqa: E402
from test_coverage_regions_gpu import _base, _run_sd  # noqa: E402
from test_coverage_spectrum_gpu import SMALL_CHUNKS, job  # noqa: E402,F401  (job: the fixture)

REC = ["--coverage-recurrence", "--recurrence-pairs"]
SUFFIXES = ("coverage_depth", "coverage_spectrum", "coverage_regions", "coverage_recurrence", "coverage_recurrence_pairs", "kmer_hits.gz")


@pytest.fixture(scope="module")
def rjob(job):  # noqa: F811
    r = random.Random(99)
    (job.d / "none.fa").write_bytes(_fa([_synth.rand_dna(r, 80) for _ in range(200)]))
    (job.d / "T4.txt").write_text(f"SE\t{job.d}/se.fq.gz\nSE\t{job.d}/none.fa\nPE\t{job.d}/pe_1.fa\t{job.d}/pe_2.fa\nPEI\t{job.d}/il.fq\n")
    return job


def _prog(job, tag, flags, strains=(1,), targets="T4.txt", env=None):  # noqa: F811
    d = job.d / ("rec_" + tag)
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


def _parse(hist_table, pairs_table):
    h = [ln.split(b"\t") for ln in hist_table.split(b"\n")[1:-1]]
    p = [ln.split(b"\t") for ln in pairs_table.split(b"\n")[1:-1]]
    return {int(f[2]): int(f[3]) for f in h}, {(f[1], f[2]): (int(f[3]), int(f[4])) for f in p}


def _check_against_main(hist_table, pairs_table, coverage_table):
    """the diagonal equals the main table's unique column, in its order, and sum of m * n[m] its sum"""
    n, sh = _parse(hist_table, pairs_table)
    mt = main_table(coverage_table)
    assert [a for (a, b) in sh if a == b] == list(mt)
    for s, (uq, _) in mt.items():
        assert sh[(s, s)] == (max(uq, 0), max(uq, 0))
    assert sum(m * c for m, c in n.items()) == sum(max(uq, 0) for uq, _ in mt.values())
    for (a, b), (both, either) in sh.items():
        assert both <= min(sh[(a, a)][0], sh[(b, b)][0]) and either == sh[(a, a)][0] + sh[(b, b)][0] - both


def test_program_every_form_gives_the_models_tables(rjob):
    plain, _, _, _ = _prog(rjob, "plain_depth", ["--coverage-depth"])                      # a -o run without the flags: the model's input
    hits = str(rjob.d / "rec_plain_depth" / (NAME % 1))
    want = tables_from_hits(gzip.decompress(plain[1]["kmer_hits.gz"]), hits, 1)
    assert want[0].count(b"\n") >= 4 and want[1].count(b"\n") == 1 + 10                   # four samples: ten pairs
    n, sh = _parse(*want)
    assert sh[(b"none.fa", b"none.fa")] == (0, 0) and sh[(b"se.fq.gz", b"pe_1.fa")][0] > 0 and n[0] > 0
    only, stats, err, _ = _prog(rjob, "only", ["--coverage-only"] + REC)
    went = WENT.search(err)
    assert went and stats[0] > 0 and stats[1] > 0 and stats[2] == 0, stats                # folded on the device AND replayed
    depth, _, _, _ = _prog(rjob, "depth", ["--coverage-depth"] + REC)
    for got in (only, depth):
        assert (got[1]["coverage_recurrence"], got[1]["coverage_recurrence_pairs"]) == want
        assert got[1]["coverage_depth"] == plain[1]["coverage_depth"]
    assert "kmer_hits.gz" not in only[1] and gzip.decompress(depth[1]["kmer_hits.gz"]) == gzip.decompress(plain[1]["kmer_hits.gz"])
    _check_against_main(want[0], want[1], plain[1]["coverage_depth"])
    # coverage_depth --recurrence on the -o list of the same job
    o1, o2 = rjob.d / "cd_rec.tsv", rjob.d / "cd_pairs.tsv"
    p = subprocess.run([sk.cli_path("coverage_depth"), "-k", hits, "--recurrence=" + str(o1), "--recurrence-pairs=" + str(o2)], capture_output=True)
    assert (p.returncode, p.stdout) == (0, plain[1]["coverage_depth"]), p.stderr.decode()[-400:]
    assert (o1.read_bytes(), o2.read_bytes()) == want
    # the histogram alone; explicit file names; the default paths of coverage_depth
    alone, _, _, _ = _prog(rjob, "alone", ["--coverage-only", "--coverage-recurrence=" + str(rjob.d / "x.tsv")])
    assert (rjob.d / "x.tsv").read_bytes() == want[0] and "coverage_recurrence" not in alone[1] and "coverage_recurrence_pairs" not in alone[1]
    shutil.copy(hits, rjob.d / "copy.kmer_hits.gz")
    p = subprocess.run([sk.cli_path("coverage_depth"), "-k", "copy.kmer_hits.gz", "--recurrence", "--recurrence-pairs"], cwd=rjob.d, capture_output=True)
    assert p.returncode == 0
    name = tables_from_hits(gzip.decompress(plain[1]["kmer_hits.gz"]), "copy.kmer_hits.gz", 1)
    assert ((rjob.d / "copy.coverage_recurrence").read_bytes(), (rjob.d / "copy.coverage_recurrence_pairs").read_bytes()) == name


def test_program_many_strains_unions_devices_and_the_other_tables(rjob):
    md, _, _, _ = _prog(rjob, "S_plain", ["--coverage-depth"], strains=(0, 1, 2))
    want = {s: tables_from_hits(gzip.decompress(md[s]["kmer_hits.gz"]), str(rjob.d / "rec_S_plain" / (NAME % s)), 1) for s in (0, 1, 2)}
    assert want[1] != want[2]                                                            # (the related strain)
    extra = ["--coverage-regions", "--region-window", "500", "--coverage-spectrum", "--spectrum-max", "3"]
    ref, _, _, _ = _prog(rjob, "S_other", ["--coverage-only"] + extra, strains=(0, 1, 2))
    for form, env, flags in (("S", {}, []), ("dev2", {"SK_DEVICES": "0,0", "SK_SD_GROUP": "2"}, []), ("nounion", {"SK_SD_NO_UNION": "1"}, []),
                             ("S_all", {}, extra)):
        for table in ("--coverage-only", "--coverage-depth") if form == "S" else ("--coverage-only",):
            many, st, _, _ = _prog(rjob, form + table, [table] + REC + flags, strains=(0, 1, 2), env=env)
            for s in (0, 1, 2):
                assert (many[s]["coverage_recurrence"], many[s]["coverage_recurrence_pairs"]) == want[s], (form, table, s)
                assert many[s]["coverage_depth"] == md[s]["coverage_depth"]
                _check_against_main(want[s][0], want[s][1], md[s]["coverage_depth"])
                if flags:                                                                # the other tables beside it are what they are without it
                    assert many[s]["coverage_regions"] == ref[s]["coverage_regions"] and many[s]["coverage_spectrum"] == ref[s]["coverage_spectrum"]
                    hits = str(rjob.d / "rec_S_plain" / (NAME % s))
                    assert many[s]["coverage_spectrum"] == table_from_hits(gzip.decompress(md[s]["kmer_hits.gz"]), hits, 3, 1)
            if table == "--coverage-only":
                assert st[0] > 0 and st[1] > 0


def test_program_two_targets_with_one_basename(rjob):
    """the host accumulator: both targets are one sample"""
    only, stats, err, _ = _prog(rjob, "dup_only", ["--coverage-only"] + REC, targets="dup.txt")
    depth, _, _, _ = _prog(rjob, "dup_depth", ["--coverage-depth"] + REC, targets="dup.txt")
    assert stats[2] == 2 and stats[0] == 0 and err.count(b"share a file name") == 1
    hits = str(rjob.d / "rec_dup_depth" / (NAME % 1))
    want = tables_from_hits(gzip.decompress(depth[1]["kmer_hits.gz"]), hits, 1)
    for got in (only, depth):
        assert (got[1]["coverage_recurrence"], got[1]["coverage_recurrence_pairs"]) == want
    n, sh = _parse(*want)
    assert list(sh) == [(b"same.fa", b"same.fa")] and set(n) == {0, 1}
    _check_against_main(want[0], want[1], only[1]["coverage_depth"])


def test_program_with_the_flags_off_writes_what_it_wrote(rjob):
    """without the flags nothing of recurrence is written or said, and with them every other output keeps its bytes"""
    extra = ["--coverage-regions", "--region-window", "500", "--coverage-spectrum", "--spectrum-max", "3"]
    for table in ("--coverage-only", "--coverage-depth"):
        a, _, ea, oa = _prog(rjob, "off" + table, [table] + extra, env={"SK_SD_TIMING": "1"})
        b, _, eb, ob = _prog(rjob, "on" + table, [table] + extra + REC)
        assert "coverage_recurrence" not in a[1] and "coverage_recurrence_pairs" not in a[1] and b"recurrence" not in ea
        for x in ("coverage_depth", "coverage_regions", "coverage_spectrum"):
            assert a[1][x] == b[1][x], x
        assert oa == ob
        if table == "--coverage-depth":
            text = gzip.decompress(a[1]["kmer_hits.gz"])
            assert text == gzip.decompress(b[1]["kmer_hits.gz"])
            hits = str(rjob.d / ("rec_off" + table) / (NAME % 1))
            assert a[1]["coverage_spectrum"] == table_from_hits(text, hits, 3, 1)         # the model's, not the code's own
    t, _, et, _ = _prog(rjob, "timing", ["--coverage-only"] + REC, env={"SK_SD_TIMING": "1"})
    assert re.search(rb"recurrence on the device: marks \d+\.\d+ ms \(4 targets\), finish: histogram \d+\.\d+ ms, pairs \d+\.\d+ ms", et)


def test_program_fused_with_the_scrub(golden, rjob):
    """kmer_scrub_count -S .. --scrub .. --detect .. --coverage-recurrence --recurrence-pairs on the bundled pair: both modes write
    the model's tables, computed from the hit lists --coverage-depth writes; the coverage tables are the reference chain's"""
    facts = json.load(open(os.path.join(golden, "pair_workflow_facts.json")))
    b = rjob.d / "rec_bundled_pair"
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
        t = rjob.d / ("rec_pair" + flag)
        t.mkdir()
        base = {n: str(t / os.path.basename(g)[: -len(".fna.gz")]) for n, g in facts["strains"].items()}
        with open(t / "S.txt", "w") as f:
            for n, g in facts["strains"].items():
                f.write("\t".join((g, base[n] + ".scrubbed_kmers", base[n] + ".kmer_hits.gz")) + "\n")
        argv = (["-S", str(t / "S.txt"), "-A", "genomes_to_scrub.txt", "-B", "metagenomes_to_scrub.txt"] + c["kmer_scrub_count"] +
                ["--scrub", facts["min_fraction"], "--detect"] + facts["detect_args"] + [flag] + REC)
        p = subprocess.run([sk.cli_path()] + argv, cwd=str(b), capture_output=True)
        assert p.returncode == 0, p.stderr.decode()[-800:]
        for n in base:
            assert hashlib.md5(open(base[n] + ".coverage_depth", "rb").read()).hexdigest() == c["strains"][n]["coverage_md5"], (flag, n)
        got[flag] = {n: (open(base[n] + ".coverage_recurrence", "rb").read(), open(base[n] + ".coverage_recurrence_pairs", "rb").read()) for n in base}
        if flag == "--coverage-depth":
            for n in base:
                want = tables_from_hits(gzip.open(base[n] + ".kmer_hits.gz", "rb").read(), base[n] + ".kmer_hits.gz", 1)
                assert got[flag][n] == want and want[0].startswith(HIST_HEADER) and want[1].startswith(PAIRS_HEADER) and want[0].count(b"\n") >= 3, n
                _check_against_main(want[0], want[1], open(base[n] + ".coverage_depth", "rb").read())
    assert got["--coverage-depth"] == got["--coverage-only"]


def test_coverage_depth_refuses_general_text(tmp_path):
    d = os.path.join(COV_CASES, "general_text")
    prepare_cov_case("general_text", d)
    argv = json.load(open(os.path.join(d, "case.json")))["argv"]
    out = tmp_path / "r.tsv"
    p = subprocess.run([sk.cli_path("coverage_depth")] + argv + ["--recurrence=" + str(out)], cwd=d, capture_output=True)
    assert p.returncode != 0 and p.stdout == b"" and p.stderr.count(b"\n") == 1 and b"--recurrence" in p.stderr
    assert not out.exists()


def test_program_one_target_on_the_command_line(rjob):
    """a -b run has one sample: T = 1, one pair"""
    tabs = {}
    for tag, flags in (("b_plain", ["--coverage-depth"]), ("b_only", ["--coverage-only"] + REC), ("b_depth", ["--coverage-depth"] + REC)):
        d = rjob.d / ("rec_" + tag)
        d.mkdir()
        o = d / (NAME % 1)
        argv = ["-r", str(rjob.d / "s1.fa"), "-a", str(rjob.d / "s1.inf.gz"), "-o", str(o), "-n", "-b", str(rjob.d / "se.fq.gz")] + flags
        rc, err, _ = _run_sd(argv, dict(SMALL_CHUNKS), d, "run")
        assert rc == 0, err.decode()[-600:]
        tabs[tag] = {x: open(_base(o) + "." + x, "rb").read() for x in SUFFIXES if os.path.exists(_base(o) + "." + x)}
    want = tables_from_hits(gzip.decompress(tabs["b_plain"]["kmer_hits.gz"]), str(rjob.d / "rec_b_plain" / (NAME % 1)), 1)
    for tag in ("b_only", "b_depth"):
        assert (tabs[tag]["coverage_recurrence"], tabs[tag]["coverage_recurrence_pairs"]) == want
        assert tabs[tag]["coverage_depth"] == tabs["b_plain"]["coverage_depth"]
    n, sh = _parse(*want)
    assert set(n) == {0, 1} and list(sh) == [(b"se.fq.gz", b"se.fq.gz")]
