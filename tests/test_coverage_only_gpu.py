"""The coverage accumulator (sk_covacc_*, strainer2_amd.CoverageAcc) against a model.

A tally is launched on a small batch; the expected per-row depth is computed here, in Python, from what the EXISTING collections
(sk_tally_collect_sparse, sk_union_tally_collect) return, under the rule of include/strainer_kmer.h: every informative hit of
either mate of a pair is one line, all lines of a pair carry h1 + h2 (the mates' "all hits"), a line counts iff h1 + h2 >
min_kmer_hits; depth = lines per row, total = their sum, unique = rows with a line.  The same launch is then made again, collected
with the counters-only call (nothing but two numbers comes home) and folded on the device.

World: a strain of 3 kbp with about 1 % of its rows informative, 1,500 reads of 31 to 150 bases (all of k bases or more: the rule's
precondition), about 130 KiB of stream -- four scan tiles of 32 KiB, with a read that hits an informative row laid across the
first tile boundary, reads of exactly 31 bases, and a read that holds one informative 31-mer twice."""
import random

import numpy as np
import pytest

import _synth
import strainer2_amd as sk
from strainer2_amd import native

pytestmark = pytest.mark.gpu

TILE = 1 << 15
ROW_BITS = 27


def _mutate(rng, seq, rate, keep):
    b = bytearray(seq)
    for i in range(len(b)):
        if not (keep[0] <= i < keep[1]) and rng.random() < rate:
            b[i] = rng.choice(b"ACGT")
    return bytes(b)


def _one_read(rng, strains):
    ln = rng.choice([31, 31, 32, 47, 64, 100, 149, 150])
    if rng.random() < 0.6:
        g = strains[rng.randrange(len(strains))]
        a = rng.randrange(len(g) - ln)
        seq = g[a:a + ln]
        if rng.random() < 0.3:
            seq = _mutate(rng, seq, 0.02, (0, 0))
        return _synth.revcomp(seq) if rng.random() < 0.5 else seq
    return _synth.rand_dna(rng, ln)


def _reads(rng, strains, n, straddle, double):
    """n reads; `straddle` starts 75 bytes before the first tile boundary, `double` follows it"""
    recs, off = [], 0
    edge = TILE - 75
    while edge - off > 300:
        recs.append(_one_read(rng, strains))
        off += len(recs[-1]) + 1
    gap = edge - off                                         # 150..300 bytes to fill exactly
    fill = [gap - 1] if gap - 1 <= 150 else [gap // 2 - 1, gap - gap // 2 - 1]
    for ln in fill:
        assert 31 <= ln <= 150
        recs.append(_synth.rand_dna(rng, ln))
        off += ln + 1
    assert off == edge
    recs += [straddle, double]
    while len(recs) < n:
        recs.append(_one_read(rng, strains))
    return recs


def _stream(recs):
    return b"\n".join(recs) + b"\n", np.cumsum([0] + [len(r) + 1 for r in recs[:-1]]).astype(np.uint32)


class World:
    pass


@pytest.fixture(scope="module")
def world():
    rng = random.Random(20261)
    w = World()
    g0 = _synth.rand_dna(rng, 3000)
    W = g0[1500:1531]                                        # the informative 31-mer two strains share
    w.strains = [g0, _mutate(rng, g0, 0.03, (1400, 1600)), _synth.rand_dna(rng, 2800)]
    straddle, double = g0[1420:1570], W + W
    w.recs1 = _reads(rng, w.strains, 1500, straddle, double)
    w.recs2 = _reads(rng, w.strains, 1500, _synth.revcomp(straddle), double)
    assert all(31 <= len(r) <= 150 for r in w.recs1 + w.recs2)
    w.s1, w.st1 = _stream(w.recs1)
    w.s2, w.st2 = _stream(w.recs2)
    assert len(w.s1) > 3 * TILE and len(w.s1) < (1 << 20)
    w.ctxs, w.sets, w.wrow = [], [], []
    for i, g in enumerate(w.strains):
        ks = sk.Keyset.from_stream(g + b"\n", default_val=1, incr=0)
        c = sk.KmerContext(0)
        c.load_keyset(ks, 6)
        typ = np.full(ks.nrows, 2, dtype=np.uint32)         # (all rows informative for a moment: which row is W's?)
        c.set_counts(0, typ)
        _, h = c.tally_batch(W + b"\n", np.zeros(1, dtype=np.uint32), 0, 2)
        typ[:] = 1
        typ[np.array(rng.sample(range(ks.nrows), ks.nrows // 100))] = 2
        if i < 2:
            assert len(h) == 1
            typ[int(h[0, 1])] = 2
            w.wrow.append(int(h[0, 1]))
        else:
            assert len(h) == 0
        c.set_counts(0, typ)
        w.ctxs.append(c)
        w.sets.append(ks)
    w.nrows = [k.nrows for k in w.sets]
    w.b1, w.b2 = native.TallyBatch(w.ctxs[0]), native.TallyBatch(w.ctxs[0])
    w.b1.fill(w.s1, w.st1)
    w.b2.fill(w.s2, w.st2)
    w.union = sk.KmerUnion(w.ctxs, 0, 2)
    # the reference results, once: what the existing collections return for each batch, from a context and from the union
    w.single, w.uni = [], []
    for b in (w.b1, w.b2):
        w.ctxs[0].tally_launch(b)
        recs, hits, nh = w.ctxs[0].tally_collect_sparse()
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


def _union_collect(u, b):
    import ctypes as C
    n = len(u._members)
    cap = u._inflight[1]
    recs = np.zeros((b.nrec * n + 1, 3), dtype=np.uint32)
    hits = np.zeros((cap, 2), dtype=np.uint32)
    nr, nh = C.c_uint64(0), C.c_uint64(0)
    u._uck(sk.lib.sk_union_tally_collect(u._h, recs.ctypes.data, b.nrec * n, C.byref(nr), hits.ctypes.data, C.byref(nh)))
    assert nh.value <= cap
    return recs[: nr.value].copy(), hits[: nh.value].copy()


def _pair(rec, r0, step, npairs):
    if rec < r0 or (rec - r0) % step:
        return None
    j = (rec - r0) // step
    return j if j < npairs else None


def model(nrows, ns, is_union, sides, npairs, min_hits):
    """sides: (recs, hits, starts, r0, step) per mate -> per-member depth arrays"""
    tot = np.zeros((npairs, ns), dtype=np.int64)
    for recs, _, _, r0, step in sides:
        for key, al, _ in recs.tolist():
            j = _pair(key // ns, r0, step, npairs)
            if j is not None:
                tot[j, key % ns] += al
    depth = [np.zeros(n, dtype=np.uint32) for n in nrows]
    for _, hits, starts, r0, step in sides:
        rec_of = np.searchsorted(starts, hits[:, 0], side="right") - 1
        for (pos, row), rec in zip(hits.tolist(), rec_of.tolist()):
            m, row = (row >> ROW_BITS, row & ((1 << ROW_BITS) - 1)) if is_union else (0, row)
            j = _pair(rec, r0, step, npairs)
            if j is not None and tot[j, m] > min_hits:
                depth[m][row] += 1
    return depth


def _max_all(*results):
    return max(int(r[0][:, 1].max()) for r in results)


def _check(acc, want, member0=0):
    for m, d in enumerate(want):
        assert np.array_equal(acc.rows(member0 + m), d), ("rows of member", member0 + m)
    uq, tot = acc.finish_target()
    for m in range(len(acc.nrows)):
        d = want[m - member0] if member0 <= m < member0 + len(want) else np.zeros(1, dtype=np.uint32)
        assert (int(uq[m]), int(tot[m])) == (int(np.count_nonzero(d)), int(d.sum())), ("member", m)
    uq2, tot2 = acc.finish_target()                          # a second finish: everything was cleared
    assert not uq2.any() and not tot2.any()
    for m in range(len(acc.nrows)):
        assert not acc.rows(m).any()
    return uq, tot


def _sorted(recs, hits):
    return recs[np.lexsort((recs[:, 2], recs[:, 1], recs[:, 0]))], hits[np.lexsort((hits[:, 1], hits[:, 0]))]


def test_world_has_the_cases_it_claims(world):
    w = world
    recs, hits = w.single[0]
    rec_of = np.searchsorted(w.st1, hits[:, 0], side="right") - 1
    ends = np.append(w.st1[1:], len(w.s1))
    across = (w.st1[rec_of] < TILE) & (ends[rec_of] > TILE) & (hits[:, 0] > TILE)
    assert across.any(), "an informative hit of a record that lies across the first tile boundary"
    d = model(w.nrows[:1], 1, False, [(recs, hits, w.st1, 0, 1)], len(w.st1), 0)[0]
    assert d[w.wrow[0]] >= 3 and d.max() >= 2                # (straddle once, the double read twice)
    dbl = int(np.searchsorted(w.st1, TILE - 75)) + 1          # (the read behind the one that starts 75 bytes before the boundary)
    assert w.recs1[dbl] == w.recs1[dbl][:31] * 2
    assert (hits[rec_of == dbl, 1] == w.wrow[0]).sum() == 2, hits[rec_of == dbl].tolist()     # one row, twice in one read
    lens31 = [i for i, r in enumerate(w.recs1) if len(r) == 31]
    assert len(set(rec_of.tolist()) & set(lens31)) > 0, "a read of exactly 31 bases with an informative hit"
    urecs, uhits = w.uni[0]
    shared = [(int(h[1]) >> ROW_BITS, int(h[1]) & ((1 << ROW_BITS) - 1)) for h in uhits]
    assert (0, w.wrow[0]) in shared and (1, w.wrow[1]) in shared


@pytest.mark.parametrize("min_hits", ["0", "1", "above"])
def test_single_reads(world, min_hits):
    w = world
    recs, hits = w.single[0]
    mh = _max_all(w.single[0]) + 1 if min_hits == "above" else int(min_hits)
    c = w.ctxs[0]
    with sk.CoverageAcc(c, w.nrows[:1], mh) as acc:
        c.tally_launch(w.b1)
        nr, nh = c.tally_collect_counts()
        assert (nr, nh) == (len(recs), len(hits))
        fr, fh = c.tally_fetch_held()                        # what the host's fallback would get: the same results
        a, b = _sorted(fr, fh), _sorted(recs, hits)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        acc.add(c, 0, 1, w.b1.nrec)
        uq, tot = _check(acc, model(w.nrows[:1], 1, False, [(recs, hits, w.st1, 0, 1)], w.b1.nrec, mh))
        if min_hits == "above":
            assert int(uq[0]) == 0 and int(tot[0]) == 0
        else:
            assert int(tot[0]) > int(uq[0]) > 0


@pytest.mark.parametrize("min_hits", [0, 40])
def test_interleaved_pairs_in_one_batch(world, min_hits):
    w = world
    recs, hits = w.single[0]
    c = w.ctxs[0]
    np_ = w.b1.nrec // 2
    with sk.CoverageAcc(c, w.nrows[:1], min_hits) as acc:
        c.tally_launch(w.b1)
        c.tally_collect_counts()
        acc.add(c, 0, 2, np_, mate=("same", 1, 2))
        want = model(w.nrows[:1], 1, False, [(recs, hits, w.st1, 0, 2), (recs, hits, w.st1, 1, 2)], np_, min_hits)
        _check(acc, want)
        # a run that starts in the middle of the batch (a chunk whose first pair was completed by the chunk before)
        c.tally_launch(w.b1)
        c.tally_collect_counts()
        acc.add(c, 11, 2, np_ - 6, mate=("same", 12, 2))
        want = model(w.nrows[:1], 1, False, [(recs, hits, w.st1, 11, 2), (recs, hits, w.st1, 12, 2)], np_ - 6, min_hits)
        _check(acc, want)


@pytest.mark.parametrize("min_hits", [0, 1, 40])
def test_pairs_over_two_batches(world, min_hits):
    w = world
    (r1, h1), (r2, h2) = w.single
    c = w.ctxs[0]
    with sk.CoverageAcc(c, w.nrows[:1], min_hits) as acc:
        c.tally_launch(w.b1)
        c.tally_collect_counts()
        acc.hold(c)
        c.tally_launch(w.b2)                                 # (overwrites the context's buffers: the accumulator has its copy)
        c.tally_collect_counts()
        n = w.b1.nrec - 4
        acc.add(c, 4, 1, n, mate=("held", 2, 1))             # PE2 = this launch from record 4, PE1 = the held one from record 2
        want = model(w.nrows[:1], 1, False, [(r2, h2, w.st2, 4, 1), (r1, h1, w.st1, 2, 1)], n, min_hits)
        _check(acc, want)
        with pytest.raises(sk.SKError):
            acc.add(c, 0, 1, 1, mate=("held", 0, 1))         # the held launch was used up


@pytest.mark.parametrize("form", ["se", "pei", "pe"])
@pytest.mark.parametrize("min_hits", ["0", "1", "above"])
def test_union_of_three(world, form, min_hits):
    w = world
    u = w.union
    (r1, h1), (r2, h2) = w.uni
    mh = _max_all(*w.uni) * 2 + 1 if min_hits == "above" else int(min_hits)
    nrows = [7] + w.nrows + [9]                              # the union's members are members 1..3 of five
    with sk.CoverageAcc(w.ctxs[0], nrows, mh) as acc:
        u.tally_launch(w.b1, results_stay=True)              # (nothing but the counters travels home with this launch)
        nr, nh = u.tally_collect_counts()
        assert (nr, nh) == (len(r1), len(h1))
        fr, fh = u.tally_fetch_held()
        a, b = _sorted(fr, fh), _sorted(r1, h1)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        if form == "se":
            acc.add(u, 0, 1, w.b1.nrec, member0=1)
            sides, n = [(r1, h1, w.st1, 0, 1)], w.b1.nrec
        elif form == "pei":
            n = w.b1.nrec // 2
            acc.add(u, 0, 2, n, mate=("same", 1, 2), member0=1)
            sides = [(r1, h1, w.st1, 0, 2), (r1, h1, w.st1, 1, 2)]
        else:
            acc.hold(u)
            u.tally_launch(w.b2, results_stay=(min_hits != "1"))
            u.tally_collect_counts()
            n = w.b2.nrec
            acc.add(u, 0, 1, n, mate=("held", 0, 1), member0=1)
            sides = [(r2, h2, w.st2, 0, 1), (r1, h1, w.st1, 0, 1)]
        want = model(w.nrows, 3, True, sides, n, mh)
        uq, tot = _check(acc, want, member0=1)
        assert int(uq[0]) == 0 and int(uq[4]) == 0
        if min_hits == "above":
            assert not uq.any() and not tot.any()
        else:
            assert want[0][w.wrow[0]] >= 3 and want[1][w.wrow[1]] >= 3      # the shared informative k-mer counts for both
            assert int(tot[1]) > 0 and int(tot[2]) > 0


def test_ordinary_collect_after_a_launch_whose_results_stay(world):
    w = world
    u = w.union
    for stay in (True, False, True):
        u.tally_launch(w.b1, results_stay=stay)
        a, b = _sorted(*_union_collect(u, w.b1)), _sorted(*w.uni[0])
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), stay


def test_rows_from_the_host_and_bad_calls(world):
    w = world
    c = w.ctxs[0]
    with sk.CoverageAcc(c, w.nrows, 0) as acc:
        acc.add_rows(1, [5, 5, 7])
        acc.add_rows(2, [0, w.nrows[2] - 1])
        acc.add_rows(0, [])
        assert acc.rows(1)[5] == 2 and acc.rows(1)[7] == 1
        uq, tot = acc.finish_target()
        assert uq.tolist() == [0, 2, 2] and tot.tolist() == [0, 3, 2]
        with pytest.raises(sk.SKError):
            acc.add_rows(1, [w.nrows[1]])                    # no such row
        with pytest.raises(sk.SKError):
            acc.add_rows(3, [0])                             # no such member
        c.tally_launch(w.b1)
        c.tally_collect_counts()
        with pytest.raises(sk.SKError):
            acc.add(c, 0, 1, w.b1.nrec + 1)                  # the run leaves the batch
        with pytest.raises(sk.SKError):
            acc.add(c, 0, 1, 5, member0=3)                   # no such member
        c.tally_launch(w.b1)
        c.tally_collect_sparse()                             # an ordinary collection holds nothing on the device
        with pytest.raises(sk.SKError):
            acc.add(c, 0, 1, 5)
        uq, tot = acc.finish_target()
        assert not uq.any() and not tot.any()


def test_log_overflow_is_refused(world):
    w = world
    c = w.ctxs[0]
    with sk.CoverageAcc(c, w.nrows[:1], 0) as acc:
        c.tally_launch(w.b1, hits_cap=5)
        nr, nh = c.tally_collect_counts()
        assert nh > 5
        with pytest.raises(sk.SKError):
            acc.add(c, 0, 1, w.b1.nrec)
        uq, tot = acc.finish_target()
        assert not uq.any() and not tot.any()


def test_pick_and_fetch_hold_against_the_ordinary_collection(world):
    """sk_covacc_pick: exactly the records and log entries of record 0 and the last three records, from a context's launch, a
    union's, and the launch held; sk_covacc_fetch_hold: the held launch in full."""
    w = world
    for src, ref, ns in ((w.ctxs[0], w.single[0], 1), (w.union, w.uni[0], 3)):
        recs, hits = ref
        rec_of = np.searchsorted(w.st1, hits[:, 0], side="right") - 1
        n = w.b1.nrec
        keep_r = (recs[:, 0] // ns == 0) | (recs[:, 0] // ns >= n - 3)
        keep_h = (rec_of == 0) | (rec_of >= n - 3)
        with sk.CoverageAcc(w.ctxs[0], w.nrows[:ns], 0) as acc:
            src.tally_launch(w.b1)
            src.tally_collect_counts()
            a, b = _sorted(*acc.pick(src, first=True, ntail=3)), _sorted(recs[keep_r], hits[keep_h])
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
            a, b = _sorted(*acc.pick(src, first=False, ntail=n)), _sorted(recs, hits)          # (a tail as long as the batch: everything)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
            a = acc.pick(src, first=True, ntail=3, cap=1, hits_cap=1)                          # (too little room: picked again with what it takes)
            assert len(a[0]) == int(keep_r.sum()) and len(a[1]) == int(keep_h.sum())
            acc.hold(src)
            a, b = _sorted(*acc.fetch_hold()), _sorted(recs, hits)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
            a, b = _sorted(*acc.pick(from_hold=True, first=False, ntail=3)), _sorted(recs[recs[:, 0] // ns >= n - 3], hits[rec_of >= n - 3])
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


# ---------------------------------------------------------------------------------------------------------------------------------
# the program: strain_detect --coverage-only against --coverage-depth of the same test (issue checks 2 to 4)
# ---------------------------------------------------------------------------------------------------------------------------------
import gzip      # noqa: E402
import json      # noqa: E402
import os        # noqa: E402
import subprocess  # noqa: E402

NAME = "Genus_species_st%d.kmer_hits.gz"


def _canon(k):
    r = _synth.revcomp(k)
    return k if k >= r else r


def _fa(reads):
    return b"".join(b">r%d\n%s\n" % (i, x) for i, x in enumerate(reads))


def _fq(reads):
    return b"".join(b"@r%d\n%s\n+\n%s\n" % (i, x, b"I" * len(x)) for i, x in enumerate(reads))


class Job:
    pass


@pytest.fixture(scope="module")
def job(tmp_path_factory):
    """four strains of ~3 kbp (1 and 2 related: 2 % apart), every 97th k-mer informative (~1 %), and reads of 31-150 bases, a third
    of them from the strains; a hit read's neighbours are hit reads often enough for a short read between them to repeat lines"""
    d = tmp_path_factory.mktemp("covonly")
    rng = random.Random(90210)
    j = Job()
    j.d = d
    g1 = _synth.rand_dna(rng, 3000)
    j.strains = [_synth.rand_dna(rng, 3100), g1, _mutate(rng, g1, 0.02, (0, 0)), _synth.rand_dna(rng, 2900)]
    for s, g in enumerate(j.strains):
        (d / f"s{s}.fa").write_bytes(b">s%d\n%s\n" % (s, g))
        kms = sorted({_canon(g[i:i + 31]) for i in range(s, len(g) - 31, 97)} | {_canon(g[i:i + 31]) for i in range(1000, 1060)})
        with gzip.open(d / f"s{s}.inf.gz", "wb") as f:
            f.write(b"#informative\n" + b"\n".join(kms) + b"\n")

    def reads(n, seed):
        r = random.Random(seed)
        out = []
        for _ in range(n):
            ln = r.choice([31, 31, 75, 100, 150, r.randrange(31, 151)])
            if r.random() < 0.35:
                g = j.strains[r.randrange(4)]
                a = r.randrange(900, 1100) if r.random() < 0.5 else r.randrange(0, len(g) - ln)
                rd = g[a:a + ln]
                rd = _synth.revcomp(rd) if r.random() < 0.5 else rd
            else:
                rd = _synth.rand_dna(r, ln)
            out.append(rd)
        return out

    j.reads = reads
    j.hit = j.strains[1][1000:1100]                          # a read with informative hits on strains 1 and 2
    se, p1, p2, il = reads(1200, 1), reads(700, 2), reads(700, 3), reads(800, 4)
    assert all(len(x) >= 31 for x in se + p1 + p2 + il)
    with gzip.open(d / "se.fq.gz", "wb", compresslevel=1) as f:
        f.write(_fq(se))
    (d / "pe_1.fa").write_bytes(_fa(p1))
    (d / "pe_2.fa").write_bytes(_fa(p2))
    (d / "il.fq").write_bytes(_fq(il))
    (d / "clean.txt").write_text(f"SE\t{d}/se.fq.gz\nPE\t{d}/pe_1.fa\t{d}/pe_2.fa\nPEI\t{d}/il.fq\n")
    return j


def _sd(argv, tag, d):
    out, err = str(d / (tag + ".out")), str(d / (tag + ".err"))
    rc = native.run_strain_detect_inprocess(argv, out, err)
    return rc, open(out, "rb").read(), open(err, "rb").read()


def _both(job, tag, targets, strain=1, extra=(), want_rc=0):
    """--coverage-depth and --coverage-only on the same targets: (table, stats, stderr of each); the tables must be the same bytes"""
    d = job.d / tag
    d.mkdir()
    base = ["-r", str(job.d / f"s{strain}.fa"), "-a", str(job.d / f"s{strain}.inf.gz")] + list(targets) + list(extra)
    hits = d / "depth" / (NAME % strain)
    only = d / "only" / (NAME % strain)
    hits.parent.mkdir()
    only.parent.mkdir()
    rc1, out1, err1 = _sd(base + ["-o", str(hits), "--coverage-depth"], "depth", d)
    native.coverage_only_stats(reset=True)
    rc2, out2, err2 = _sd(base + ["-o", str(only), "--coverage-only"], "only", d)
    stats = native.coverage_only_stats(reset=True)
    said = b"".join(ln for ln in err2.splitlines(True) if b"share a file name" not in ln)     # (the one line the flag adds, checked by its test)
    assert (rc1 != 0, out1, err1) == (rc2 != 0, out2, said.replace(str(only).encode(), str(hits).encode()))
    assert (rc1 != 0) == (want_rc != 0), err1.decode()[-500:]
    assert not only.exists(), "no file at the -o path"
    if want_rc:
        return None, stats, err2
    t1 = open(str(hits)[: -len(".kmer_hits.gz")] + ".coverage_depth", "rb").read()
    t2 = open(str(only)[: -len(".kmer_hits.gz")] + ".coverage_depth", "rb").read()
    assert t1 == t2 and t1.count(b"\n") >= 2
    assert sorted(os.listdir(only.parent)) == [(NAME % strain)[: -len(".kmer_hits.gz")] + ".coverage_depth"]
    return t1, stats, err2


@pytest.mark.parametrize("extra", [[], ["--min-kmer-hits", "0"], ["--min-kmer-hits", "40"]])
def test_program_clean_inputs(job, extra):
    """reads of 31 bases or more, SE (.gz FASTQ), PE over two files and PEI: every run is counted on the device"""
    t, (dev, replayed, hostacc), _ = _both(job, "clean" + "".join(extra), ["-B", str(job.d / "clean.txt")], extra=extra)
    assert dev >= 3 and replayed == 0 and hostacc == 0
    rows = [ln.split(b"\t") for ln in t.splitlines()[1:]]
    assert len(rows) == 3 and (extra == ["--min-kmer-hits", "40"] or all(int(r[9]) > int(r[8]) > 0 for r in rows))


@pytest.mark.parametrize("mode,files", [("SE", ["se.fq.gz"]), ("PE", ["pe_1.fa", "pe_2.fa"]), ("PEI", ["il.fq"])])
def test_program_clean_single_target(job, mode, files):
    argv = ["-b", str(job.d / files[0]), "-t", mode] + (["-c", str(job.d / files[1])] if mode == "PE" else [])
    _, (dev, replayed, hostacc), _ = _both(job, "one" + mode, argv)
    assert dev == 1 and replayed == 0 and hostacc == 0


def test_program_bundled_step_3(golden, job):
    """the bundled step 3 (its reads all have 31 bases or more): the table test_bundled_steps_3_and_4 compares against, no replay"""
    from test_sanitizers import COV_CASES
    b = os.path.join(golden, "bundled")
    facts = json.load(open(os.path.join(b, "step3_facts.json")))
    nm = "Bacteroides_ovatus_1001283st1_B8_1001283B150210_160208.kmer_hits.gz"
    d = job.d / "bundled"
    d.mkdir()
    argv = [os.path.join(b, a) if os.path.exists(os.path.join(b, a)) else a for a in facts["argv"]]
    argv[argv.index("-o") + 1] = str(d / nm)
    lst = d / "targets.txt"                                  # (the list's paths are relative to the bundle)
    lst.write_text("".join("\t".join([f[0]] + [os.path.join(b, x) for x in f[1:]]) + "\n"
                           for f in (ln.split("\t") for ln in open(os.path.join(b, "target_metagenomes.txt")).read().splitlines())))
    argv[argv.index("-B") + 1] = str(lst)
    native.coverage_only_stats(reset=True)
    rc, _, err = _sd(argv + ["--coverage-only"], "b", d)
    dev, replayed, hostacc = native.coverage_only_stats(reset=True)
    assert rc == 0, err.decode()[-500:]
    want = open(os.path.join(COV_CASES, "bundled_step4", "expected.stdout"), "rb").read()
    assert open(d / nm.replace(".kmer_hits.gz", ".coverage_depth"), "rb").read() == want
    assert not (d / nm).exists()
    assert dev >= 2 and replayed == 0 and hostacc == 0


@pytest.mark.parametrize("name", ["batch", "cli_pe", "cli_pei", "cli_se", "cli_default", "background"])
def test_program_on_the_goldens_with_short_reads(golden, job, name):
    """the sd_cases goldens (every one of them has reads shorter than 31 bases: all of them replay)"""
    d = os.path.join(golden, "sd_cases", name)
    meta = json.load(open(os.path.join(d, "case.json")))
    tabs = []
    for flag in ("--coverage-depth", "--coverage-only"):
        t = job.d / (name + flag)
        t.mkdir()
        argv = list(meta["argv"])
        argv[argv.index("-o") + 1] = str(t / "Genus_species_st1.kmer_hits.gz")
        p = subprocess.run([sk.cli_path("strain_detect")] + argv + [flag], cwd=d, capture_output=True)
        assert p.returncode == 0, p.stderr.decode()[-500:]
        tabs.append(open(t / "Genus_species_st1.coverage_depth", "rb").read())
        assert (t / "Genus_species_st1.kmer_hits.gz").exists() == (flag == "--coverage-depth")
    assert tabs[0] == tabs[1]


def _short_cases(job):
    h, r = job.hit, job.reads
    a, b = r(40, 11), r(40, 12)
    stale = a[:20] + [h, h[:12], h[10:80]] + a[20:]                    # a short read between two hit reads
    pe1 = a[:10] + [h, h[5:90]] + a[10:]
    pe2 = b[:10] + [_synth.revcomp(h), h[:9]] + b[10:]                 # a short PE2 mate behind a hit pair: it repeats that mate's tallies
    odd = a[:11] + [h, _synth.revcomp(h), h[20:100]]                   # 41 + ... records: an odd count, the last one a hit read
    return {
        "stale": ("SE", [_fa(stale)]),
        "short_mate": ("PE", [_fa(pe1), _fa(pe2)]),
        # (FASTA: behind an odd FASTQ file the reference takes the last length for a mate and fails, as test_program_pe2_ends_early has it)
        "pei_odd": ("PEI", [_fa(odd if len(odd) % 2 else odd + [h])]),
    }


@pytest.mark.parametrize("case", ["stale", "short_mate", "pei_odd"])
def test_program_fallback_inputs(job, case):
    mode, files = _short_cases(job)[case]
    paths = []
    for i, data in enumerate(files):
        paths.append(job.d / f"{case}_{i}.fx")
        paths[-1].write_bytes(data)
    argv = ["-b", str(paths[0]), "-t", mode] + (["-c", str(paths[1])] if mode == "PE" else [])
    t, (dev, replayed, hostacc), _ = _both(job, "fb_" + case, argv)
    assert replayed > 0 and hostacc == 0
    assert int(t.splitlines()[1].split(b"\t")[9]) > 0


def test_program_pe2_ends_early(job):
    """PE2 runs out while PE1 still has reads: the same words on stderr and the same exit status as without the flag"""
    a, b = job.reads(30, 21), job.reads(20, 22)
    (job.d / "early_1.fq").write_bytes(_fq(a[:5] + [job.hit] + a[5:]))         # (FASTQ: behind its last record the parser still holds that record's length)
    (job.d / "early_2.fq").write_bytes(_fq(b))
    _, _, err = _both(job, "early", ["-b", str(job.d / "early_1.fq"), "-c", str(job.d / "early_2.fq"), "-t", "PE"], want_rc=1)
    assert b"reached end of PE2" in err


def test_program_two_targets_with_one_basename(job):
    r = job.reads
    for sub, seed in (("x", 31), ("y", 32)):
        (job.d / sub).mkdir()
        (job.d / sub / "same.fa").write_bytes(_fa(r(60, seed) + [job.hit, _synth.revcomp(job.hit)]))
    (job.d / "dup.txt").write_text(f"SE\t{job.d}/x/same.fa\nSE\t{job.d}/y/same.fa\n")
    t, (dev, replayed, hostacc), err = _both(job, "dup", ["-B", str(job.d / "dup.txt")])
    assert hostacc == 2 and dev == 0
    assert err.count(b"share a file name") == 1
    assert t.count(b"\n") == 2                               # one sample


def _strains_file(job, d, tag):
    (d / tag).mkdir()
    f = d / (tag + ".txt")
    f.write_text("".join(f"{job.d}/s{s}.fa\t{job.d}/s{s}.inf.gz\t{d}/{tag}/{NAME % s}\n" for s in range(4)))
    return str(f)


def _tables(d, tag):
    return [open(d / tag / ((NAME % s)[: -len(".kmer_hits.gz")] + ".coverage_depth"), "rb").read() for s in range(4)]


def test_many_strains(job):
    """-S with four strains (1 and 2 related): union table, strain by strain, and two logical devices"""
    d = job.d / "many"
    d.mkdir()
    exe = sk.cli_path("strain_detect")
    p = subprocess.run([exe, "-S", _strains_file(job, d, "depth"), "-B", str(job.d / "clean.txt"), "--coverage-depth"], capture_output=True)
    assert p.returncode == 0, p.stderr.decode()[-500:]
    want = _tables(d, "depth")
    assert len(set(want)) == 4 and all(t.count(b"\n") == 4 for t in want)
    assert all(int(ln.split(b"\t")[9]) > 0 for ln in want[1].splitlines()[1:] + want[2].splitlines()[1:])
    native.coverage_only_stats(reset=True)
    rc, _, err = _sd(["-S", _strains_file(job, d, "only"), "-B", str(job.d / "clean.txt"), "--coverage-only"], "only", d)
    dev, replayed, hostacc = native.coverage_only_stats(reset=True)
    assert rc == 0, err.decode()[-500:]
    assert _tables(d, "only") == want and (replayed, hostacc) == (0, 0) and dev >= 3
    assert sorted(os.listdir(d / "only")) == sorted((NAME % s)[: -len(".kmer_hits.gz")] + ".coverage_depth" for s in range(4))
    for tag, env in (("nounion", {"SK_SD_NO_UNION": "1"}), ("twodev", {"SK_DEVICES": "0,0", "SK_SD_GROUP": "2"})):
        p = subprocess.run([exe, "-S", _strains_file(job, d, tag), "-B", str(job.d / "clean.txt"), "--coverage-only"], capture_output=True,
                           env=dict(os.environ, **env))
        assert p.returncode == 0, p.stderr.decode()[-500:]
        assert _tables(d, tag) == want, tag
        assert len(os.listdir(d / tag)) == 4


def test_many_strains_fused_with_the_scrub(golden, job):
    """kmer_scrub_count -S .. --scrub .. --detect .. --coverage-only on the bundled pair of strains: the tables of the reference's
    chain (tests/golden/pair_workflow_facts.json), which --coverage-depth writes too; no hit list is created"""
    import hashlib
    import shutil
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
    tabs = {}
    for flag in ("--coverage-depth", "--coverage-only"):
        t = job.d / ("pair" + flag)
        t.mkdir()
        base = {n: str(t / os.path.basename(g)[: -len(".fna.gz")]) for n, g in facts["strains"].items()}
        with open(t / "S.txt", "w") as f:
            for n, g in facts["strains"].items():
                f.write("\t".join((g, base[n] + ".scrubbed_kmers", base[n] + ".kmer_hits.gz")) + "\n")
        argv = (["-S", str(t / "S.txt"), "-A", "genomes_to_scrub.txt", "-B", "metagenomes_to_scrub.txt"] + c["kmer_scrub_count"] +
                ["--scrub", facts["min_fraction"], "--detect"] + facts["detect_args"] + [flag])
        p = subprocess.run([sk.cli_path()] + argv, cwd=str(b), capture_output=True)
        assert p.returncode == 0, p.stderr.decode()[-800:]
        tabs[flag] = {n: open(base[n] + ".coverage_depth", "rb").read() for n in base}
        for n in base:
            assert os.path.exists(base[n] + ".kmer_hits.gz") == (flag == "--coverage-depth"), (flag, n)
            assert hashlib.md5(tabs[flag][n]).hexdigest() == c["strains"][n]["coverage_md5"], (flag, n)
    assert tabs["--coverage-depth"] == tabs["--coverage-only"]


# ---------------------------------------------------------------------------------------------------------------------------------
# many small chunks (SK_SD_CHUNK_BYTES): what one chunk leaves to the next
# ---------------------------------------------------------------------------------------------------------------------------------
import re  # noqa: E402

WENT = re.compile(rb"--coverage-only: (\d+) runs counted on the device, (\d+) replayed")


def _chunk_cases(job):
    h, r = job.hit, job.reads
    hits = [h, _synth.revcomp(h), h[3:97], h[10:100]]
    clean = r(900, 41)
    for i in range(5, 900, 7):                               # (a hit read every seventh: most chunks end near one)
        clean[i] = hits[i % 4]
    se = []
    for i, x in enumerate(r(1200, 42)):                      # blocks of clean reads that end in a hit read, a short read behind each; all
        se.append(x[:100].ljust(100, b"G"))                  # reads have 100 bases, so every chunk holds as many, and 25 reads a block
        if i % 23 == 22:                                     # walk the short read through every place in a chunk: some chunk begins
            se += [hits[i % 2], h[:7 + i % 20]]              # with it, behind a chunk that was counted on the device
    same = [x[:100].ljust(100, b"A") for x in r(700, 43)]    # reads of one length: the two files' chunks line up
    for i in range(3, 700, 5):
        same[i] = hits[i % 4][:100].ljust(100, b"C")
    mates = [_synth.revcomp(x) for x in same]
    return {
        "pei_chunks": ("PEI", [_fa(clean[:899])]),           # 899 records: pairs across chunk boundaries, the last mate missing
        "se_short_first": ("SE", [_fa(se)]),
        "pe_lined_up": ("PE", [_fa(same), _fa(mates)]),
        "pe_not_lined_up": ("PE", [_fa(clean[:700]), _fa(r(700, 44))]),     # other lengths in PE2: its chunks hold other records
    }


@pytest.mark.parametrize("case", ["pei_chunks", "se_short_first", "pe_lined_up", "pe_not_lined_up"])
def test_program_over_many_small_chunks(job, case):
    """chunks of about fifteen reads: interleaved pairs whose mates lie in two chunks (either of which may be counted on the device),
    a short read that opens a chunk behind a counted one and repeats its last read's lines, PE chunks that line up and PE chunks
    that do not (a held PE1 chunk comes home after all) -- the table --coverage-depth writes with the same chunks, and with one
    chunk per file; a strain's replayed rows go to the device one at a time (SK_SD_CO_FLUSH_ROWS=1)"""
    mode, files = _chunk_cases(job)[case]
    d = job.d / ("chunks_" + case)
    d.mkdir()
    paths = []
    for i, data in enumerate(files):
        paths.append(d / f"in_{i}.fa")
        paths[-1].write_bytes(data)
    base = ["-r", str(job.d / "s1.fa"), "-a", str(job.d / "s1.inf.gz"), "-b", str(paths[0]), "-t", mode] + (["-c", str(paths[1])] if mode == "PE" else [])
    tabs, went = {}, {}
    for tag, flag, env in (("depth", "--coverage-depth", {"SK_SD_CHUNK_BYTES": "1500"}),
                           ("only", "--coverage-only", {"SK_SD_CHUNK_BYTES": "1500", "SK_SD_CO_FLUSH_ROWS": "1"}),
                           ("one_chunk", "--coverage-only", {})):
        (d / tag).mkdir()
        p = subprocess.run([sk.cli_path("strain_detect")] + base + ["-o", str(d / tag / (NAME % 1)), flag], capture_output=True,
                           env=dict(os.environ, SK_SD_RESULT_BYTES="1", **env))
        assert p.returncode == 0, p.stderr.decode()[-500:]
        tabs[tag] = open(d / tag / ((NAME % 1)[: -len(".kmer_hits.gz")] + ".coverage_depth"), "rb").read()
        went[tag] = tuple(int(x) for x in WENT.search(p.stderr).groups())
    assert tabs["only"] == tabs["depth"] == tabs["one_chunk"]
    assert int(tabs["only"].splitlines()[1].split(b"\t")[9]) > 50
    dev, replayed = went["only"]
    if case == "pe_not_lined_up":                            # (the held PE1 chunks came home: nearly every run is replayed)
        assert replayed >= 10 and went["one_chunk"] == (1, 0), went
        return
    assert dev >= 10, went                                   # (chunks were counted on the device ...)
    if case != "pe_lined_up":
        assert replayed >= 3, went                           # (... and runs between or behind them replayed)
    else:
        assert replayed == 0 and went["one_chunk"] == (1, 0), went
