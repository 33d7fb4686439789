"""Step 2's ranking on the device (sk_filter.hip) at chosen inputs: the worlds of tests/_rank_worlds.py -- ties across the two columns,
scores one ulp apart, keys that differ in one byte of one radix pass, a score of 1.0, rows of score 0, integers that meet as doubles,
a tie run over the shares of flt_eq_scan's threads -- against the numpy model of the script's stable descending sort; flt_hist around
its LDS / global split; the program against the oracle on the tie world; and the fused route's loader (sk_filter_load_counts) against
sk_filter_load of the same columns.  Every comparison is exact.  tests/test_rank_worlds_host.py proves the worlds."""
import gzip
import os
import random
import subprocess

import numpy as np
import pytest

import _rank_worlds as w
import _synth
import strainer2_amd as sk
from _sweep_model import joint_classes
from strainer2_amd import native

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE_DIR = os.path.join(REPO, "oracle")


def _oracle_bin(name):
    p = os.path.join(ORACLE_DIR, name)
    if not os.path.exists(p):
        subprocess.run(["make", "-C", ORACLE_DIR, name], check=True, stdout=subprocess.DEVNULL)
    return p


@pytest.fixture(scope="module")
def ctx():
    c = sk.KmerContext(0)
    yield c
    c.close()


def _loaded(ctx, world):
    gone = getattr(world, "gone", None)
    if gone is None:
        gone = np.zeros(len(world.pan), dtype=np.uint8)
    f = native.ScrubFilter(ctx)
    f.load(world.pan, world.meta, gone)
    order = w.rank_order(w.score_model(world.pan, world.meta, world.pan_sum, world.meta_sum), gone)
    return f, gone, order


def _check_cuts(f, world, gone, order, cuts, single=()):
    """classes_joint over the cuts, sixteen at a time, and joint at the cuts of `single`"""
    cuts = sorted(int(c) for c in cuts)
    for i in range(0, len(cuts), 16):
        ns = cuts[i:i + 16]
        want, kept = w.classes_from_order(order, gone, ns)
        got, gk = f.classes_joint(world.pan_sum, world.meta_sum, ns)
        assert np.array_equal(got, want), (ns, np.flatnonzero(got != want)[:8].tolist())
        assert np.array_equal(gk, kept)
    for c in single:
        got = f.joint(world.pan_sum, world.meta_sum, int(c))
        want = w.marks_from_order(order, gone, int(c))
        assert np.array_equal(got, want), (c, np.flatnonzero(got != want)[:8].tolist())


def _every_rank(ctx, world):
    f, gone, order = _loaded(ctx, world)
    n = len(order)
    _check_cuts(f, world, gone, order, range(n + 1), single=sorted({0, 1, 2, n // 2, n - 1, n}))
    f.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# the primitive route
# ---------------------------------------------------------------------------------------------------------------------------------
def test_ties_across_the_two_columns(ctx):
    """3k / 3S and k / S are one double: the rows of both forms go in row order (flt_score's division, flt_mark's tie rule)"""
    t = w.tie_world()
    f, gone, order = _loaded(ctx, t)
    cuts = t.inside + t.edge
    _check_cuts(f, t, gone, order, cuts, single=cuts)
    f.close()


def test_scores_one_ulp_apart(ctx):
    """1024 rows, 512 scores one ulp apart, each through either column: a cut at every rank (all eight radix passes; the + 1's carry)"""
    _every_rank(ctx, w.ulp_ladder())


@pytest.mark.parametrize("p", [2, 3, 4, 5, 6, 7])
def test_keys_that_differ_in_one_radix_pass(ctx, p):
    """flt_digit / flt_pick of pass p over all 256 digits, digit 0 and digit 255 among the cuts"""
    _every_rank(ctx, w.digit_ladder(p))


def test_top_nibble_and_exponent_ladders(ctx):
    """passes 1 and 0"""
    _every_rank(ctx, w.nibble_ladder())
    _every_rank(ctx, w.exponent_ladder())


def test_a_score_of_exactly_one(ctx):
    _every_rank(ctx, w.one_world())


def test_integers_that_are_one_double_go_in_row_order(ctx):
    """counts above 2^53 of a sum of 2^63 - 1: the int -> double conversions of flt_score, count and sum"""
    _every_rank(ctx, w.bigint_world())


def test_alive_rows_of_score_zero(ctx):
    """both counts zero or negative: key 1, ranked last, in row order; all participants can go, one more cannot"""
    z = w.zero_world()
    f, gone, order = _loaded(ctx, z)
    n, nz = len(order), int(z.zero.sum())
    cuts = sorted({0, n - nz - 1, n - nz, n - nz + 1, n - nz // 2, n - 2, n - 1, n})
    _check_cuts(f, z, gone, order, cuts, single=cuts)
    all_gone = f.joint(z.pan_sum, z.meta_sum, n)
    assert all_gone.all()
    with pytest.raises(sk.SKError):
        f.joint(z.pan_sum, z.meta_sum, n + 1)
    with pytest.raises(sk.SKError):
        f.classes_joint(z.pan_sum, z.meta_sum, [n, n + 1])
    f.close()
    # nothing but zero rows
    only = w.World(pan=np.array([0, -1, -(1 << 31), 0, 0], dtype=np.int64), meta=np.array([0, 0, -1, -(1 << 31), 0], dtype=np.int64),
                   gone=np.array([0, 0, 0, 0, 1], dtype=np.uint8), pan_sum=1, meta_sum=1)
    f, gone, order = _loaded(ctx, only)
    assert order.tolist() == [0, 1, 2, 3]
    _check_cuts(f, only, gone, order, range(5), single=range(5))
    with pytest.raises(sk.SKError):
        f.joint(1, 1, 5)
    f.close()


def test_a_tie_run_over_the_shares_of_the_scan_threads(ctx):
    """258 chunks: flt_eq_scan's threads own two each (per = 2); the run's rows lie in the shares of threads 0, 1 and 128"""
    e = w.eq_scan_world()
    f, gone, order = _loaded(ctx, e)
    in_chunk1 = int(((e.pan[: 2 * w.FLT_CHUNK] == 500) & (gone[: 2 * w.FLT_CHUNK] == 0)).sum())
    cuts = [e.above + in_chunk1 + 5, e.above + e.run - 1]
    for c in cuts:
        got = f.joint(e.pan_sum, e.meta_sum, c)
        want = w.marks_from_order(order, gone, c)
        assert np.array_equal(got, want), (c, np.flatnonzero(got != want)[:8].tolist())
    assert want[13999] == 1 and want[e.n - 1] == 0               # the whole run but its last row, which is the table's last
    f.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# hist
# ---------------------------------------------------------------------------------------------------------------------------------
def test_hist_around_the_lds_split(ctx):
    """flt_hist keeps bins below 2048 in LDS and adds the others to HBM directly: nbins on both sides, the overflow bin on both sides"""
    pan, meta = w.hist_column(19), w.hist_column(20, top=4200)
    f = native.ScrubFilter(ctx)
    for which, col in ((0, pan), (1, meta)):
        other = np.full(len(col), 7, dtype=np.int64)
        f.load(*((col, other) if which == 0 else (other, col)))
        top = int(col.max())
        for lo in (1, 5, top, top + 1):
            for nbins in (1, 2047, 2048, 2049):
                got = f.hist(which, lo, nbins)
                assert np.array_equal(got, w.hist_model(col, lo, nbins)), (which, lo, nbins)
        for nbins in (2047, 2048, 2049):                         # values exactly at lo + nbins - 1 and at lo + nbins
            assert (col == 1 + nbins - 1).any() and (col == 1 + nbins).any()
    f.load(np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64))
    for nbins in (1, 2047, 2048, 2049):
        assert not f.hist(0, 1, nbins).any() and len(f.hist(1, 1, nbins)) == nbins + 1
    f.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# the program
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("drug,m", w.TABLE_RUNS)
def test_filter_program_on_the_tie_table(tmp_path, drug, m):
    """kmer_scrub_filter on the tie world with its true sums (a balancing row makes them 3S and S) against the oracle"""
    t = w.tie_table(drug=drug)
    path = str(tmp_path / "t.gz")
    with gzip.GzipFile(path, "wb", compresslevel=1, mtime=0) as g:
        g.write(t.text)
    argv = ["-s", path, "-m", repr(m)]
    want = subprocess.run([_oracle_bin("ksf_oracle")] + argv, capture_output=True)
    got = subprocess.run([sk.cli_path("kmer_scrub_filter")] + argv, capture_output=True)
    assert want.returncode == 0 and want.stdout.count(b"\n") > 500
    assert (got.returncode, got.stdout, got.stderr) == (0, want.stdout, want.stderr)


# ---------------------------------------------------------------------------------------------------------------------------------
# the fused route's loader
# ---------------------------------------------------------------------------------------------------------------------------------
SPECIAL = [0, 1, (1 << 31) - 1, 1 << 31, (1 << 32) - 1]


@pytest.mark.parametrize("perm", [True, False])
def test_load_counts_is_load_of_the_printed_columns(perm):
    """sk_filter_load_counts -> sk_counts_rows_to_device_ -> flt_from_u32: the counters as the table prints them (%d of an unsigned:
    2^31 and above are negative and have no share), gathered through the locality permutation where the context has one"""
    g = _synth.rand_dna(random.Random(5), 3000)
    ks = sk.Keyset.from_stream(g + b"\n")
    rng = np.random.default_rng(6)
    with sk.KmerContext(0) as c:
        if perm:
            c.load_keyset(ks, 4)                                 # (skh_keyset_load hands the key set's locality order to sk_table_load_ex)
        else:
            c.load_table(ks.packed(), 4)                         # (sk_table_load: the caller's row order)
        n = c.nrows
        assert n == ks.nrows and 2000 < n < 3000
        cols = {1: rng.choice(SPECIAL + [2, 3, 7, 7], n), 2: rng.choice(SPECIAL + [5, 5, 900], n),
                3: rng.choice([0, 0, 0, 0, 0, 0, 1, 1 << 31], n)}
        for col, v in cols.items():
            v[: len(SPECIAL)] = SPECIAL if col != 3 else [0, 1, 1 << 31, 0, 1]
            cols[col] = v.astype(np.uint32)
            c.set_counts(col, cols[col])
            assert np.array_equal(c.counts(col), cols[col])
            raw = c.dev_download(c.counts_device_ptr() + col * n * 4, n * 4).view(np.uint32)
            assert np.array_equal(np.sort(raw), np.sort(cols[col]))
            assert np.array_equal(raw, cols[col]) != perm        # the device's order is the caller's only without a permutation
        pan, meta, drug = (cols[k].view(np.int32).astype(np.int64) for k in (1, 2, 3))
        assert pan.min() == -(1 << 31) and meta.max() == (1 << 31) - 1
        for drug_col, gone in ((3, (drug > 0).astype(np.uint8)), (-1, np.zeros(n, dtype=np.uint8))):
            a, b = native.ScrubFilter(c), native.ScrubFilter(c)
            a.load_counts(1, 2, drug_col)
            b.load(pan, meta, gone)
            assert a.n == b.n == n
            sums = a.sums()
            ps, ms = int(pan[pan > 0].sum()), int(meta[meta > 0].sum())
            assert sums == b.sums() == (ps, ms, int((pan > 0).sum()), int((meta > 0).sum()), int(gone.sum()))
            for which, col in ((0, pan), (1, meta)):
                for lo, nbins in ((1, 8), (1, 4096), ((1 << 31) - 1, 2)):
                    h = a.hist(which, lo, nbins)
                    assert np.array_equal(h, b.hist(which, lo, nbins)) and np.array_equal(h, w.hist_model(col, lo, nbins))
            for tp, tm in ((0, 0), (2, 5), (1 << 31, 899)):
                want = (gone != 0) | ((pan > 0) & (pan > tp)) | ((meta > 0) & (meta > tm))
                got = a.above(tp, tm)
                assert np.array_equal(got, b.above(tp, tm)) and np.array_equal(got, want.astype(np.uint8))
            score = w.score_model(pan, meta, ps, ms)
            order = w.rank_order(score, gone)
            alive = len(order)
            top = int((score[order] == score[order[0]]).sum())
            assert 4 < top < alive // 2
            cuts = sorted({0, 1, top // 2, top, alive // 3, alive // 2, alive - 1, alive})       # top // 2: inside the first tie run
            for k in cuts:
                got = a.joint(ps, ms, k)
                assert np.array_equal(got, b.joint(ps, ms, k)) and np.array_equal(got, w.marks_from_order(order, gone, k)), k
            got, kept = a.classes_joint(ps, ms, cuts)
            ref, rkept = b.classes_joint(ps, ms, cuts)
            want, wkept, wps, wms = joint_classes(pan, meta, gone, cuts)
            assert (wps, wms) == (ps, ms)
            assert np.array_equal(got, ref) and np.array_equal(got, want) and np.array_equal(kept, rkept) and np.array_equal(kept, wkept)
            a.close()
            b.close()
        f = native.ScrubFilter(c)
        for bad in ((4, 2, -1), (1, 4, -1), (1, 2, 4)):
            with pytest.raises(sk.SKError):
                f.load_counts(*bad)
        f.close()
    ks.close()
