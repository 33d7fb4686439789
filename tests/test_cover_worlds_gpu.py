"""Step 4's hit-list counters on the device (sk_cover.hip) at chosen inputs: sk_first_seen_count against the script's rule, cov_count's
one-atomic-per-run aggregation on crafted sample sequences, the five insert kernels' linear probe on keys that home at the end of
their segment (tests/_rank_worlds.py; tests/test_rank_worlds_host.py proves the worlds), and coverage_depth against the oracle on
a hit list that switches to general mode late.  Every comparison is exact."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import _rank_worlds as w
import strainer2_amd as sk
from _recurrence_model import check_tables, recurrence
from _spectrum_model import spectrum
from _thresholds_model import numbers

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE_DIR = os.path.join(REPO, "oracle")
SK_E_ARG = -3
U64 = np.uint64


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


# ---------------------------------------------------------------------------------------------------------------------------------
# first sightings
# ---------------------------------------------------------------------------------------------------------------------------------
def _first_seen_check(ctx, ids, sample, nids, nsamples):
    ids, sample = np.asarray(ids, dtype=np.uint32), np.asarray(sample, dtype=np.uint32)
    uq, tot = ctx.first_seen_count(ids, sample, nids, nsamples)
    wu, wt = w.first_seen_model(ids, sample, nsamples)
    assert np.array_equal(tot, wt) and np.array_equal(uq, wu), (len(ids), nids, nsamples)
    return uq, tot


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 70001])
def test_first_seen_count_against_the_rule(ctx, n):
    rng = np.random.default_rng(n)
    ns = 7
    smp = rng.integers(0, ns - 2, n)                             # samples 5 and 6 have no line
    uq, tot = _first_seen_check(ctx, np.zeros(n), smp, 1, ns)    # all lines one id: the first line's sample has it
    assert uq.sum() == 1 and uq[smp[0]] == 1 and tot.sum() == n
    uq, tot = _first_seen_check(ctx, rng.permutation(n), smp, n, ns)         # all ids distinct
    assert np.array_equal(uq, tot) and not tot[5:].any()
    ids = rng.integers(0, max(n // 3, 1), n)
    _first_seen_check(ctx, ids, smp, max(n // 3, 1), ns)
    _first_seen_check(ctx, ids * 5 + 3, smp, 5 * n + 1000, ns)   # nids larger than the ids used
    _first_seen_check(ctx, ids, smp + 2, max(n // 3, 1), ns + 5000)          # ... and nsamples than the samples


def test_first_seen_credit_goes_to_the_first_line_across_workgroups(ctx):
    """ids whose first line is the last lane of a workgroup and whose later lines lie in other workgroups, under other samples"""
    n, ns = 70001, 9
    rng = np.random.default_rng(3)
    ids = np.arange(n, dtype=np.int64) + 10                      # everything else: distinct
    smp = rng.integers(0, 3, n)
    lines = {0: [255, 256, 511, 512, 4096, 70000], 1: [767, 768, 1023, 69999], 2: [69887, 69888, 70000 - 1 - 64], 3: [63, 64, 127, 128]}
    used = set()
    for special, at in lines.items():
        for j, i in enumerate(at):
            if i not in used:
                used.add(i)
                ids[i], smp[i] = special, 3 + (j + special) % 6  # a different sample at every line
    assert lines[0][0] % 256 == 255 and lines[1][0] % 256 == 255 and lines[2][0] % 256 == 255 and lines[3][0] % 64 == 63
    uq, tot = _first_seen_check(ctx, ids, smp, n + 10, ns)
    only = np.zeros(ns, dtype=U64)
    for special, at in lines.items():
        only[smp[at[0]]] += U64(1)
    assert np.array_equal(uq[3:], only[3:])                      # the samples of the first lines, no other


def test_first_seen_count_edges_and_errors(ctx):
    uq, tot = ctx.first_seen_count([], [], 5, 3)
    assert uq.tolist() == [0, 0, 0] and tot.tolist() == [0, 0, 0]
    uq, tot = ctx.first_seen_count([], [], 0, 3)
    assert not uq.any() and not tot.any()
    for bad in (dict(ids=[0, 5], sample=[0, 0], nids=5, nsamples=2), dict(ids=[0, 1], sample=[0, 2], nids=5, nsamples=2),
                dict(ids=[0], sample=[0], nids=5, nsamples=0), dict(ids=[0], sample=[0], nids=0, nsamples=1)):
        with pytest.raises(sk.SKError) as e:
            ctx.first_seen_count(**bad)
        assert e.value.code == SK_E_ARG, bad


# ---------------------------------------------------------------------------------------------------------------------------------
# cov_count's runs
# ---------------------------------------------------------------------------------------------------------------------------------
def _count_model(keys, sample, nsamples):
    keys, sample = np.asarray(keys, dtype=U64), np.asarray(sample, dtype=np.int64)
    total = np.bincount(sample, minlength=nsamples).astype(U64)
    uniq = np.zeros(nsamples, dtype=U64)
    for s in np.unique(sample):
        uniq[s] = len(np.unique(keys[sample == s]))
    return uniq, total


SEQUENCES = {
    "one_sample": lambda i: np.zeros(len(i), dtype=np.int64),
    "new_sample_every_lane": lambda i: i % 7,
    "runs_start_at_lane_63": lambda i: ((i + 1) // 64) % 5,
    "runs_of_100": lambda i: (i // 100) % 6,                    # across wave and workgroup boundaries
    "runs_of_256_off_by_200": lambda i: ((i + 200) // 256) % 3,
    "lane_63_alone": lambda i: np.where(i % 64 == 63, 1 + (i // 64) % 3, 0),
    "tail_lane_alone": lambda i: np.where(i == len(i) - 1, 4, (i // 64) % 2),
}


@pytest.mark.parametrize("n", [1, 63, 65, 127, 257, 319, 69951, 69953, 70001])
def test_distinct_count_on_crafted_sample_sequences(ctx, n):
    """the same 50 key values under every sample: one atomic per run of equal samples, whatever the run's first and last lane"""
    assert n % 64 in (1, 63, 49)
    i = np.arange(n, dtype=np.int64)
    keys = ((i * 7919) % 50).astype(U64) + U64(1 << 40)
    for name, seq in SEQUENCES.items():
        smp = seq(i)
        for nsamples, where in ((8, smp), (5000, np.array([0, 4999, 77, 1, 2500, 31, 4998, 64])[smp])):       # few of many samples used
            uq, tot = ctx.distinct_count(keys, where, nsamples)
            wu, wt = _count_model(keys, where, nsamples)
            assert np.array_equal(tot, wt) and np.array_equal(uq, wu), (name, n, nsamples)


# ---------------------------------------------------------------------------------------------------------------------------------
# clusters at the end of a segment: the probe wraps inside its own segment
# ---------------------------------------------------------------------------------------------------------------------------------
def _per_sample(world):
    for s in range(world.nsamples):
        sel = world.sample == s
        yield s, world.keys[sel], world.totals[sel], world.cls[sel]


@pytest.mark.parametrize("large", [False, True])
def test_end_of_segment_clusters_through_the_per_sample_calls(ctx, large):
    """cov_count, cov_count_depth, cov_thr_insert, cov_cls_insert: keys that home in the last slots of their sample's segment, a
    neighbour that holds the same key values, and one whose keys home where a walk that left the segment would land"""
    s = w.segment_world(large=large)
    ns, D, F = s.nsamples, 2, 3
    uq, tot = ctx.distinct_count(s.keys, s.sample, ns)
    su, st, spec, deep = ctx.distinct_spectrum(s.keys, s.sample, ns, D)
    tu, tt = ctx.distinct_thresholds(s.keys, s.sample, s.totals, ns, w.THRESHOLDS)
    cu, ct = ctx.distinct_classes(s.keys, s.sample, s.cls, ns, F)
    for smp, keys, totals, cls in _per_sample(s):
        _, mult = np.unique(keys, return_counts=True)
        assert (int(uq[smp]), int(tot[smp])) == (len(mult), len(keys)), smp
        assert (int(su[smp]), int(st[smp])) == (len(mult), len(keys)), smp
        bins, dp = spectrum(mult, D)
        assert np.array_equal(spec[smp], bins) and int(deep[smp]) == dp, smp
        wu, wt = numbers(keys.tolist(), totals.tolist(), w.THRESHOLDS)
        assert tu[smp].tolist() == wu and tt[smp].tolist() == wt, smp
        for q in range(F):
            sel = cls >= q + 1
            assert (int(cu[smp, q]), int(ct[smp, q])) == (len(set(keys[sel].tolist())), int(sel.sum())), (smp, q)
    if large:
        assert (int(uq[w.SEG_A]), int(tot[w.SEG_A])) == (1024, 2048) and (int(uq[w.SEG_B]), int(tot[w.SEG_B])) == (1024, 1024)
        assert int(spec[w.SEG_A, 1]) == 1024 and int(spec[w.SEG_B, 0]) == 1024 and int(spec[w.SEG_C, 1]) == 256
    assert (int(uq[w.SEG_TINY]), int(tot[w.SEG_TINY])) == (2, 2) and not tot[w.SEG_EMPTY] and not spec[w.SEG_EMPTY].any()


@pytest.mark.parametrize("large", [False, True])
def test_end_of_segment_cluster_in_the_shared_set(ctx, large):
    """cov_recur_insert: one set for all samples; the keys home in its last slots"""
    for r in (w.recurrence_world(large=large), w.segment_world(large=large)):
        uniq, col = np.unique(r.keys, return_inverse=True)
        planes = np.zeros((r.nsamples, len(uniq)), dtype=bool)
        planes[r.sample.astype(np.int64), col] = True
        wh, ws = recurrence(planes)
        wh[0] = 0
        hist, shared = ctx.distinct_recurrence(r.keys, r.sample, r.nsamples, pairs=True)
        assert np.array_equal(hist, wh) and np.array_equal(shared, ws)
        check_tables(hist, shared)
        assert np.array_equal(ctx.distinct_recurrence(r.keys, r.sample, r.nsamples), wh)


# ---------------------------------------------------------------------------------------------------------------------------------
# the program in general mode
# ---------------------------------------------------------------------------------------------------------------------------------
def test_coverage_program_in_general_mode_vs_oracle(tmp_path):
    """200 000 hit lines, ragged k-mer text after the midpoint (to_general replays the packed lines), sample names that are prefixes
    of each other so that joined strings collide across samples: first sightings far apart in the file, in other workgroups"""
    text, rows, nclean = w.general_hits()
    path = tmp_path / "Some_strain_x1.kmer_hits.gz"
    with gzip.GzipFile(path, "wb", compresslevel=1, mtime=0) as g:
        g.write(text)
    for extra, min_hits in (([], 1), (["-m", "3"], 3)):
        argv = ["-k", str(path)] + extra
        want = subprocess.run([_oracle_bin("kcd_oracle")] + argv, capture_output=True)
        got = subprocess.run([sk.cli_path("coverage_depth")] + argv, capture_output=True)
        assert want.returncode == 0 and want.stdout.count(b"\n") == 5
        assert (got.returncode, got.stdout) == (0, want.stdout)
        assert w.table_counts(got.stdout) == w.script_counts(rows, min_hits)
