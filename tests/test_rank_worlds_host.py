"""The crafted worlds of tests/_rank_worlds.py are what they claim to be (no GPU): every property a world is built for is asserted
here, so that a change of a builder, of cov_mix or of the host's segment sizes fails in this file instead of silently turning a
crafted world into a random one."""
import gzip
import os
import re
import subprocess

import numpy as np
import pytest

import _rank_worlds as w
from _sweep_model import informative, joint_classes

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE_DIR = os.path.join(REPO, "oracle")
U64 = np.uint64


def _oracle_bin(name):
    p = os.path.join(ORACLE_DIR, name)
    if not os.path.exists(p):
        subprocess.run(["make", "-C", ORACLE_DIR, name], check=True, stdout=subprocess.DEVNULL)
    return p


def _bytes(keys):
    """[n, 8]: the keys' bytes, byte 0 the most significant (the one radix pass 0 looks at)"""
    return np.asarray(keys, dtype=">u8").view(np.uint8).reshape(-1, 8)


# ---------------------------------------------------------------------------------------------------------------------------------
# the tie world
# ---------------------------------------------------------------------------------------------------------------------------------
def test_tie_parameters_tie_under_true_division_only():
    S, ks = w.tie_params()
    assert len(ks) == 3 and len(set(ks)) == 3 and ks == sorted(ks, reverse=True)
    for k in ks:
        f = w.tie_forms(k, S)
        assert f["true"][0] == f["true"][1]
        assert f["recip"][0] != f["recip"][1]
        assert f["f32"][0] != f["f32"][1]
        assert f["true"][0] == (3 * k) / (3 * S) == k / S       # Python's own int / int is correctly rounded
    # the search rejects what does not split: float32 holds 3k and 3S exactly while 3S < 2^24, and then divides them to one value
    assert not w.tie_ok(1777, 1000003) and w.tie_forms(1777, 1000003)["f32"][0] == w.tie_forms(1777, 1000003)["f32"][1]


def _check_tie_cuts(t, cuts, n_alive):
    score = w.score_model(t.pan, t.meta, t.pan_sum, t.meta_sum)
    order = w.rank_order(score, t.gone)
    assert len(order) == n_alive
    for c in cuts:
        (a, b), = [g for g in t.groups if g[0] < c < g[1]]      # strictly inside exactly one group
        rows = order[a:b]
        assert len(set(score[rows].tolist())) == 1 and set(t.form[rows].tolist()) == {0, 1}     # one tie group, both forms in it
        assert (np.diff(rows) > 0).all()                         # ... which goes in row order
        assert (a == 0 or score[order[a - 1]] > score[rows[0]]) and (b == n_alive or score[order[b]] < score[rows[0]])
        true = w.joint_model(t.pan, t.meta, t.gone, t.pan_sum, t.meta_sum, c)
        # the reciprocal multiply's marks differ at every cut; a float32 division ranks the forms the other way round, so the world's
        # first and last row of a group cannot serve both: it must differ at the cuts further in
        for how in ("recip", "f32") if a + 1 < c < b - 1 else ("recip",):
            wrong = w.joint_model(t.pan, t.meta, t.gone, t.pan_sum, t.meta_sum, c, how)
            assert (wrong != true).any(), (c, how)
        assert int(true.sum()) == c + int(t.gone.sum())


def test_tie_world_cuts_fall_inside_groups_and_tell_the_divisions_apart():
    t = w.tie_world()
    n_alive = int((t.gone == 0).sum())
    assert 2900 <= len(t.pan) <= 3100 and 0 < int(t.gone.sum()) < len(t.pan) // 5
    assert len(t.inside) == 4 * len(t.ks) and {g[0] + 1 for g in t.groups} <= set(t.inside) and {g[1] - 1 for g in t.groups} <= set(t.inside)
    assert {g[0] for g in t.groups} | {g[1] for g in t.groups} <= set(t.edge)
    order = w.rank_order(w.score_model(t.pan, t.meta, t.pan_sum, t.meta_sum), t.gone)
    assert not np.array_equal(order, np.sort(order))            # the row order is not the rank order
    _check_tie_cuts(t, t.inside, n_alive)
    # the reciprocal multiply splits every group in two
    wrong = w.score_model(t.pan, t.meta, t.pan_sum, t.meta_sum, "recip")
    assert len(set(wrong[t.gone == 0].tolist())) == 2 * len(t.ks)


@pytest.mark.parametrize("drug,m", w.TABLE_RUNS)
def test_tie_table_has_the_true_sums_and_the_oracle_is_the_model(tmp_path, drug, m):
    t = w.tie_table(drug=drug)
    assert int(t.pan.sum()) == 3 * t.S == t.pan_sum and int(t.meta.sum()) == t.S == t.meta_sum
    assert bool(t.gone.any()) == drug
    n_alive = int((t.gone == 0).sum())
    cut = w.script_n_scrub(m, t.all_kmers, t.drug_scrubbed, n_alive)
    _check_tie_cuts(t, [cut], n_alive)
    marks = w.joint_model(t.pan, t.meta, t.gone, t.pan_sum, t.meta_sum, cut)
    with gzip.GzipFile(tmp_path / "t.gz", "wb", mtime=0) as g:
        g.write(t.text)
    p = subprocess.run([_oracle_bin("ksf_oracle"), "-s", str(tmp_path / "t.gz"), "-m", repr(m)], capture_output=True)
    assert p.returncode == 0, p.stderr
    assert informative(p.stdout) == [k for k, gone in zip(t.kmers, marks) if not gone]
    cl, kept, ps, ms = joint_classes(t.pan, t.meta, t.gone, [cut])                  # the sweep's model computes the same sums and marks
    assert (ps, ms) == (t.pan_sum, t.meta_sum) and np.array_equal(cl, 1 - marks)


# ---------------------------------------------------------------------------------------------------------------------------------
# ladders
# ---------------------------------------------------------------------------------------------------------------------------------
def _ladder_keys(world):
    """the keys of the world's distinct counts, ascending"""
    return w.key_model(w.score_model(world.counts, np.zeros(len(world.counts), dtype=np.int64), world.pan_sum, world.meta_sum))


def test_ulp_ladder_keys_are_consecutive_and_carry():
    u = w.ulp_ladder()
    keys = _ladder_keys(u)
    assert len(keys) == 512 and (np.diff(keys.astype(np.int64)) == 1).all()
    assert int(keys[0]) == 0x3FE0000000000001 and int(keys[255]) == 0x3FE0000000000100 and int(keys[511]) == 0x3FE0000000000200
    score = w.score_model(u.pan, u.meta, u.pan_sum, u.meta_sum)
    vals, mult = np.unique(score, return_counts=True)
    assert len(vals) == 512 and (mult == 2).all() and len(u.pan) == 1024
    assert ((u.pan > 0) ^ (u.meta > 0)).all() and int((u.pan > 0).sum()) == 512      # every value once through either column
    assert (np.diff(vals) == 2.0 ** -53).all()


@pytest.mark.parametrize("p", [2, 3, 4, 5, 6, 7])
def test_digit_ladder_varies_one_byte(p):
    d = w.digit_ladder(p)
    kb = _bytes(_ladder_keys(d))
    assert len(kb) == 256
    if p < 7:
        assert (kb[:, :p] == kb[0, :p]).all() and kb[:, p].tolist() == list(range(256))       # digits 0 .. 255 of pass p
        assert (kb[:, p + 1: 7] == 0).all() and (kb[:, 7] == 1).all()                         # below it: the + 1 alone
    else:
        # the + 1 lands in the last byte itself: digits 1 .. 255 under one prefix, and the last key carries out of the byte
        assert (kb[:255, :7] == kb[0, :7]).all() and kb[:255, 7].tolist() == list(range(1, 256))
        assert kb[255, 7] == 0 and kb[255, 6] == kb[0, 6] + 1 and (kb[255, :6] == kb[0, :6]).all()
    assert sorted(np.maximum(d.pan, d.meta).tolist()) == d.counts.tolist()


def test_nibble_and_exponent_ladders():
    kb = _bytes(_ladder_keys(w.nibble_ladder()))
    assert (kb[:, 0] == 0x3F).all() and kb[:, 1].tolist() == [0xE0 + d for d in range(16)] and (kb[:, 2:7] == 0).all() and (kb[:, 7] == 1).all()
    e = w.exponent_ladder()
    keys = _ladder_keys(e)
    assert [int(k) for k in keys] == [((1023 - 62 + x) << 52) + 1 for x in range(63)]
    kb = _bytes(keys)
    assert set(kb[:, 0].tolist()) == {0x3C, 0x3D, 0x3E, 0x3F} and len(set(kb[:, 1].tolist())) == 16 and int(keys[-1]) == 0x3FF0000000000001


def test_one_world_holds_one_and_its_neighbour():
    o = w.one_world()
    score = w.score_model(o.pan, o.meta, o.pan_sum, o.meta_sum)
    keys = {int(k) for k in w.key_model(score)}
    assert 1.0 in score.tolist() and 1.0 - 2.0 ** -53 in score.tolist()
    assert {0x3FF0000000000001, 0x3FF0000000000000, 0x3FEFFFFFFFFFFFFF} <= keys     # 1.0; its neighbour's key is 1.0's bit pattern
    assert score.max() == 1.0


def test_zero_world_has_every_kind_of_zero_row():
    z = w.zero_world()
    score = w.score_model(z.pan, z.meta, z.pan_sum, z.meta_sum)
    assert (score[z.zero] == 0.0).all() and (score[(z.gone == 0) & ~z.zero] > 0.0).all() and int(z.zero.sum()) > 100
    kinds = set(zip(z.pan[z.zero].tolist(), z.meta[z.zero].tolist()))
    assert kinds == {(0, 0), (-(1 << 31), -1), (-1, 0), (0, -(1 << 31))}
    order = w.rank_order(score, z.gone)
    tail = order[len(order) - int(z.zero.sum()):]
    assert np.array_equal(tail, np.flatnonzero(z.zero))          # last, in row order
    assert (w.key_model(score[z.zero]) == 1).all()


def test_bigint_world_pairs():
    for a, b in w.BIG_EQUAL:
        assert a != b and float(a) == float(b) and a < (1 << 63) and b < (1 << 63)
    for a, b in w.BIG_APART:
        assert float(a) != float(b)
    listed = [tuple(p) for p in w.BIG_EQUAL]
    assert ((1 << 53), (1 << 53) + 1) in listed and ((1 << 63) - 512, (1 << 63) - 1) in listed
    # the pair 2^53 + 2, 2^53 + 3: round-to-nearest-even sends 2^53 + 3 up to 2^53 + 4, so the two are NOT one double; the world holds
    # the triple, and their order tells a truncating conversion (which would join them) from the right one
    assert float((1 << 53) + 3) == float((1 << 53) + 4) != float((1 << 53) + 2) and ((1 << 53) + 2, (1 << 53) + 3) in w.BIG_APART
    b = w.bigint_world()
    every = {v for pair in w.BIG_EQUAL + w.BIG_APART for v in pair}
    assert every <= set(np.maximum(b.pan, b.meta).tolist())
    assert [float(v) for v in b.counts.tolist()] == b.counts.astype(np.float64).tolist()      # numpy converts as Python does
    score = w.score_model(b.pan, b.meta, b.pan_sum, b.meta_sum)
    assert float(b.pan_sum) == 2.0 ** 63 and len(set(score.tolist())) < len(every)
    for x, y in w.BIG_EQUAL:
        sx = score[np.maximum(b.pan, b.meta) == x]
        sy = score[np.maximum(b.pan, b.meta) == y]
        assert len(sx) == len(sy) == 3 and set(sx.tolist()) == set(sy.tolist()) and len(set(sx.tolist())) == 1
    order = w.rank_order(score, np.zeros(len(score), dtype=np.uint8))
    ties = [order[score[order] == s] for s in set(score.tolist())]
    assert any((np.diff(np.maximum(b.pan, b.meta)[t]) < 0).any() and (np.diff(np.maximum(b.pan, b.meta)[t]) > 0).any() for t in ties)
    assert all((np.diff(t) > 0).all() for t in ties)            # inside a tie, row order -- not integer order


def test_eq_scan_world_spans_the_threads_shares():
    e = w.eq_scan_world()
    nchunk = (e.n + w.FLT_CHUNK - 1) // w.FLT_CHUNK
    per = (nchunk + w.FLT_THREADS - 1) // w.FLT_THREADS
    assert e.n == 257 * 4096 + 1 and nchunk == 258 and per == 2
    tie = np.flatnonzero((e.pan == 500) & (e.gone == 0))
    chunks = sorted(set((tie // w.FLT_CHUNK).tolist()))
    assert chunks == [1, 2, 3, 257]
    assert {c // per for c in chunks} == {0, 1, 128}             # the shares of three threads, the last of them one chunk long
    assert e.run == len(tie) and e.above == int(((e.pan > 500) & (e.gone == 0)).sum())
    in_chunk1 = int((tie < 2 * w.FLT_CHUNK).sum())
    assert 0 < in_chunk1 < e.run - 1                             # cuts above in_chunk1 end in another thread's share


def test_hist_column():
    col = w.hist_column()
    assert col.max() == 2060 and (col == 0).any() and (col < 0).any() and set(range(2061)) <= set(col.tolist())
    h = w.hist_model(col, 1, 2047)
    assert h[2046] == (col == 2047).sum() and h[2047] == (col >= 2048).sum() and h.sum() == (col > 0).sum()


# ---------------------------------------------------------------------------------------------------------------------------------
# the hash, the probe, the segments
# ---------------------------------------------------------------------------------------------------------------------------------
def _source(name):
    return open(os.path.join(REPO, "strainer2_amd", "csrc", name)).read()


def test_cov_mix_is_the_sources():
    src = _source("sk_cover.hip")
    body = re.search(r"uint64_t cov_mix\(uint64_t x\)\s*\{(.*?)return x;", src, re.S).group(1)
    assert [int(m, 16) for m in re.findall(r"x \*= (0x[0-9A-Fa-f]+)ull", body)] == list(w.COV_MIX_MULTIPLIERS)
    assert [int(s) for s in re.findall(r"x \^= x >> (\d+)", body)] == [w.COV_MIX_SHIFT] * 3
    assert re.sub(r"\s+", "", body) == "x^=x>>33;x*=0xFF51AFD7ED558CCDull;x^=x>>33;x*=0xC4CEB9FE1A85EC53ull;x^=x>>33;"
    # ... and the model computes it: murmur3's finaliser, by Python's own integers
    def mix(x):
        x ^= x >> 33
        x = x * 0xFF51AFD7ED558CCD % 2 ** 64
        x ^= x >> 33
        x = x * 0xC4CEB9FE1A85EC53 % 2 ** 64
        return x ^ (x >> 33)
    xs = [0, 1, 2 ** 62 - 1, 2 ** 64 - 2, 0x0123456789ABCDEF] + [int(v) for v in np.random.default_rng(1).integers(0, 2 ** 62, 200)]
    assert [int(v) for v in w.cov_mix(np.array(xs, dtype=U64))] == [mix(x) for x in xs]


def test_segment_sizes_are_the_hosts():
    src = _source("sk_cover.hip")
    assert len(re.findall(r"uint64_t c = 2;\s*while \(c < 2 \* cnt\[s\]\) c <<= 1;", src)) == 4       # count, spectrum, thresholds, classes
    assert re.search(r"uint64_t slots = 64;[^\n]*\n\s*while \(slots < 2 \* n\) slots <<= 1;", src)    # recurrence: one shared set
    assert re.search(r"if \(c\) cnt\[sample\[i\]\]\+\+;", src)                                          # thresholds: lines of class >= 1
    assert [w.segment_slots(n) for n in (0, 1, 2, 3, 512, 1024, 1025, 2048)] == [2, 2, 4, 8, 1024, 2048, 4096, 4096]
    assert w.segment_slots(2, 64) == 64 and w.segment_slots(2048, 64) == 4096


@pytest.mark.parametrize("large", [False, True])
def test_segment_world_clusters_sit_at_the_end_and_wrap(large):
    s = w.segment_world(large=large)
    assert s.keys.max() < 2 ** 62 and len(s.keys) == (3886 if large else 302)
    lines = np.bincount(s.sample, minlength=s.nsamples)
    want = {w.SEG_TINY: (2, 4, 1)}
    if large:
        want.update({w.SEG_A: (2048, 4096, w.SEG_LAST), w.SEG_B: (1024, 2048, w.SEG_LAST)})
    assert lines[w.SEG_EMPTY] == 0 and lines[w.SEG_D] == 300
    cls1 = np.bincount(s.sample[s.totals > w.THRESHOLDS[0]], minlength=s.nsamples)
    assert np.array_equal(cls1, lines)                            # every line has class >= 1: the thresholds' segments are the same
    assert set(s.cls.tolist()) == {1, 2, 3} and all(int(t) > w.THRESHOLDS[c - 1] and (c == 3 or int(t) <= w.THRESHOLDS[c])
                                                     for t, c in zip(s.totals.tolist(), s.cls.tolist()))
    pairs = {}
    for smp, k, c in zip(s.sample.tolist(), s.keys.tolist(), s.cls.tolist()):
        assert pairs.setdefault((smp, k), c) == c                 # a (sample, key) pair carries one class
    longest = 0
    for smp, (n, slots, last) in want.items():
        assert lines[smp] == n and w.segment_slots(n) == slots
        k = s.keys[s.sample == smp]
        home, slot, steps, wrapped = w.probe_walk(k, slots - 1)
        assert home.min() >= slots - last and wrapped and slot.min() == 0       # homes at the end; the cluster goes on at slot 0
        taken = np.zeros(slots, dtype=bool)
        taken[slot] = True
        nkeys = len(set(k.tolist()))
        assert taken.sum() == nkeys and taken[home.min():].all() and taken[: nkeys - (slots - home.min())].all()      # one run
        longest = max(longest, int(steps.max()))
    if large:
        assert longest > 128
        a, b = s.keys[s.sample == w.SEG_A], s.keys[s.sample == w.SEG_B]
        assert set(a.tolist()) == set(b.tolist()) and len(set(a.tolist())) == 1024 and len(b) == 1024
        c = s.keys[s.sample == w.SEG_C]
        assert lines[w.SEG_C] == 512 and w.segment_slots(512) == 1024 and not set(c.tolist()) & set(a.tolist())
        home, slot, _, wrapped = w.probe_walk(c, 1023)
        assert home.max() < 16 and not wrapped                    # where a walk that ran out of sample 2's segment would land
    assert lines[w.SEG_TINY] == 2 and len(set(s.keys[s.sample == w.SEG_TINY].tolist())) == 2
    home, slot, steps, wrapped = w.probe_walk(s.keys[s.sample == w.SEG_TINY], 3)
    assert home.tolist() == [3, 3] and sorted(slot.tolist()) == [0, 3] and wrapped


@pytest.mark.parametrize("large", [False, True])
def test_recurrence_world_wraps_in_the_shared_set(large):
    r = w.recurrence_world(large=large)
    slots = w.segment_slots(len(r.keys), 64)
    assert slots == r.mask + 1 == (4096 if large else 64)
    home, slot, steps, wrapped = w.probe_walk(r.keys, r.mask)
    assert home.min() >= slots - (w.SEG_LAST if large else 1) and wrapped and slot.min() == 0
    assert int(steps.max()) > (128 if large else 0)
    assert len(set(r.sample.tolist())) == (4 if large else 2) and r.sample.max() < r.nsamples


# ---------------------------------------------------------------------------------------------------------------------------------
# the general-mode hit list
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def general():
    return w.general_hits()


def test_general_hit_list_collides_and_switches_late(general):
    text, rows, nclean = general
    assert len(rows) == 200_000 and text.count(b"\n") == 200_000 + 16
    acgt = set(b"ACGT")
    plain = [len(k) == 31 and set(k) <= acgt for _, _, _, k in rows]
    first_ragged = plain.index(False)
    assert first_ragged == nclean > len(rows) // 2 and not any(plain[nclean:])       # the switch: past the midpoint
    assert any(a + c > 1 for _, a, c, _ in rows[:nclean])                            # ... with packed lines to replay
    for min_hits in (1, 3):
        made = {}
        for s, a, c, k in rows:
            if a + c > min_hits:
                made.setdefault(s + k, set()).add((s, k))
        assert sum(len(v) >= 2 for v in made.values()) >= 300                        # one string, two (sample, k-mer) pairs
        assert sum(len({s for s, _ in v}) >= 3 for v in made.values()) >= 50
    ragged = [k for _, _, _, k in rows[nclean:]]
    assert len({len(k) for k in ragged}) > 10 and {k[:1] for k in ragged} >= {b"1", b"A"}
    names = {s for s, _, _, _ in rows}
    assert names == set(w.GENERAL_SAMPLES) and all(any(x != y and y.startswith(x) for x in names) for y in names if y != b"s")


@pytest.mark.parametrize("extra,min_hits", [([], 1), (["-m", "3"], 3)])
def test_general_hit_list_oracle_is_the_restatement(general, tmp_path, extra, min_hits):
    text, rows, _ = general
    path = tmp_path / "Some_strain_x1.kmer_hits.gz"
    with gzip.GzipFile(path, "wb", compresslevel=1, mtime=0) as g:
        g.write(text)
    p = subprocess.run([_oracle_bin("kcd_oracle"), "-k", str(path)] + extra, capture_output=True)
    assert p.returncode == 0, p.stderr
    got = w.table_counts(p.stdout)
    want = w.script_counts(rows, min_hits)
    assert list(got) == list(want) and got == want and len(got) == 4
    per_pair = {}
    for s, a, c, k in rows:
        if a + c > min_hits:
            per_pair.setdefault(s, set()).add(k)
    assert any(len(per_pair[s]) != want[s][0] for s in want)     # the global rule differs from per-sample distinct counting here


def test_first_seen_model():
    uq, tot = w.first_seen_model([3, 3, 1, 3, 1, 0], [2, 0, 0, 1, 2, 2], 4)
    assert uq.tolist() == [1, 0, 2, 0] and tot.tolist() == [2, 1, 3, 0]
