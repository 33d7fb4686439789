"""Count scans of resident batches take two lanes (streams) in turn, each with its own flag words and odd-chunk list, and meet at
every other call of the context (option "scan_lanes", default 2; 1 = the one stream of before).  Every count here is compared,
by equality, with the CPU oracle's for the same bytes, computed once per batch."""
import random
import time

import numpy as np
import pytest

import _oracle
import _synth
import strainer2_amd as sk

pytestmark = pytest.mark.gpu

NA, NB = 100_003, 98_317          # three tiles of 32,768 bytes and a ragged tail, each


def _cut(stream: bytes, n: int) -> bytes:
    assert len(stream) >= n
    return stream[: n - 1] + b"\n"


@pytest.fixture(scope="module")
def world():
    """strain, key set, three batches (A with IUPAC letters / U / junk bytes, B and C clean) and the oracle's count vector of each"""
    rng = random.Random(2024)
    strain = _synth.rand_dna(rng, 30_000)
    sstream = strain[:17_000] + b"\n" + strain[17_000:] + b"\n"
    ks = sk.Keyset.from_stream(sstream)
    a = _cut(_synth.fuzz_stream(rng, strain, 1200, p_junk=0.004, min_len=20, max_len=250), NA)
    b = _cut(_synth.fuzz_stream(rng, strain, 1200, p_junk=0.0, min_len=20, max_len=250), NB)
    c = _cut(_synth.fuzz_stream(rng, strain, 700, p_junk=0.0, min_len=20, max_len=250), 70_001)
    assert set(b) <= set(b"ACGT\n") and set(c) <= set(b"ACGT\n") and not set(a) <= set(b"ACGTNacgtn\n")
    t = _oracle.OracleTable()
    assert t.build_stream(sstream) == 0
    for col, data in ((1, a), (2, b), (3, c)):
        t.scan_stream(data, col)
    okeys, ocounts = t.rows()
    assert ks.keys() == okeys
    want = {"A": ocounts[:, 1].astype(np.int64), "B": ocounts[:, 2].astype(np.int64), "C": ocounts[:, 3].astype(np.int64)}
    assert want["A"].sum() > 10_000 and want["B"].sum() > 10_000 and want["C"].sum() > 5_000
    return {"ks": ks, "A": a, "B": b, "C": c, "want": want}


def _context(world, lanes, **options):
    c = sk.KmerContext(0)
    c.set_option("scan_lanes", lanes)
    for k, v in options.items():
        c.set_option(k, v)
    c.load_keyset(world["ks"], 4)
    return c


def _resident(c, data):
    buf = c.dev_alloc(len(data))
    c.dev_upload(buf, np.frombuffer(data, dtype=np.uint8))
    return buf


def test_alternation_matches_oracle_and_single_lane(world):
    """A and B scanned in turn, 40 scans into one column: 20 x (oracle of A + oracle of B), and what one lane gives"""
    got = {}
    for lanes in (2, 1):
        with _context(world, lanes) as c:
            da, db = _resident(c, world["A"]), _resident(c, world["B"])
            for _ in range(20):
                c.scan_device(da, NA, 2)
                c.scan_device(db, NB, 2)
            got[lanes] = c.counts(2)
    want = 20 * (world["want"]["A"] + world["want"]["B"])
    assert np.array_equal(got[2], want)
    assert np.array_equal(got[1], got[2])


@pytest.mark.parametrize("cap", [0, 3])
@pytest.mark.parametrize("order", ["ABAB", "BABA"])
def test_odd_bytes_on_one_lane_only(world, order, cap):
    """A fills a lane's odd-chunk list and gives its byte-string kernel work, B leaves the other lane's untouched; in the other
    order the lanes swap.  Then a lane that was dirty scans the clean batch and the other way round: AABB puts A on both lanes, and
    B on both after it.  cap = 3: the list overflows (A holds far more odd chunks) and the byte-string kernel visits every position."""
    seq = order * 3 + "AABB" + order
    with _context(world, 2, odd_list_cap=cap) as c:
        dev = {"A": _resident(c, world["A"]), "B": _resident(c, world["B"])}
        for x in seq:
            c.scan_device(dev[x], len(world[x]), 1)
        got = c.counts(1)
    want = seq.count("A") * world["want"]["A"] + seq.count("B") * world["want"]["B"]
    assert np.array_equal(got, want)


def test_joins(world):
    """zero_counts, a change of column, counts(), counts_device_ptr() and a dev_free right behind a scan, each between scans on
    both lanes: the columns hold exactly the scans made since they were last zeroed"""
    w = world["want"]
    with _context(world, 2) as c:
        da, db = _resident(c, world["A"]), _resident(c, world["B"])
        for _ in range(3):                                   # lanes 0, 1, 0 ...
            c.scan_device(da, NA, 1)
        c.zero_counts(1)                                     # ... all three gone
        c.scan_device(db, NB, 1)                             # lane 1
        c.scan_device(da, NA, 1)
        c.scan_device(da, NA, 2)                             # another column: the pending increments of column 1 are folded in first
        c.scan_device(db, NB, 2)
        c.scan_device(db, NB, 1)                             # and back
        assert np.array_equal(c.counts(2), w["A"] + w["B"])  # read between scans
        c.scan_device(da, NA, 1)
        c.scan_device(db, NB, 2)
        assert c.counts_device_ptr()
        c.scan_device(da, NA, 2)
        dc = _resident(c, world["C"])
        c.scan_device(dc, len(world["C"]), 1)
        c.scan_device(dc, len(world["C"]), 1)
        c.dev_free(dc)                                       # right behind its scans, one on each lane
        dd = _resident(c, world["B"])                        # (most likely the memory just freed)
        c.scan_device(dd, NB, 1)
        c.scan_device(dd, NB, 1)
        c.dev_free(dd)
        assert np.array_equal(c.counts(1), 2 * w["A"] + 4 * w["B"] + 2 * w["C"])
        assert np.array_equal(c.counts(2), 2 * w["A"] + 2 * w["B"])
        assert not c.counts(3).any()


@pytest.mark.parametrize("nscans", [3, 4])
def test_other_sinks_after_lane_scans(world, nscans):
    """a TALLY launch and a scan_stream right behind count scans that ended on either lane: what a fresh context gives"""
    data = world["A"]
    rec_start = np.array([0] + [i + 1 for i, ch in enumerate(data[:-1]) if ch == 10], dtype=np.uint32)
    with _context(world, 1) as f:
        want_tally, want_hits = f.tally_batch(data, rec_start)
        f.scan_stream(world["A"], 3)
        want3 = f.counts(3)
    assert want_tally.sum() > 0 and np.array_equal(want3, world["want"]["A"])
    with _context(world, 2) as c:
        da = _resident(c, world["A"])
        for _ in range(nscans):
            c.scan_device(da, NA, 2)
        tally, hits = c.tally_batch(data, rec_start)
        for _ in range(nscans):
            c.scan_device(da, NA, 2)
        c.scan_stream(world["A"], 3)
        assert np.array_equal(tally, want_tally) and np.array_equal(hits, want_hits)
        assert np.array_equal(c.counts(3), want3)
        assert np.array_equal(c.counts(2), 2 * nscans * world["want"]["A"])


@pytest.mark.parametrize("lanes", [2, 1])
def test_timing_counts_overlap_once(world, lanes):
    """20 scans: 20 launches, and the time the scan kernels kept the card busy is no longer than the loop took with its sync --
    the sum of two lanes' overlapping launches could be"""
    with _context(world, lanes) as c:
        db = _resident(c, world["B"])
        c.scan_device(db, NB, 1)
        c.sync()
        c.scan_timing(reset=True)
        t0 = time.perf_counter()
        for _ in range(20):
            c.scan_device(db, NB, 1)
        c.sync()
        wall_ms = (time.perf_counter() - t0) * 1e3
        ms, launches = c.scan_timing(reset=True)
        assert launches == 20
        assert 0.0 < ms <= wall_ms
        assert c.scan_timing() == (0.0, 0)


def test_timing_with_launches_that_really_overlap(world):
    """the same with a batch of 2,048 copies of B (201 MB, 6,145 tiles: three rounds of the card's resident workgroups, so the
    kernels, not the host's launch calls, set the pace and consecutive launches overlap at their edges): the busy time is still no
    longer than the loop took, which the plain sum of the launches' durations need not be"""
    big = np.tile(np.frombuffer(world["B"], dtype=np.uint8), 2048)
    with _context(world, 2) as c:
        dev = c.dev_alloc(big.size)
        c.dev_upload(dev, big)
        for _ in range(4):
            c.scan_device(dev, big.size, 1)
        c.sync()
        c.scan_timing(reset=True)
        t0 = time.perf_counter()
        for _ in range(20):
            c.scan_device(dev, big.size, 1)
        c.sync()
        wall_ms = (time.perf_counter() - t0) * 1e3
        ms, launches = c.scan_timing(reset=True)
        print(f"20 launches of {big.size} bytes on two lanes: busy {ms:.3f} ms, wall {wall_ms:.3f} ms")
        assert launches == 20
        assert 0.0 < ms <= wall_ms
        assert np.array_equal(c.counts(1), 24 * 2048 * world["want"]["B"])


@pytest.mark.parametrize("before", ["one_lane", "scan_stream"])
def test_lane_one_first_used_behind_a_full_event_ring(world, before):
    """70 launches on the context's stream alone (more than the ring of 64 event pairs holds) -- count scans with one lane, or
    scan_stream calls -- and only then the first scans that take lane 1: the ring's oldest pairs are added up while lane 1 is new"""
    with _context(world, 1 if before == "one_lane" else 2) as c:
        db = _resident(c, world["B"])
        for _ in range(70):
            if before == "one_lane":
                c.scan_device(db, NB, 1)
            else:
                c.scan_stream(world["B"], 1)
        c.set_option("scan_lanes", 2)
        for _ in range(70):
            c.scan_device(db, NB, 1)
        ms, launches = c.scan_timing()
        assert launches == 140 and ms > 0.0
        assert np.array_equal(c.counts(1), 140 * world["want"]["B"])
