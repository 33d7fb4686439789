"""The hash table, the byte-string index, the union table and the filters at geometries that are chosen, not left to chance
(tests/_craft.py; what each world is, is asserted on the CPU in tests/test_hash_worlds_host.py): key clusters at the END of a table
so that the walks of present and absent keys run over the last slot into slot 0 and are longer than two waves; a table 90 % full;
a table of 2^25 slots (the kh << 24 half of sk_slot0); level-1 filters that are full, of an odd block count, nearly empty; and the
two edges of the partitioned pipeline's bins.  Every consumer of the table is run on them -- both key builders, COUNT from bytes,
resident on both lanes and packed, with and without the text stage, both pipelines, the listed and the exhaustive byte-string
kernel, TALLY in its forms, the union -- and compared, by integer equality, with the CPU oracle (per-row counts:
_oracle.OracleTable; per-record tallies and the log of informative hits: _tally_ref)."""
import ctypes as C
import functools
import os
import random
import time

import numpy as np
import pytest

import _craft
import _oracle
import _synth
import _tally_ref as tr
import strainer2_amd as sk
from strainer2_amd.native import TallyBatch, lib

pytestmark = pytest.mark.gpu

SK_E_ARG = -3
STRAIN_ORDER = 0xFFFFFFFF                                              # Keyset.from_stream(initial_slots=...): rows by first occurrence
_CODE = np.full(256, 255, dtype=np.uint8)
for _i, _b in enumerate(b"ACGT"):
    _CODE[_b] = _i
_CLEAN = bytes(b if b in b"ACGTacgtNn\n" else ord("N") for b in range(256))


def _oracle_rows(t):
    """(packed keys, counts[rows, ncols]) of an oracle table whose keys are all A/C/G/T, in row order"""
    n = t.size
    keys = np.zeros((max(n, 1), 32), dtype=np.uint8)
    counts = np.zeros((max(n, 1), t.ncols), dtype=np.uint32)
    _oracle.L.kso_table_rows(t.h, 31, keys.ctypes.data, counts.ctypes.data)
    code = _CODE[keys[:n, :31]]
    assert (code < 4).all()
    packed = np.zeros(n, dtype=np.uint64)
    for i in range(31):
        packed = (packed << np.uint64(2)) | code[:, i].astype(np.uint64)
    return packed, counts[:n]


def _type_col(informative):
    t = np.ones(len(informative), dtype=np.uint32)
    t[informative] = 2
    return t


def _context(load_pct=50, **options):
    c = sk.KmerContext(0)
    if load_pct != 50:
        c.set_option("table_load_pct", load_pct)
    for k, v in options.items():
        c.set_option(k, v)
    return c


def _resident(c, data):
    buf = c.dev_alloc(len(data))
    c.dev_upload(buf, np.frombuffer(data, dtype=np.uint8))
    return buf


def _scan_packed(c, data, col):
    """sk_pack_stream on the host, then sk_scan_pinned_packed"""
    pk = c.pinned_alloc(int(lib.sk_packed_bytes(len(data))) + 16)
    try:
        _, odd = sk.pack_stream(data, out=pk)
        assert not odd
        c.ticket_wait(c.scan_pinned_packed(pk, len(data), col))
    finally:
        c.pinned_free(pk)


# ---- what the oracle says, once per world -----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _want(name):
    """the world, its key set in the oracle's row order, and the oracle's counts of its reads (all of them / the packable ones)"""
    w = getattr(_craft, name)()
    small = name != "sparse5"
    t = _oracle.OracleTable(capacity=_craft.CAP) if small else _oracle.OracleTable()
    assert t.build_stream(w.sstream) == 0
    t.scan_stream(w.stream, 1)
    t.scan_stream(w.stream_clean, 2)
    opacked, ocounts = _oracle_rows(t)
    t.close()
    ks = sk.Keyset.from_stream(w.sstream, initial_slots=_craft.CAP, default_val=1, incr=0) if small else sk.Keyset.from_stream(w.sstream, default_val=1, incr=0)
    assert np.array_equal(ks.packed(), opacked), "row order differs from the oracle"
    allc, clean = ocounts[:, 1].astype(np.int64), ocounts[:, 2].astype(np.int64)
    row_of = {int(k): i for i, k in enumerate(opacked.tolist())}
    crafted_rows = np.array([row_of[int(k)] for k in w.crafted])
    assert (clean[crafted_rows] >= 2).all() and allc.sum() > clean.sum() > 2 * len(w.crafted)   # every crafted key hit on both strands; U windows hit
    return {"w": w, "ks": ks, "all": allc, "clean": clean, "packed": opacked, "row_of": row_of}


@functools.lru_cache(maxsize=None)
def _tally_want(name):
    """the oracle strain of a small world, informative rows (half of the crafted keys and a quarter of the rest), and the reference
    tallies and log of its reads, all of them and the packable ones"""
    x = _want(name)
    w = x["w"]
    o = tr.OracleStrain(w.sstream, capacity=_craft.CAP)
    assert o.keys == x["ks"].keys()
    rng = random.Random(w.seed)
    informative = np.array([rng.random() < 0.25 for _ in range(o.nrows)])
    for k in w.crafted[::2]:
        informative[x["row_of"][int(k)]] = True
    starts, starts_clean = tr.starts_of(w.recs), tr.starts_of(w.recs_clean)
    ref = o.tally(w.stream, starts, informative)
    ref_clean = o.tally(w.stream_clean, starts_clean, informative)
    assert int(ref[0][:, 1].sum()) > int(ref_clean[0][:, 1].sum()) > 100
    return {"o": o, "informative": informative, "starts": starts, "starts_clean": starts_clean, "ref": ref, "ref_clean": ref_clean}


# ---- both key builders ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["wrap50", "full90"])
def test_table_from_the_hosts_key_set(name):
    """Keyset.from_stream + load_keyset (sk_table_insert, sk_table_load_text): counts of all reads, U windows included"""
    x = _want(name)
    w = x["w"]
    with _context(w.load_pct) as c:
        c.load_keyset(x["ks"], 4)
        c.scan_stream(w.stream, 1)
        c.scan_stream(w.stream_clean, 2)
        assert np.array_equal(c.counts(1), x["all"]) and np.array_equal(c.counts(2), x["clean"])


@pytest.mark.parametrize("name", ["wrap50", "full90"])
def test_table_built_on_the_device(name, tmp_path):
    """skh_keyset_build_on_device (sk_build_insert, sk_build_first, sk_build_index): the host's key set exactly, row by row that of
    the host builder in strain order, column 0 all col0_value, and the oracle's count for every key"""
    x = _want(name)
    w = x["w"]
    fa = tmp_path / "s.fa"
    fa.write_bytes(b"".join(b">r%d\n%s\n" % (i, r) for i, r in enumerate(w.strain_recs)))
    with _context(w.load_pct) as cd:
        dks = sk.native._KeysetStruct()
        lib.skh_keyset_build_on_device.argtypes = [C.c_void_p, C.c_void_p, C.c_char_p, C.c_uint32, C.c_uint32]
        assert lib.skh_keyset_build_on_device(C.byref(dks), cd._h, os.fsencode(str(fa)), 4, 7) == 0
        try:
            n = dks.nrows
            assert n == w.nkeys == cd.nrows
            whole = np.zeros(n, dtype=np.uint64)
            lib.sk_table_export_keys.argtypes = [C.c_void_p, C.c_void_p]
            assert lib.sk_table_export_keys(cd._h, whole.ctypes.data) == 0
            assert np.array_equal(np.sort(whole), np.sort(x["packed"]))
            ordered = sk.Keyset.from_stream(w.sstream, initial_slots=STRAIN_ORDER, default_val=1, incr=0)
            try:                                                           # and in the ORDER of the host's key set in strain order
                assert ordered.nrows == n and np.array_equal(whole, ordered.packed()), np.nonzero(whole != ordered.packed())[0][:10]
            finally:
                ordered.close()
            assert cd.counts(0).tolist() == [7] * n
            cd.scan_stream(w.stream, 1)
            cd.scan_stream(w.stream_clean, 2)
            rows = np.array([x["row_of"][int(k)] for k in whole])        # the host's row of every device row
            assert np.array_equal(cd.counts(1), x["all"][rows]) and np.array_equal(cd.counts(2), x["clean"][rows])
            assert cd.counts(0).tolist() == [7] * n
        finally:
            lib.skh_keyset_free(C.byref(dks))


# ---- every consumer form on the table that is 90 % full ---------------------------------------------------------------------------------
@pytest.mark.parametrize("odd_list_cap", [0, 3])
@pytest.mark.parametrize("pipeline", [1, 2])
@pytest.mark.parametrize("text_stage", [1, 0])
def test_full90_count_options(text_stage, pipeline, odd_list_cap):
    """scan_stream with the text stage and without, the single kernel and the partitioned pipeline, the byte-string kernel from
    its list and (odd_list_cap = 3: the list runs over) over every position"""
    x = _want("full90")
    w = x["w"]
    with _context(90, text_stage=text_stage, pipeline=pipeline, odd_list_cap=odd_list_cap) as c:
        c.load_keyset(x["ks"], 4)
        c.scan_stream(w.stream, 1)
        assert np.array_equal(c.counts(1), x["all"])


@pytest.mark.parametrize("lanes", [2, 1])
def test_full90_resident_batches_on_both_lanes(lanes):
    """scan_device: the batch with U windows and the clean one in turn, three times each -- with two lanes each lane sees both"""
    x = _want("full90")
    w = x["w"]
    with _context(90, scan_lanes=lanes) as c:
        c.load_keyset(x["ks"], 4)
        da, db = _resident(c, w.stream), _resident(c, w.stream_clean)
        for _ in range(3):
            c.scan_device(da, len(w.stream), 1)
        for _ in range(3):
            c.scan_device(db, len(w.stream_clean), 1)
            c.scan_device(da, len(w.stream), 1)
        assert np.array_equal(c.counts(1), 6 * x["all"] + 3 * x["clean"])


def test_full90_packed():
    """scan_pinned_packed of the reads without U windows, next to the same bytes unpacked"""
    x = _want("full90")
    w = x["w"]
    with _context(90) as c:
        c.load_keyset(x["ks"], 4)
        _scan_packed(c, w.stream_clean, 2)
        assert np.array_equal(c.counts(2), x["clean"])
    with _context(90, text_stage=0) as c:
        c.load_keyset(x["ks"], 4)
        _scan_packed(c, w.stream_clean, 2)
        assert np.array_equal(c.counts(2), x["clean"])


@pytest.mark.parametrize("name", ["full90", "wrap50"])
@pytest.mark.parametrize("text_stage", [1, 0])
def test_tally_forms(name, text_stage):
    """sk_tally_batch (single kernel, pipeline 2, a three-entry odd-chunk list) on all reads; a TallyBatch filled with bytes and
    filled packed, collected dense and sparse: tallies exactly, the log as a multiset and entry by entry against the oracle"""
    x, y = _want(name), _tally_want(name)
    w, o = x["w"], y["o"]
    with _context(w.load_pct, text_stage=text_stage) as c:
        c.load_keyset(x["ks"], 6)
        c.set_counts(0, _type_col(y["informative"]))
        t, h = c.tally_batch(w.stream, y["starts"], 0, 2)
        tr.check_single(o, w.stream, y["starts"], y["ref"], t, h, (name, "tally_batch"))
        for opt, val in (("pipeline", 2), ("odd_list_cap", 3)):
            c.set_option(opt, val)
            try:
                t, h = c.tally_batch(w.stream, y["starts"], 0, 2)
            finally:
                c.set_option(opt, 0)
            tr.check_single(o, w.stream, y["starts"], y["ref"], t, h, (name, opt, val))
        with TallyBatch(c) as b:
            for stream, starts, ref, packed in ((w.stream, y["starts"], y["ref"], False), (w.stream_clean, y["starts_clean"], y["ref_clean"], False),
                                                (w.stream_clean, y["starts_clean"], y["ref_clean"], True)):
                b.fill(stream, starts, packed=packed)
                c.tally_launch(b, 0, 2)
                t, h, n = c.tally_collect()
                assert n == len(h)
                tr.check_single(o, stream, starts, ref, t, h, (name, "launch+collect", packed))
                c.tally_launch(b, 0, 2)
                r, h, n = c.tally_collect_sparse()
                assert n == len(h) and len(np.unique(r[:, 0])) == len(r)
                t = np.zeros((len(starts), 2), dtype=np.uint32)
                t[r[:, 0]] = r[:, 1:]
                tr.check_single(o, stream, starts, ref, t, h, (name, "launch+sparse", packed))


# ---- 2^25 slots --------------------------------------------------------------------------------------------------------------------------
def test_sparse5_table_of_2_to_the_25_slots():
    """table_load_pct = 5 and 838,900 keys: the first slot takes the hash's low byte on top, and the crafted cluster wraps at
    2^25.  COUNT from bytes, resident on both lanes and packed, with the text stage and without; TALLY against the numpy reference"""
    t0 = time.perf_counter()
    x = _want("sparse5")
    w, ks = x["w"], x["ks"]
    t1 = time.perf_counter()
    starts = tr.starts_of(w.recs_clean)
    informative = np.arange(ks.nrows) % 3 == 0
    for k in w.crafted[::2]:
        informative[x["row_of"][int(k)]] = True
    want_tally = tr.canonical_tally(x["packed"], informative, w.stream_clean, starts)
    assert int(want_tally[0][:, 1].sum()) > 100
    t2 = time.perf_counter()
    for text_stage in (1, 0):
        with _context(5, text_stage=text_stage) as c:
            c.load_keyset(ks, 3)
            c.scan_stream(w.stream, 1)
            assert np.array_equal(c.counts(1), x["all"]), text_stage
            if text_stage:
                da = _resident(c, w.stream)
                c.scan_device(da, len(w.stream), 2)
                c.scan_device(da, len(w.stream), 2)
                _scan_packed(c, w.stream_clean, 2)
                assert np.array_equal(c.counts(2), 2 * x["all"] + x["clean"])
            c.set_counts(0, _type_col(informative))
            tl, h = c.tally_batch(w.stream_clean, starts, 0, 2)
            tr.check_exact(want_tally, tl, h, ("sparse5", text_stage))
    t3 = time.perf_counter()
    print(f"sparse5: world and oracle {t1 - t0:.2f} s, numpy reference {t2 - t1:.2f} s, on the card (two loads) {t3 - t2:.2f} s")


# ---- the byte-string index ---------------------------------------------------------------------------------------------------------------
def test_wide_index_wraps():
    """12 byte-string keys that all start in the last 4 slots of their 32-slot index: the keys in both orientations and either
    case, near misses, absent keys whose walk crosses the index's end -- COUNT (listed chunks and every position) and TALLY"""
    w = _craft.wide_wrap()
    ks = sk.Keyset.from_stream(w.sstream, initial_slots=_craft.CAP, default_val=1, incr=0)
    t = _oracle.OracleTable(capacity=_craft.CAP)
    assert t.build_stream(w.sstream) == 0
    t.scan_stream(w.stream, 1)
    okeys, ocounts = t.rows()
    t.close()
    assert ks.keys() == okeys and ks.nwide == 12
    want = ocounts[:, 1].astype(np.int64)
    wide_rows = [okeys.index(k) for k in w.keys]
    assert (want[wide_rows] >= 5).all() and want.sum() > want[wide_rows].sum() > 0
    o = tr.OracleStrain(w.sstream, capacity=_craft.CAP)
    assert o.keys == okeys
    informative = np.arange(o.nrows) % 4 == 0
    informative[wide_rows[::2]] = True
    informative[wide_rows[1::2]] = False
    starts = tr.starts_of(w.recs)
    ref = o.tally(w.stream, starts, informative)
    try:
        for cap in (0, 3):
            for text_stage in (1, 0):
                with _context(odd_list_cap=cap, text_stage=text_stage) as c:
                    c.load_keyset(ks, 6)
                    c.scan_stream(w.stream, 1)
                    assert np.array_equal(c.counts(1), want), (cap, text_stage)
                    c.set_counts(0, _type_col(informative))
                    tl, h = c.tally_batch(w.stream, starts, 0, 2)
                    tr.check_single(o, w.stream, starts, ref, tl, h, ("wide", cap, text_stage))
    finally:
        ks.close()


# ---- the union -----------------------------------------------------------------------------------------------------------------------------
def _same_as_member(t, h, s, own, what):
    wt, wh = own
    assert np.array_equal(t[:, s, :], wt), what
    mine = h[h[:, 0] == s][:, 1:]
    wh = wh[np.lexsort((wh[:, 1], wh[:, 0]))]
    assert np.array_equal(mine, wh), (what, len(mine), len(wh))


def test_union_of_members_with_clusters_at_the_tables_end():
    """four members, table_load_pct = 90 on the first (the union's 920 rows get 1024 slots), every member's crafted keys at the
    end of its own table and of the union's; shared keys, keys informative in one member only, absent keys through U windows.
    Members against the oracle; the union's tallies and log against the members' own; the union's COUNT against the oracle"""
    w = _craft.union_wrap()
    starts, starts_clean = tr.starts_of(w.recs), tr.starts_of(w.recs_clean)
    ctxs, sets, own, own_clean, counts = [], [], [], [], []
    try:
        for s, mw in enumerate(w.members):
            ks = sk.Keyset.from_stream(mw.sstream, initial_slots=_craft.CAP, default_val=1, incr=0)
            sets.append(ks)
            o = tr.OracleStrain(mw.sstream, capacity=_craft.CAP)
            assert ks.keys() == o.keys
            c = _context(90 if s == 0 else 50)
            ctxs.append(c)
            c.load_keyset(ks, 6)
            informative = np.arange(o.nrows) % 4 == 0
            for k in mw.crafted:
                informative[o.row_of[_craft.kmer_bytes(k)]] = int(k) in mw.informative_keys
            c.set_counts(0, _type_col(informative))
            ref = o.tally(w.stream, starts, informative)
            assert int(ref[0][:, 1].sum()) > 100
            t, h = c.tally_batch(w.stream, starts, 0, 2)
            tr.check_single(o, w.stream, starts, ref, t, h, ("member", s))
            own.append((t, h))
            own_clean.append(c.tally_batch(w.stream_clean, starts_clean, 0, 2))
            tt = _oracle.OracleTable(capacity=_craft.CAP)
            assert tt.build_stream(mw.sstream) == 0
            tt.scan_stream(w.stream, 2)
            counts.append(tt.counts()[:, 2].copy())
            tt.close()
        with sk.KmerUnion(ctxs, 0, 2) as u:
            assert u.rows == sum(k.nrows for k in sets) == 920
            forms = [("union", w.stream, starts, False, own), ("union packed", w.stream_clean, starts_clean, True, own_clean),
                     ("union bytes, clean", w.stream_clean, starts_clean, False, own_clean)]
            for name, stream, st, packed, want in forms:
                t, h = u.tally_batch(stream, st, packed=packed)
                for s in range(len(ctxs)):
                    _same_as_member(t, h, s, want[s], (name, s))
            u.set_option("odd_list_cap", 3)
            t, h = u.tally_batch(w.stream, starts)
            u.set_option("odd_list_cap", 0)
            for s in range(len(ctxs)):
                _same_as_member(t, h, s, own[s], ("union odd_list_cap=3", s))
            u.count_enable(1)
            u.scan_stream(w.stream, 0)
            u.fold_counts(0, 2)
            for s, c in enumerate(ctxs):
                assert np.array_equal(c.counts(2), counts[s]), s
    finally:
        for c in ctxs:
            c.close()
        for k in sets:
            k.close()


# ---- the level-1 filter's size -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _grid_world():
    rng = random.Random(5061)
    strain = _synth.rand_dna(rng, 45_000)
    strains = [strain[:20_000] + b"\n" + strain[20_000:], _synth.mutate(rng, strain[5_000:20_000], 0.02), _synth.rand_dna(rng, 10_000)]
    recs = _synth.fuzz_stream(rng, strain, 1500, p_junk=0.004, min_len=20, max_len=250).split(b"\n")[:-1]
    for _ in range(500):                                               # diverged reads, either strand
        a = rng.randrange(len(strain) - 200)
        r = _synth.mutate(rng, strain[a:a + rng.choice([64, 150, 200])], rng.choice([0.03, 0.1]))
        recs.append(_synth.revcomp(r) if rng.random() < 0.5 else r)
    for g in strains[1:]:
        for _ in range(150):
            a = rng.randrange(len(g) - 150)
            recs.append(g[a:a + 150])
    recs += [bytes(rng.choice(b"ACGTNRYU-. \r*acgtn") for _ in range(rng.randrange(0, 200))) for _ in range(200)]       # junk
    rng.shuffle(recs)
    stream = b"\n".join(recs) + b"\n"
    clean = stream.translate(_CLEAN)
    starts = tr.starts_of(recs)
    out = {"strains": strains, "stream": stream, "clean": clean, "starts": starts, "sets": [], "count": [], "count_clean": [], "tally": [], "informative": []}
    for g in strains:
        ks = sk.Keyset.from_stream(g + b"\n", default_val=1, incr=0)
        t = _oracle.OracleTable()
        assert t.build_stream(g + b"\n") == 0
        t.scan_stream(stream, 1)
        t.scan_stream(clean, 2)
        opacked, ocounts = _oracle_rows(t)
        t.close()
        assert np.array_equal(ks.packed(), opacked)
        informative = np.arange(ks.nrows) % 5 == 0
        out["sets"].append(ks)
        out["count"].append(ocounts[:, 1].astype(np.int64))
        out["count_clean"].append(ocounts[:, 2].astype(np.int64))
        out["informative"].append(informative)
        out["tally"].append(tr.canonical_tally(opacked, informative, clean, starts))
    assert out["count"][0].sum() > 50_000 and out["count"][1].sum() > 5_000 and out["count"][2].sum() > 5_000
    return out


@pytest.mark.parametrize("grid_kib", [1, 5, None, 65536])
def test_grid_geometry(grid_kib):
    """grid_kib = 1: the floor makes 4 KiB = 32,768 bits, into which the strain's 45 k 16-mers set four bits each -- all but a
    fraction of a per cent are set and nearly every chunk passes level 1; 5: 640 blocks, no power of two; the default; 65536:
    nearly empty.  COUNT from bytes and packed, TALLY, and a union of three
    members (its level-1 filter: the first member's grid_kib times three): the oracle's counts whatever the size"""
    g = _grid_world()
    ctxs = []
    try:
        for s, ks in enumerate(g["sets"]):
            c = sk.KmerContext(0)
            ctxs.append(c)
            if grid_kib is not None and s == 0:
                c.set_option("grid_kib", grid_kib)
            c.load_keyset(ks, 6)
            c.set_counts(0, _type_col(g["informative"][s]))
        c = ctxs[0]
        c.scan_stream(g["stream"], 1)
        _scan_packed(c, g["clean"], 2)
        assert np.array_equal(c.counts(1), g["count"][0]) and np.array_equal(c.counts(2), g["count_clean"][0])
        t, h = c.tally_batch(g["clean"], g["starts"], 0, 2)
        tr.check_exact(g["tally"][0], t, h, ("single", grid_kib))
        with sk.KmerUnion(ctxs, 0, 2) as u:
            for packed in (False, True):
                t, h = u.tally_batch(g["clean"], g["starts"], packed=packed)
                for s in range(len(ctxs)):
                    tr.check_exact(g["tally"][s], t[:, s, :], h[h[:, 0] == s][:, 1:], ("union", grid_kib, packed, s))
            u.count_enable(1)
            u.scan_stream(g["stream"], 0)
            u.fold_counts(0, 3)
            for s, m in enumerate(ctxs):
                assert np.array_equal(m.counts(3), g["count"][s]), (grid_kib, s)
    finally:
        for c in ctxs:
            c.close()


# ---- the partitioned pipeline's bins -----------------------------------------------------------------------------------------------------
def test_bins_segment_overflow_and_the_no_entry_word():
    """pipeline = 2: a bin tile of 4096 equal chunks (one partition, a segment of 40: the rest must arrive as candidates unasked),
    and the chunk whose entry would equal the "no entry" word 0xFFFFFFFF (chunk 4095, 20 key bits all ones) inside a read that
    hits -- the oracle's counts, and the single kernel's on the same bytes; TALLY against the numpy reference"""
    w = _craft.bins()
    ks = sk.Keyset.from_stream(w.sstream, default_val=1, incr=0)
    t = _oracle.OracleTable()
    assert t.build_stream(w.sstream) == 0
    t.scan_stream(w.stream, 1)
    opacked, ocounts = _oracle_rows(t)
    t.close()
    assert np.array_equal(ks.packed(), opacked)
    want = ocounts[:, 1].astype(np.int64)
    repeat_rows = np.nonzero(want > 1000)[0]
    assert len(repeat_rows) == 16 and want[repeat_rows].sum() == len(w.recs[w.repeat_index]) - 30
    starts = tr.starts_of(w.recs)
    informative = np.arange(ks.nrows) % 2 == 0
    want_tally = tr.canonical_tally(opacked, informative, w.stream, starts)
    # the 16 windows whose whole chunk is chunk 4095 of the first tile lie inside the read and hit
    assert int(want_tally[0][w.read_index, 0]) == len(w.recs[w.read_index]) - 30
    got = {}
    try:
        for pipeline in (2, 1):
            for text_stage in (1, 0):
                with _context(pipeline=pipeline, text_stage=text_stage) as c:
                    c.load_keyset(ks, 4)
                    c.scan_stream(w.stream, 1)
                    got[pipeline, text_stage] = c.counts(1)
                    assert np.array_equal(got[pipeline, text_stage], want), (pipeline, text_stage)
                    c.set_counts(0, _type_col(informative))
                    tl, h = c.tally_batch(w.stream, starts, 0, 2)
                    tr.check_exact(want_tally, tl, h, ("bins", pipeline, text_stage))
        assert np.array_equal(got[2, 1], got[1, 1])
    finally:
        ks.close()


# ---- the options' ranges -------------------------------------------------------------------------------------------------------------------
def test_option_ranges():
    """table_load_pct 4 and 91, grid_kib 0 and -2: SK_E_ARG, the option keeps its value, and a later load counts as ever"""
    x = _want("full90")
    w = x["w"]
    with _context(90) as c:
        c.set_option("grid_kib", 5)
        for name, value in (("table_load_pct", 4), ("table_load_pct", 91), ("grid_kib", 0), ("grid_kib", -2)):
            with pytest.raises(sk.SKError) as e:
                c.set_option(name, value)
            assert e.value.code == SK_E_ARG, (name, value)
        c.load_keyset(x["ks"], 4)
        c.scan_stream(w.stream, 1)
        assert np.array_equal(c.counts(1), x["all"])
        for name, value in (("table_load_pct", 5), ("table_load_pct", 90), ("grid_kib", 1), ("grid_kib", 1 << 22), ("grid_kib", -1)):
            c.set_option(name, value)                                  # the ends of the ranges are accepted
        c.load_keyset(x["ks"], 4)                                      # (90 again: the same 1024 slots)
        c.scan_stream(w.stream, 2)
        assert np.array_equal(c.counts(2), x["all"])
