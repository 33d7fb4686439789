"""The premises of tests/test_hash_worlds_gpu.py, on the CPU: every crafted world is what it claims to be.  The key search and
the model of a table filled by linear probing (tests/_craft.py, tests/native/hash_craft.c) use the library's own hash functions,
and these are conditions on the inputs, for seeds fixed in tests/_craft.py: should a hash ever change, they fail instead of
letting the GPU tests turn into ordinary random ones."""
import ctypes as C
import os
import random

import numpy as np
import pytest

import _craft
import _synth
import strainer2_amd as sk

NONE = np.uint64(sk.native.SK_KEY_NONE)


def test_model_on_a_table_small_enough_to_do_by_hand():
    """8 slots; keys start at 6, 7, 7, 7, 2: they rest at 6, 7, 0, 1, 2"""
    m = _craft.Model([6, 7, 7, 7, 2], 8)
    assert m.final.tolist() == [6, 7, 0, 1, 2] and m.wrapped.tolist() == [False, False, True, True, False]
    ln, wr = m.present_walks()
    assert ln.tolist() == [1, 1, 2, 3, 1] and wr.tolist() == [False, False, True, True, False]
    ln, wr = m.walk([6, 7, 0, 3, 2])                                   # absent keys: to the first empty slot, 3
    assert ln.tolist() == [6, 5, 4, 1, 2] and wr.tolist() == [True, True, False, False, False]
    same = _craft.Model([7, 2, 7, 6, 7], 8)                            # another order: the same slots, as many keys wrapped
    assert sorted(np.nonzero(same.table)[0]) == sorted(np.nonzero(m.table)[0]) and same.wrapped.sum() == m.wrapped.sum()


def test_crafted_keys_are_what_was_asked_for():
    keys = _craft.craft_keys(1, 20, (1 << 20) - 16, (1 << 20) - 1, 24, need_u=True)
    assert len(set(keys.tolist())) == 24
    assert (_craft.slot0(keys, 20) >= (1 << 20) - 16).all()
    ok, tmask = _craft.u_info(keys)
    assert ok.all()
    rng = random.Random(1)
    for k, tm in zip(keys.tolist(), tmask.tolist()):
        w = _craft.kmer_bytes(k)
        assert _craft.pack(w) == k and w >= _synth.revcomp(w)          # canonical
        u = _synth.u_window_of(rng, w)
        assert u and len(u) == 31
        i = u.upper().index(b"U")
        assert tm >> i & 1 and _synth.revcomp(w)[:i] + b"T" + _synth.revcomp(w)[i + 1:] == _synth.revcomp(w)
    plain = _craft.craft_keys(2, 10, 1000, 1023, 50)
    assert ((_craft.slot0(plain, 10) >= 1000)).all()
    assert all(_craft.kmer_bytes(k) >= _synth.revcomp(_craft.kmer_bytes(k)) for k in plain.tolist())
    assert _synth.u_window_of(rng, b"A" * 31) is None and _synth.u_window_of(rng, b"ACGN" + b"A" * 27) is None


def _keyset(sstream, small=True):
    return sk.Keyset.from_stream(sstream, initial_slots=_craft.CAP, default_val=1, incr=0) if small else sk.Keyset.from_stream(sstream, default_val=1, incr=0)


def _table_premises(keys, lg, load_pct, absent, what):
    """the list of tests/test_hash_worlds_gpu.py's premises, on the model of the table that holds `keys`"""
    keys = np.asarray(keys, dtype=np.uint64)
    assert _craft.slots_log2(len(keys), load_pct) == lg, what          # the slot count the library picks
    assert not set(absent.tolist()) & set(keys.tolist()), what
    m = _craft.Model(_craft.slot0(keys, lg), 1 << lg)
    assert int(m.wrapped.sum()) >= 64, (what, "present keys that rest below their first slot", int(m.wrapped.sum()))
    ln, wr = m.present_walks()
    assert np.array_equal(wr, m.wrapped)
    assert int(ln.max()) >= 128, (what, "longest walk of a present key", int(ln.max()))
    aln, awr = m.walk(_craft.slot0(absent, lg))
    assert int(awr.sum()) >= 32, (what, "absent queries that walk across the end", int(awr.sum()))
    assert int((aln[awr] >= 128).sum()) >= 8, (what, "of those, walks of 128 slots or more", int((aln[awr] >= 128).sum()))
    return m


@pytest.mark.parametrize("name", ["wrap50", "full90", "sparse5"])
def test_table_world_premises(name):
    w = getattr(_craft, name)()
    ks = _keyset(w.sstream, small=name != "sparse5")
    try:
        keys = ks.packed()
        assert ks.nrows == w.nkeys and ks.nwide == 0 and not (keys == NONE).any()
        # as many window starts as keys: the builder on the device, which sizes by the starts, picks the same table
        assert sum(len(r) - 30 for r in w.strain_recs) == w.nkeys
        assert set(w.crafted.tolist()) <= set(keys.tolist())
        n = 1 << w.lg
        assert (_craft.slot0(w.crafted, w.lg) >= n - w.width).all() and (_craft.slot0(w.absent, w.lg) >= n - w.width).all()
        if name == "full90":
            assert w.lg == 10 and ks.nrows / n >= 0.89
            assert _craft.slots_log2(ks.nrows + 1, 90) == 11            # (one key more and the table doubles)
        if name == "wrap50":
            assert w.lg == 10 and w.load_pct == 50
        if name == "sparse5":
            assert w.lg == 25 and _craft.slots_log2(ks.nrows, 50) < 25
            # slots that bits 8..31 of the hash alone (24 bits) cannot address: the hash's low byte on top put the keys there
            assert (_craft.slot0(w.crafted, w.lg) >= 1 << 24).all() and (_craft.slot0(w.absent, w.lg) >= 1 << 24).all()
        _table_premises(keys, w.lg, w.load_pct, w.absent, name)
        assert _craft.u_info(w.absent)[0].all()
    finally:
        ks.close()
    # the reads: both forms, the packable one without a byte for the byte-string kernel
    assert len(w.recs) > len(w.recs_clean) >= 2 * len(w.key_recs) and len(w.recs) < 5000
    assert not sk.pack_stream(w.stream_clean)[1] and sk.pack_stream(w.stream)[1]


def test_union_world_premises():
    w = _craft.union_wrap()
    rows, union_keys = 0, set()
    for s, mw in enumerate(w.members):
        ks = _keyset(mw.sstream)
        try:
            keys = ks.packed()
            assert ks.nrows == mw.nkeys == sum(len(r) - 30 for r in mw.strain_recs) and ks.nwide == 0
            assert set(mw.crafted.tolist()) <= set(keys.tolist()) and mw.informative_keys <= set(keys.tolist())
            # a member's own table: 1024 slots whatever its load option
            for pct in (50, 90):
                _table_premises(keys, 10, pct, w.absent, ("member", s, pct))
            rows += ks.nrows
            union_keys |= set(keys.tolist())
        finally:
            ks.close()
    assert _craft.slots_log2(rows, 90) == w.lg == 10 and _craft.slots_log2(rows, 50) == 11       # (the first member's 90 makes the difference)
    uk = np.array(sorted(union_keys), dtype=np.uint64)
    m = _craft.Model(_craft.slot0(uk, w.lg), 1 << w.lg)
    assert int(m.wrapped.sum()) >= 64 and int(m.present_walks()[0].max()) >= 128
    aln, awr = m.walk(_craft.slot0(w.absent, w.lg))
    assert int(awr.sum()) >= 32 and int((aln[awr] >= 128).sum()) >= 8 and not set(w.absent.tolist()) & union_keys
    # sharing: one key in every member, the pairs in two, and keys informative in one member of those that hold them
    holds = lambda k: [s for s, mw in enumerate(w.members) if k in set(mw.crafted.tolist())]   # noqa: E731
    assert holds(w.all_key) == list(range(_craft.UNION_MEMBERS))
    for s in range(_craft.UNION_MEMBERS):
        k = int(w.pair[s][0])
        assert holds(k) == sorted({s, (s + 1) % _craft.UNION_MEMBERS})
        assert [k in mw.informative_keys for mw in w.members].count(True) == 1
        assert holds(int(w.own[s][0])) == [s]


def test_wide_world_premises():
    w = _craft.wide_wrap()
    ks = sk.Keyset.from_stream(w.sstream, initial_slots=_craft.CAP, default_val=1, incr=0)
    try:
        assert ks.nwide == len(w.keys) == 12
        raw = C.string_at(ks._s.wide_keys, 32 * ks.nwide)
        stored = [raw[32 * i:32 * i + 31] for i in range(ks.nwide)]    # (in the order the index is filled in)
        assert sorted(stored) == sorted(w.keys), "the library stores the crafted byte-string keys in another orientation"
        assert sorted(ks.key(int(r)) for r in np.nonzero(ks.packed() == NONE)[0]) == sorted(w.keys)
    finally:
        ks.close()
    lg = 4
    while (1 << lg) < len(stored) * 2:                                 # sk_table_load_wide's sizing
        lg += 1
    assert (1 << lg) == w.wmask + 1 == 32
    first = _craft.wide_slot0(stored, w.wmask)
    assert (first >= w.lo).all()
    m = _craft.Model(first, w.wmask + 1)
    assert int(m.wrapped.sum()) >= 4, int(m.wrapped.sum())
    assert not set(w.absent) & set(stored)
    aln, awr = m.walk(_craft.wide_slot0(w.absent, w.wmask))
    assert awr.any() and int(aln.max()) > int(m.wrapped.sum())
    assert all(k in w.recs for k in w.keys + w.absent)
    for k in w.keys + w.absent:                                        # IUPAC letters only: nothing here is a key of the 2-bit table
        assert set(k) & set(_craft.WIDE_LETTERS) and set(k) <= set(b"ACGT" + _craft.WIDE_LETTERS)


def test_bins_world_premises():
    w = _craft.bins()
    T = _craft.BIN_TILE
    key, part = _craft.bin16_of(w.x16)
    assert key == _craft.BIN_NO_ENTRY_KEY == (1 << 20) - 1 and part == w.x_part
    assert ((T // 16 - 1) << 20 | key) == 0xFFFFFFFF                   # chunk 4095 with that key: the "no entry" word
    assert _craft.bin16_of(_synth.revcomp(w.x16)) == (key, part)       # (either strand: the canonical 16-mer is hashed)
    assert w.stream[T - 16:T] == w.x16 and w.x16 in w.strain_recs[0]
    starts = np.cumsum([0] + [len(r) + 1 for r in w.recs[:-1]])
    s = int(starts[w.read_index])
    assert s <= T - 16 - 30 and s + len(w.recs[w.read_index]) >= T + 30 and w.recs[w.read_index] in w.strain_recs[0]
    # the third tile holds nothing but the repeat: 4096 equal chunks, one partition, a segment of 40
    tile = w.stream[2 * T:3 * T]
    assert int(starts[w.repeat_index]) <= 2 * T and set(tile[i:i + 16] for i in range(0, T, 16)) == {tile[:16]}
    assert tile[:16] in w.unit * 2 and len({w.unit[i:] + w.unit[:i] for i in range(16)}) == 16
    assert w.strain_recs[1] == w.unit * 4


def test_the_helper_restates_no_hash():
    """the search calls sk_common.h's functions; none of their multipliers stands in the helper or beside it"""
    for name in ("native/hash_craft.c", "_craft.py", "test_hash_worlds_gpu.py"):
        text = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), name)).read().upper()
        for const in ("9E3779B", "85EBCA7", "1677761", "5BD1E99", "C2B2AE3", "27D4EB2"):
            assert const not in text, (name, const)
    assert '#include "../../strainer2_amd/csrc/sk_common.h"' in open(_craft.SRC).read()
