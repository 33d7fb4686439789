"""Rarefaction (include/strainer_kmer.h has the rule) without a device: the model (tests/_rarefaction_model.py) on known values, the
library's parser, draw and class against it, the premises of the worlds tests/test_coverage_rarefaction_gpu.py runs in -- checked on the
model alone, so that a kernel which ignores the class cannot pass there -- and the host side (strainer2_amd/csrc/sk_host_rarefaction.c)
driven by tests/native/rarefaction_check.c as a stand-alone program under AddressSanitizer + UBSan."""
import os
import subprocess

import numpy as np
import pytest

import _rarefaction_model as rm
from strainer2_amd import native

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
EDGE = 1 << 32

# u(i) at seed 0 is the 32-bit finalizer of MurmurHash3 (public domain) applied to i's low word xor the high word times 0x9E3779B9:
# fmix32(1) = 0x514E28B7 and fmix32(0) = 0 are its published values; i = 2^32 is fmix32(0x9E3779B9), i = 2^32 + 1 fmix32(0x9E3779B8)
KNOWN = [(0, 0, 0x00000000), (1, 0, 0x514E28B7), (EDGE, 0, 0x92CA2F0E), (0x9E3779B9, 0x9E3779B9, 0x00000000), (1, 1, 0x00000000),
         (0x9E3779B9 ^ 1, 0x9E3779B9, 0x514E28B7), (EDGE + 0x9E3779B9, 0, 0x00000000), (EDGE + 1, 0x9E3779B8, 0x00000000)]
BAD_LISTS = ["", ",", "1,", ",1", "1,,0.5", "0.5,0.5", "0.25,0.5", "1,0.5,0.75", "1.5", "1.0000001", "0", "0.0", "-0.5", "+0.5", " 0.5", "0.5 ",
             "abc", "0x1p-1", "nan", "inf", "1e", "e5", "1e-400", ".", "1..5", "0.5f", "1;0.5",
             "1,1e-10,1e-11",                                  # two fractions with T = 0
             "0.50000000001,0.5",                              # two fractions with equal T
             "0." + "0" * 40 + "1",                            # a field of more than 39 characters
             ",".join("%g" % (1.0 / (k + 1)) for k in range(17))]
GOOD_LISTS = [None, "1", "0.5", "1.", ".5", "1e0", "5E-1", "1,0.1,1e-9", "1.0,0.50,0.25", ",".join("%g" % (1.0 / (k + 1)) for k in range(16)),
              "1,1e-10"] + rm.LISTS


def test_the_draw_at_known_values():
    for i, seed, u in KNOWN:
        assert rm.draw(i, seed) == u, (i, seed)
        assert native.lib.skh_rarefaction_draw(i, seed) == u, (i, seed)
    assert rm.draw(EDGE, 0) != rm.draw(0, 0) and rm.draw((1 << 64) - 1, 5) == rm.draw((1 << 64) - 1, 5) < EDGE
    i = np.array([0, 1, EDGE - 1, EDGE, EDGE + 1, (1 << 64) - 1, 123456789012345], dtype=np.uint64)
    for seed in rm.SEEDS + [1]:
        assert rm.draws(i, seed).tolist() == [rm.draw(int(x), seed) for x in i]
        assert [native.lib.skh_rarefaction_draw(int(x), seed) for x in i] == [rm.draw(int(x), seed) for x in i]


def test_thresholds_of_fractions():
    assert rm.threshold("1") == 4294967296 and rm.threshold("0.5") == 2147483648
    assert rm.threshold("0.1") == 429496729                    # floor(429496729.6)
    assert rm.threshold("1e-9") == 4                           # floor(4.294967296)
    assert rm.parse_list(None)[0] == [EDGE >> k for k in range(6)]


def test_the_parsers_agree_and_refuse_the_same_lists():
    for text in GOOD_LISTS:
        T, fields = rm.parse_list(text)
        assert native.rarefaction_parse(text) == (T, fields), text
        assert all(a > b for a, b in zip(T, T[1:])) and T[0] <= EDGE
    for text in BAD_LISTS:
        with pytest.raises(ValueError):
            rm.parse_list(text)
        with pytest.raises(native.SKError) as e:
            native.rarefaction_parse(text)
        assert e.value.code == -3, text


def test_class_and_keep_rule():
    T, _ = rm.parse_list("1,0.5,0.25")
    r = native.RarefactionList()
    assert native.lib.skh_rarefaction_parse(b"1,0.5,0.25", 9, r) == 0
    seen = set()
    for i in list(range(300)) + [EDGE - 1, EDGE, EDGE + 1, (1 << 64) - 1]:
        c = rm.klass(i, T, 9)
        assert c == sum(rm.keep(i, t, 9) for t in T) == native.lib.skh_rarefaction_class(r, i) >= 1
        assert [rm.keep(i, t, 9) for t in T] == [True] * c + [False] * (3 - c)      # nested: subsamples 0 .. class - 1
        seen.add(c)
    assert seen == {1, 2, 3}
    assert rm.classes(np.arange(300, dtype=np.uint64), T, 9).tolist() == [rm.klass(i, T, 9) for i in range(300)]


def test_subsample_keeps_pairs_whole_and_in_order():
    recs = [b"r%d" % k for k in range(41)]
    t = rm.threshold("0.5")
    pei = rm.subsample([recs], "PEI", t, 3)[0]
    assert pei == [r for k, r in enumerate(recs) if rm.keep(k // 2, t, 3)] and 0 < len(pei) < 41
    assert rm.npairs([recs], "PEI") == 21 and rm.npairs([recs], "SE") == 41 and rm.npairs([recs, recs[:40]], "PE") == 41
    a, b = rm.subsample([recs, recs[:40]], "PE", t, 3)
    assert a[: len(b)] == b and len(a) - len(b) == rm.keep(40, t, 3)       # the mate files stay in step; the last pair has no mate
    assert rm.subsample([recs], "SE", rm.threshold("1"), 0) == [recs]


def test_table_on_a_hand_made_list():
    T, seed = rm.parse_list("1,0.5")[0], 0
    inn = [i for i in range(40) if rm.klass(i, T, seed) == 2][:2]
    out = [i for i in range(40) if rm.klass(i, T, seed) == 1][:2]
    lines = [(inn[0], 7, 9), (inn[0], 8, 9), (out[0], 7, 9), (out[1], 3, 9), (inn[1], 5, 1)]      # the last does not pass min_hits = 1
    assert rm.table(lines, T, seed, 1, inn + out) == ([4, 2], [3, 2], [4, 2])
    assert rm.table([], T, seed, 1, inn + out) == ([4, 2], [0, 0], [0, 0])


@pytest.mark.parametrize("seed", rm.SEEDS)
@pytest.mark.parametrize("which", range(len(rm.LISTS)))
def test_premises_of_the_library_world(which, seed):
    """for the fractions and seeds the GPU tests use: every subsample holds a pair that carries a counted line, adjacent subsamples
    differ in unique, and some row has its only counted lines in pairs outside the smallest subsample"""
    T, _ = rm.parse_list(rm.LISTS[which])
    entries, ranges = rm.library_world(which)
    ords = rm.world_ordinals(ranges)
    assert sorted(len(e[0]) == 0 for e in entries) == [False] * 4 + [True]
    rows, totals, o = entries[4]
    assert (o < 700).any() and (o == EDGE - 1).any() and (o == EDGE).any() and (o > np.uint64(1 << 63)).any()
    pairs, uq, tot = rm.table(np.stack([o, rows.astype(np.uint64), totals.astype(np.uint64)], axis=1), T, seed, rm.MIN_HITS, ords)
    assert tot[-1] > 0 and pairs[-1] > 0
    assert all(a > b for a, b in zip(uq, uq[1:])) and all(a > b for a, b in zip(pairs, pairs[1:]))
    counted = len(np.unique(rows[totals.astype(np.int64) > rm.MIN_HITS]))
    if T[-1] < EDGE:                                           # (the list "1" has no pair outside its smallest subsample)
        assert uq[-1] < counted
    assert (totals == rm.MIN_HITS).any() and tot[0] < len(rows)


# ---------------------------------------------------------------------------------------------------------------------------------
# the host side as a stand-alone program under the sanitizers
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("rar") / "rarefaction_check")
    subprocess.run(["gcc"] + SAN + [os.path.join(REPO, "tests", "native", "rarefaction_check.c"), "-o", exe], check=True)
    return exe


def _run(checker, *args):
    p = subprocess.run([checker] + [str(a) for a in args], env=ENV, capture_output=True)
    assert b"runtime error" not in p.stderr and b"AddressSanitizer" not in p.stderr and b"LeakSanitizer" not in p.stderr, p.stderr.decode()[-2000:]
    return p


def test_checker_parser_and_draw(checker):
    for text in GOOD_LISTS:
        p = _run(checker, "parse", "-" if text is None else text, 0)
        assert p.returncode == 0, text
        T, fields = rm.parse_list(text)
        assert p.stdout.decode().split("\n")[:-1] == ["T %d" % len(T)] + ["%d %s" % (t, f) for t, f in zip(T, fields)]
    for text in BAD_LISTS:
        assert _run(checker, "parse", text, 0).returncode == 3, text
    ii = [0, 1, EDGE - 1, EDGE, EDGE + 1, (1 << 64) - 1]
    p = _run(checker, "draw", 77, *ii)
    assert p.returncode == 0 and p.stdout.decode().split() == [str(rm.draw(i, 77)) for i in ii]


@pytest.mark.parametrize("lst,seed,mh,nrows,first,npairs,nlines", [
    (None, 0, 0, 50, 0, 400, 3000), ("1", 5, 1, 1, EDGE - 10, 20, 50), ("0.75,0.1", 0x9E3779B9, 2, 257, EDGE - 200, 1000, 20000),
    (rm.LISTS[3], 1, 5, 1000, (1 << 64) - 600, 600, 5000), ("0.5", 0, 0, 10, 7, 0, 0), ("1,0.5", 3, 0, 0, 0, 9, 5)])
def test_checker_fold_and_table_against_the_model(checker, tmp_path, lst, seed, mh, nrows, first, npairs, nlines):
    out = tmp_path / "table"
    p = _run(checker, "fold", "-" if lst is None else lst, seed, mh, nrows, first, npairs, nlines, 4242, out)
    assert p.returncode == 0, p.stderr.decode()[-1000:]
    lines = [tuple(int(x) for x in l.split()) for l in p.stdout.decode().split("\n") if l]
    assert len(lines) == nlines
    T, fields = rm.parse_list(lst)
    pairs, uq, tot = rm.table(lines if nrows else [], T, seed, mh, np.arange(npairs, dtype=np.uint64) + np.uint64(first))
    body = b"".join(b"m0.fq\t%s\t%d\t%d\t%d\n" % (f.encode(), a, b, c) for f, a, b, c in zip(fields, pairs, uq, tot))
    named = b"".join(b"Genus_species_s0\t" + l + b"\n" for l in body.split(b"\n")[:-1])
    assert out.read_bytes() == rm.HEADER + body + b"strain_name\t" + rm.HEADER + named
    if nlines >= 3000:
        assert tot[0] > tot[-1] > 0 or len(T) == 1
