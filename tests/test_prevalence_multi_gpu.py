"""Prevalence for many strains from one pass (kmer_scrub_count -S --prevalence=SUFFIX): the union item fold on the device
(sk_union_item_fold on the item slots of a union's context) against the CPU oracle of each member ALONE, scanned item by item
(tests/_prevalence_multi_worlds.py); and the program: every strain's prevalence table and item records against the model
(tests/_prevalence_model.py, the oracle item by item) and the single-strain program, under every plan of unions and every submit path
of the list walk; scrub by prevalence.  The ground truth is never the code under test.

The progress file holds a time stamp per line: it is compared with the time column taken out, everything else byte for byte."""
import gzip
import os
import random
import re
import subprocess

import numpy as np
import pytest

import _prevalence_model as model
import _prevalence_multi_worlds as worlds
import _synth
import strainer2_amd as sk
from strainer2_amd.native import lib

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(REPO, "strainer2_amd", "bin")
EXE = sk.cli_path()
BIG = 10 ** 6                                               # a min_count above every count of these worlds


# ---------------------------------------------------------------------------------------------------------- the device API
def _masks(nm):
    """all members; proper subsets (one without member 0, whose rows are the shared keys' slot rows, and with the last member --
    bit 31 of a full union; one of member 0 alone); nobody"""
    full = (1 << nm) - 1
    out = [full]
    for m in (0xAAAAAAAA & full | 1 << (nm - 1), 1):
        if m != full and m not in out:
            out.append(m)
    return out + [0]


def _records(ctx, ptr, nm):
    return ctx.dev_download(ptr, 16 * nm).view(np.uint64).reshape(nm, 2)


def _want_records(vs, mask, m):
    return np.array([[int((v >= m).sum()), int(v.astype(np.uint64).sum())] if (mask >> s) & 1 else [0, 0] for s, v in enumerate(vs)], dtype=np.uint64)


class _Union:
    """the members' contexts with their tables (four columns), the union with one count column and two item slots"""

    def __init__(self, w):
        self.w = w
        self.sets = [sk.Keyset.from_stream(s + b"\n") for s in w.strains]
        self.ctxs = [sk.KmerContext(0) for _ in self.sets]
        self.u = None
        try:
            for c, ks, keys in zip(self.ctxs, self.sets, w.keys):
                c.load_keyset(ks, 4)
                assert ks.keys() == keys, "row order differs from the oracle"
            self.u = sk.KmerUnion(self.ctxs)
            assert self.u.rows == w.base[-1]
            self.u.count_enable(1)
            self.u.item_slots(2)
        except BaseException:
            self.close()
            raise

    def close(self):
        if self.u is not None:
            self.u.close()
        for c in self.ctxs:
            c.close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


def _scan(U, data, via, held):
    if via == "stream":
        U.u.scan_stream(data, 0)
        return
    buf = np.frombuffer(data + b"\n" * ((-len(data)) % 16 + 16), dtype=np.uint8)       # (a resident batch: the two scan lanes take turns)
    p = U.ctxs[0].dev_alloc(buf.size)
    U.ctxs[0].dev_upload(p, buf)
    U.u._uck(lib.sk_scan_device(U.u.context_handle, p, len(data), 0))
    held.append(p)


def _round(U, mask, m, via="stream"):
    """one pending scan into the union's own column, then A1, B1, A2, B2 into slots 0 and 1 in turn; fold A, then B, into the members
    of `mask`; fold the emptied slots again into everybody; the union's own column last"""
    w, u, ctxs = U.w, U.u, U.ctxs
    nm = len(ctxs)
    rng = np.random.default_rng(1000 * nm + 10 * (mask % 97) + min(m, 9))
    base_c = [rng.integers(2 ** 32 - 50, 2 ** 32, r, dtype=np.uint64).astype(np.uint32) for r in w.rows]      # the fold ADDS, mod 2^32
    base_p = [rng.integers(0, 1000, r, dtype=np.uint64).astype(np.uint32) for r in w.rows]
    other = [rng.integers(0, 2 ** 32, r, dtype=np.uint64).astype(np.uint32) for r in w.rows]
    for s, c in enumerate(ctxs):
        c.set_counts(1, base_c[s])
        c.set_counts(2, base_p[s])
        c.set_counts(3, other[s])
    rec = ctxs[0].dev_alloc(3 * 16 * nm)
    ctxs[0].dev_upload(rec, np.zeros(3 * 2 * nm, dtype=np.uint64))
    held = []
    try:
        u.scan_stream(w.chunks_a[0], 0)                     # no slot set: into the union column it names, as ever (pending until its own fold)
        for i in range(2):
            for slot, chunks in ((0, w.chunks_a), (1, w.chunks_b)):
                u.item_slot(slot)
                _scan(U, chunks[i], via, held)
        u.item_slot(-1)
        u.sync()
        for s, c in enumerate(ctxs):
            assert np.array_equal(c.counts(1), base_c[s]), "a slot scan leaves the members alone until the fold"
        u.item_fold(0, 1, 2, mask, m, rec)
        u.sync()
        for s, c in enumerate(ctxs):
            on = (mask >> s) & 1
            assert np.array_equal(c.counts(1), base_c[s] + w.va[s] * np.uint32(on)), (s, "count after item a")
            assert np.array_equal(c.counts(2), base_p[s] + (w.va[s] >= m) * np.uint32(on)), (s, "prevalence after item a")
        u.item_fold(1, 1, 2, mask, m, rec + 16 * nm)
        u.sync()
        want_c = [base_c[s] + (w.va[s] + w.vb[s]) * np.uint32((mask >> s) & 1) for s in range(nm)]
        want_p = [base_p[s] + ((w.va[s] >= m).astype(np.uint32) + (w.vb[s] >= m)) * np.uint32((mask >> s) & 1) for s in range(nm)]
        for s, c in enumerate(ctxs):
            assert np.array_equal(c.counts(1), want_c[s]), (s, "count")
            assert np.array_equal(c.counts(2), want_p[s]), (s, "prevalence")
        assert np.array_equal(_records(ctxs[0], rec, nm), _want_records(w.va, mask, m))
        assert np.array_equal(_records(ctxs[0], rec + 16 * nm, nm), _want_records(w.vb, mask, m))
        # both slots are zero, for the members outside the mask too: folding them again, into everybody, changes nothing
        u.item_fold(0, 1, 2, None, 1, rec + 32 * nm)
        u.item_fold(1, 1, 2, None, 1, rec + 32 * nm)
        u.sync()
        for s, c in enumerate(ctxs):
            assert np.array_equal(c.counts(1), want_c[s]) and np.array_equal(c.counts(2), want_p[s]), s
            assert np.array_equal(c.counts(3), other[s]), (s, "a third column")
            assert np.array_equal(c.counts(0), U.sets[s].first_count()), s
        assert not _records(ctxs[0], rec + 32 * nm, nm).any()
        # the union's own column and its pending increments were left alone: the first scan arrives where it always did
        u.fold_counts(0, 3)
        for s, c in enumerate(ctxs):
            assert np.array_equal(c.counts(3), other[s] + w.va1[s]), (s, "the union's own column")
            assert np.array_equal(c.counts(1), want_c[s]) and np.array_equal(c.counts(2), want_p[s]), s
        assert not u.counts(0).any()
    finally:
        u.sync()
        for p in held + [rec]:
            ctxs[0].dev_free(p)


@pytest.mark.parametrize("min_count", [1, 2, BIG])
@pytest.mark.parametrize("name", worlds.NAMES)
def test_union_fold_equals_each_member_alone(name, min_count):
    w = worlds.world(name)
    with _Union(w) as U:
        for mask in _masks(len(w.strains)):
            _round(U, mask, min_count)


@pytest.mark.parametrize("name", ["4096", "8193"])
def test_resident_batches_on_both_scan_lanes_into_union_slots(name):
    w = worlds.world(name)
    with _Union(w) as U:
        for mask in _masks(len(w.strains))[:2]:
            _round(U, mask, 2, via="device")


def test_union_fold_calls_are_checked():
    w = worlds.world("4095")
    sets = [sk.Keyset.from_stream(s + b"\n") for s in w.strains[:3]]
    ctxs = [sk.KmerContext(0) for _ in sets]
    try:
        for c, ks, ncols in zip(ctxs, sets, (4, 4, 2)):
            c.load_keyset(ks, ncols)
        with sk.KmerUnion(ctxs) as u:
            with pytest.raises(sk.SKError):
                u.item_slots(1)                             # no count columns yet
            with pytest.raises(sk.SKError) as e:
                u.item_fold(0, 0, 1)
            assert e.value.code == sk.native.SK_E_STATE
            u.count_enable(1)
            with pytest.raises(sk.SKError):
                u.item_slot(0)                              # nothing allocated unless asked for
            with pytest.raises(sk.SKError):
                u.item_fold(0, 0, 1)
            u.item_slots(2)
            for bad in (lambda: u.item_fold(2, 0, 1), lambda: u.item_fold(0, 1, 1), lambda: u.item_fold(0, 0, 1, min_count=0),
                        lambda: u.item_fold(0, 0, 1, member_mask=0b1000), lambda: u.item_fold(0, 1, 2, member_mask=0b100),
                        lambda: u.item_fold(0, 1, 4, member_mask=0b001), lambda: u.item_fold(0, 0, 1, records=12)):
                with pytest.raises(sk.SKError):
                    bad()
            u.item_fold(0, 1, 2, member_mask=0b011)         # member 2's missing columns do not matter while it is masked out
            u.item_fold(0, 0, 1, member_mask=0)
            u.sync()
            u.item_slots(0)
            with pytest.raises(sk.SKError):
                u.item_slot(0)
    finally:
        for c in ctxs:
            c.close()


# ---------------------------------------------------------------------------------------------------------- the program
# (the refusals need no device: tests/test_prevalence_multi_host.py)
FLAGS = ["--prevalence=.prev.tsv", "--prevalence-items=.items.tsv", "--prevalence-min-count", "2"]
LISTS = ["-A", "A.txt", "-B", "B.txt", "-C", "C.txt"]


class _Panel:
    pass


def _make_panel(tmp_path_factory, name, seed, nstrains):
    p = _Panel()
    p.d = tmp_path_factory.mktemp(name)
    p.genomes = worlds.panel(p.d, seed, nstrains)
    p.models = [model.Model(g, ["A.txt", "B.txt", "C.txt"], 2, str(p.d)) for g in p.genomes]
    return p


@pytest.fixture(scope="module")
def panel3(tmp_path_factory):
    return _make_panel(tmp_path_factory, "prevmulti3", 303, 3)


@pytest.fixture(scope="module")
def panel5(tmp_path_factory):
    return _make_panel(tmp_path_factory, "prevmulti5", 505, 5)


def _S(p, tag, extra=(), env=None, genomes=None):
    """kmer_scrub_count -S over the panel's lists, outfiles <tag><i>.tsv, progress file prog_<tag>: (process, outfiles, progress lines
    without their time column)"""
    genomes = genomes or p.genomes
    outs = [f"{tag}{i}.tsv" for i in range(len(genomes))]
    (p.d / f"S_{tag}.txt").write_text("".join(f"{g}\t{o}\n" for g, o in zip(genomes, outs)))
    e = dict(os.environ, SK_CHUNK_BYTES="4096", SK_THREADS="3")
    e.update(env or {})
    r = subprocess.run([EXE, "-S", f"S_{tag}.txt", "-p", f"prog_{tag}"] + LISTS + list(extra), cwd=str(p.d), env=e, capture_output=True, timeout=240)
    prog = p.d / f"prog_{tag}"
    return r, outs, [ln.split(b"\t")[0] for ln in prog.read_bytes().split(b"\n")] if prog.exists() else None


def _said(stderr):
    return [ln for ln in stderr.split(b"\n") if b"timing" not in ln and not ln.startswith(b"key set of ")]


def _check_against_models(p, outs, models=None):
    for o, m in zip(outs, models or p.models):
        assert (p.d / (o + ".prev.tsv")).read_bytes() == m.prevalence_file(), o
        assert (p.d / (o + ".items.tsv")).read_bytes() == m.items_file(), o
        assert (p.d / o).read_bytes() == m.count_table(), o
        model.check_identities((p.d / (o + ".prev.tsv")).read_bytes(), (p.d / (o + ".items.tsv")).read_bytes(), (p.d / o).read_bytes())


def test_three_strains_equal_the_model_the_single_runs_and_the_run_without_the_flags(panel3):
    p = panel3
    assert p.models[0].n_items == [5, 3, 2] and p.models[1].n_items == [5, 3, 3] and p.models[2].n_items == [5, 3, 4]      # the -C rule is per strain
    on, outs, prog_on = _S(p, "on", FLAGS)
    assert on.returncode == 0, on.stderr.decode()[-2000:]
    _check_against_models(p, outs)
    for i, g in enumerate(p.genomes):                       # the single-strain program with the same flags
        one = subprocess.run([EXE, "-r", g] + LISTS + [f"--prevalence=one{i}.prev", f"--prevalence-items=one{i}.items", "--prevalence-min-count", "2"],
                             cwd=str(p.d), env=dict(os.environ, SK_CHUNK_BYTES="4096", SK_THREADS="3"), capture_output=True, timeout=240)
        assert one.returncode == 0, one.stderr.decode()[-2000:]
        assert (p.d / f"one{i}.prev").read_bytes() == (p.d / (outs[i] + ".prev.tsv")).read_bytes(), g
        assert (p.d / f"one{i}.items").read_bytes() == (p.d / (outs[i] + ".items.tsv")).read_bytes(), g
        assert one.stdout == (p.d / outs[i]).read_bytes(), g
    off, outs_off, prog_off = _S(p, "off")
    assert off.returncode == 0 and not (p.d / (outs_off[0] + ".prev.tsv")).exists()
    assert [(p.d / o).read_bytes() for o in outs] == [(p.d / o).read_bytes() for o in outs_off]
    assert (on.stdout, on.stderr) == (off.stdout, off.stderr) and prog_on == prog_off
    assert on.stderr == b"".join(b"skipping %s (identical match)\n" % g for g in (b"s0.fa", b"s1.fa", b"s0.fa"))


PLANS = {
    "group2": ({"SK_SCRUB_GROUP": "2"}, rb"3 union pass\(es\) \+ 0 single pass\(es\).*lists decoded 1 time"),
    "unions1": ({"SK_SCRUB_GROUP": "2", "SK_SCRUB_UNIONS": "1"}, rb"3 union pass\(es\) \+ 0 single pass\(es\).*lists decoded 3 time"),
    "hbm_defers": ({"SK_SCRUB_GROUP": "2", "SK_SCRUB_HBM_MB": "1"}, rb"3 union pass\(es\) \+ 0 single pass\(es\).*lists decoded 3 time"),
    "threads1": ({"SK_THREADS": "1"}, rb"1 union pass\(es\) \+ 0 single"),
    "threads3": ({"SK_THREADS": "3"}, rb"1 union pass\(es\) \+ 0 single"),       # (five items in -A: more items than slots)
    "no_union": ({"SK_SCRUB_NO_UNION": "1"}, rb"0 union pass\(es\) \+ 5 single pass\(es\)"),
    "list_pack2": ({"SK_LIST_PACK": "2"}, rb"1 union pass\(es\)"),
    "device_parse": ({"SK_DEVICE_PARSE": "1"}, rb"1 union pass\(es\)"),
}


@pytest.mark.parametrize("plan", sorted(PLANS))
def test_the_same_bytes_under_every_plan(panel5, plan):
    p = panel5
    env, said = PLANS[plan]
    on, outs, prog_on = _S(p, "on_" + plan, FLAGS, dict(env, SK_TIMING="1"))
    assert on.returncode == 0, on.stderr.decode()[-2000:]
    assert re.search(said, on.stderr), on.stderr.decode()[-2000:]
    assert re.search(rb"timing: prevalence: \d+ union\(s\) with \d+ item slot\(s\)", on.stderr) or plan == "no_union"
    _check_against_models(p, outs)
    off, outs_off, prog_off = _S(p, "off_" + plan, (), env)
    assert off.returncode == 0
    assert [(p.d / o).read_bytes() for o in outs] == [(p.d / o).read_bytes() for o in outs_off]
    assert _said(on.stderr) == _said(off.stderr) and prog_on == prog_off


def test_pack_cache_filling_and_served(panel5, tmp_path):
    p = panel5
    cache = str(tmp_path / "cache")
    os.mkdir(cache)
    for tag, want in (("fill", rb"(\d+) items served, (\d+) written"), ("serve", rb"(\d+) items served, (\d+) written")):
        on, outs, _ = _S(p, "pc_" + tag, FLAGS + ["--pack-cache", cache], {"SK_TIMING": "1"})
        assert on.returncode == 0, on.stderr.decode()[-2000:]
        _check_against_models(p, outs)
        served = sum(int(m.group(1)) for m in re.finditer(want, on.stderr))
        written = sum(int(m.group(2)) for m in re.finditer(want, on.stderr))
        # (12 items in the three lists; -C names s1.fa, which -A's walk has cached by then, and s0.fa twice)
        assert served + written == 12 and (written >= 10 if tag == "fill" else written == 0), on.stderr.decode()[-2000:]


def test_a_strain_with_an_iupac_letter_takes_its_own_pass_among_union_members(panel5):
    p = panel5
    g = bytearray(b"".join(ln for ln in (p.d / "s3.fa").read_bytes().split(b"\n") if not ln.startswith(b">")))
    g[700] = ord("R")                                       # inside a window: byte-string keys, which a union cannot hold
    (p.d / "iupac.fa").write_bytes(b">i\n" + bytes(g) + b"\n")
    genomes = p.genomes[:2] + ["iupac.fa"] + p.genomes[2:]
    models = p.models[:2] + [model.Model("iupac.fa", ["A.txt", "B.txt", "C.txt"], 2, str(p.d))] + p.models[2:]
    on, outs, _ = _S(p, "iupac", FLAGS, {"SK_TIMING": "1"}, genomes)
    assert on.returncode == 0, on.stderr.decode()[-2000:]
    assert re.search(rb"1 union pass\(es\) \+ 1 single pass\(es\)", on.stderr)
    _check_against_models(p, outs, models)


@pytest.mark.parametrize("independent", [False, True], ids=["joint", "independent"])
def test_scrub_by_prevalence_then_detect(panel3, independent, tmp_path):
    p = panel3
    tag = "sbp" + ("i" if independent else "j")
    lines = [(g, f"{tag}{i}.inf", f"{tag}{i}.kmer_hits.gz") for i, g in enumerate(p.genomes)]
    (p.d / f"S_{tag}.txt").write_text("".join("\t".join(l) + "\n" for l in lines))
    argv = ["-S", f"S_{tag}.txt"] + LISTS + ["--prevalence=.prev.tsv", "--scrub", "0.05", "--scrub-by", "prevalence"] + \
           (["--independent"] if independent else []) + ["--detect", "-B", "T.txt"]
    e = dict(os.environ, SK_CHUNK_BYTES="4096", SK_THREADS="3")
    on = subprocess.run([EXE] + argv, cwd=str(p.d), env=e, capture_output=True, timeout=240)
    assert on.returncode == 0, on.stderr.decode()[-2000:]
    nonempty = 0
    for (g, inf, hits), m in zip(lines, p.models):
        assert (p.d / (inf + ".prev.tsv")).read_bytes() == model.Model(g, ["A.txt", "B.txt", "C.txt"], 1, str(p.d)).prevalence_file(), g
        step2 = subprocess.run([os.path.join(BIN, "kmer_scrub_filter"), "-s", inf + ".prev.tsv", "-m", "0.05"] + (["-i"] if independent else []),
                               cwd=str(p.d), capture_output=True, timeout=120)
        assert step2.returncode == 0 and (p.d / inf).read_bytes() == step2.stdout, g
        nonempty += step2.stdout.count(b"\n") > 1
    assert nonempty, "some strain keeps informative k-mers"
    (p.d / f"S2_{tag}.txt").write_text("".join(f"{g}\t{inf}\tplain_{hits}\n" for g, inf, hits in lines))
    sd = subprocess.run([sk.cli_path("strain_detect"), "-S", f"S2_{tag}.txt", "-B", "T.txt"], cwd=str(p.d), env=e, capture_output=True, timeout=240)
    assert sd.returncode == 0, sd.stderr.decode()[-2000:]
    for g, inf, hits in lines:
        assert gzip.open(p.d / hits).read() == gzip.open(p.d / ("plain_" + hits)).read(), g
