"""sk_union_share and strain_detect -S --panel-share=FILE on the device, against the model (tests/_panel_model.py: plain set
operations over each member's keys and its informative keys; the reference has no counterpart).

Library level: random worlds of related strains in unions of 1, 2, 7 and 32; 32 members with a common key and member 31 (bit 31)
with keys of its own; two unions cut from _craft.union_wrap()'s four members, whose keys cluster at the end of the tables so that
the probes in the foreign table are long and wrap; a union of more slots than one pass of the kernel's grid covers; a foreign union
that shares nothing.  Programs: a panel of five strains in one, two and three unions and on two logical devices of one card, the
table byte for byte the model's and every other output untouched by the flag; the fused job kmer_scrub_count -S --scrub --detect."""
import gzip
import os
import random
import subprocess

import numpy as np
import pytest

import _craft
import _panel_model as model
import _synth
import strainer2_amd as sk
from test_gpu_union import _mutate, _strains

pytestmark = pytest.mark.gpu

# sk_union_share_sweep runs at most SK_SHARE_BLOCKS = 512 workgroups of 256 threads (sk_dev_union.hip.h): one pass of the grid covers
# 131072 slots
GRID_THREADS = 512 * 256


class _Members:
    """the strains of one union on the device: contexts, key sets, and per member its keys and informative keys as sets of text"""

    def __init__(self, streams, informative, load_pct=None, initial_slots=None):
        """informative(s, keys in row order) -> boolean array over the rows"""
        self.ctxs, self.sets, self.keys, self.inf = [], [], [], []
        for s, stream in enumerate(streams):
            ks = sk.Keyset.from_stream(stream, default_val=1, incr=0, **({"initial_slots": initial_slots} if initial_slots else {}))
            self.sets.append(ks)
            c = sk.KmerContext(0)
            self.ctxs.append(c)
            if load_pct and load_pct[s] != 50:
                c.set_option("table_load_pct", load_pct[s])
            c.load_keyset(ks, 6)
            rows = ks.keys()
            inf = np.asarray(informative(s, rows), dtype=bool)
            typ = np.ones(len(rows), dtype=np.uint32)
            typ[inf] = 2
            c.set_counts(0, typ)
            self.keys.append(set(rows))
            self.inf.append({k for k, f in zip(rows, inf) if f})
            assert len(self.keys[-1]) == len(rows)

    def close(self):
        for c in self.ctxs:
            c.close()
        for k in self.sets:
            k.close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


def _random_rows(rng):
    def pick(s, rows):
        f = np.zeros(len(rows), dtype=bool)
        if len(rows):
            f[np.array(sorted(rng.sample(range(len(rows)), max(1, len(rows) // rng.choice([3, 10, 50])))), dtype=np.int64)] = True
        return f
    return pick


def _invariants_self(m, a):
    """every result of a union against itself"""
    m0, m1, m2 = (x.astype(np.int64) for x in m)
    assert np.array_equal(m0, m0.T)
    assert np.array_equal(np.diag(m0), [len(k) for k in a.keys])
    assert np.array_equal(np.diag(m1), [len(k) for k in a.inf])
    _invariants(m)


def _invariants(m, self_m1=None):
    """every result: out[2] <= out[1] <= out[0] cell by cell, out[1][i][j] <= out[1][i][i] (of a's own side)"""
    m0, m1, m2 = (x.astype(np.int64) for x in m)
    assert (m2 <= m1).all() and (m1 <= m0).all()
    own = np.diag(m1 if self_m1 is None else self_m1.astype(np.int64))
    assert (m1 <= own[:, None]).all()


def _check_self(u, a):
    got = u.share()
    raw = u.share_raw.copy()
    want = model.share(a.keys, a.inf)
    n = len(a.keys)
    for k in range(3):
        assert got[k].dtype == np.uint64 and got[k].shape == (n, n)
        assert np.array_equal(got[k], want[k]), (k, got[k], want[k])
    beyond = raw.copy()
    beyond[:, :n, :n] = 0
    assert not beyond.any(), "a cell beyond the members is not 0"
    again = u.share()
    assert all(np.array_equal(x, y) for x, y in zip(got, again)) and np.array_equal(raw, u.share_raw)
    _invariants_self(got, a)
    return got


@pytest.mark.parametrize("n,seed", [(1, 100), (2, 3), (7, 5), (32, 101)])
def test_random_worlds_against_the_model(n, seed):
    """the same strain twice, a mutated copy, an unrelated strain, the other strand of a part, a repeated segment with an N
    (test_gpu_union._strains); random informative rows"""
    rng = random.Random(seed)
    strains = _strains(rng, seed, n)
    with _Members([g + b"\n" for g in strains], _random_rows(rng)) as a, sk.KmerUnion(a.ctxs, 0, 2) as u:
        got = _check_self(u, a)
        if n > 1:
            assert int(got[0].sum() - np.trace(got[0])) > 0, "no two members share a key: this world tests nothing"


def test_thirty_two_members_with_a_common_key_and_bit_31():
    """one 40-base piece in every member, informative in all of them: all 3 x 1024 cells are at least 1 (a key of all 32 members is
    1024 adds a matrix).  Member 31 alone holds a piece of its own, partly informative: bit 31 of both masks"""
    rng = random.Random(31)
    common, last = _synth.rand_dna(rng, 40), _synth.rand_dna(rng, 300)
    streams = [common + b"\n" + _synth.rand_dna(rng, 60 + 7 * s) + b"\n" + (last + b"\n" if s == 31 else b"") for s in range(32)]
    ckeys = {model.canonical(common[i:i + 31]) for i in range(10)}
    lkeys = {model.canonical(last[i:i + 31]) for i in range(0, 270, 2)}
    with _Members(streams, lambda s, rows: [k in ckeys or (s == 31 and k in lkeys) or (s % 3 == 0 and i % 5 == 0) for i, k in enumerate(rows)]) as a, \
            sk.KmerUnion(a.ctxs, 0, 2) as u:
        got = _check_self(u, a)
        assert u.share_raw.min() >= 10
        only31 = a.keys[31] - set().union(*a.keys[:31])
        assert len(only31) == 270 + 247 and only31 & a.inf[31] == lkeys       # (its piece of 300 bases and its random one of 277)
        assert len(lkeys) == 135
        assert int(got[0][31, 31]) - int(got[0][31, :31].max()) >= 270


def _wrap_unions():
    """_craft.union_wrap()'s members 0-1 and 2-3 as two unions, table_load_pct 90 on each first member; b's members also hold the
    world's absent keys (they start in the same cluster as the crafted keys)"""
    w = _craft.union_wrap()
    extra = b"".join(_craft.kmer_bytes(k) + b"\n" for k in w.absent)
    streams = [mw.sstream + (extra if s >= 2 else b"") for s, mw in enumerate(w.members)]
    crafted_inf = [{model.canonical(_craft.kmer_bytes(k)) for k in mw.informative_keys} for mw in w.members]

    def pick(base):
        return lambda s, rows: [k in crafted_inf[base + s] for k in rows]
    a = _Members(streams[:2], pick(0), load_pct=[90, 50], initial_slots=_craft.CAP)
    b = _Members(streams[2:], pick(2), load_pct=[90, 50], initial_slots=_craft.CAP)
    return w, a, b


def test_two_unions_with_long_wrapping_probes():
    """expected exactly: the key all four share, the 20 pair keys between neighbours (1 with 2, 3 with 0) and nothing else, in both
    directions.  Informative (informative_keys): the all-shared key in everyone, a member's pair keys with the NEXT member on its own
    side only -- so of 1's informative keys 2 holds 21, both call 1 informative; of 0's informative keys 3 holds the shared one only
    (pair[3] is informative in 3, not in 0)"""
    w, a, b = _wrap_unions()
    try:
        assert [len(k) for k in a.keys] == [230, 230] and [len(k) for k in b.keys] == [230 + len(w.absent)] * 2
        with sk.KmerUnion(a.ctxs, 0, 2) as ua, sk.KmerUnion(b.ctxs, 0, 2) as ub:
            assert ua.rows == 460 and ub.rows == 460 + 2 * len(w.absent)
            ab, ba = ua.share(ub), ub.share(ua)
            assert not ua.share_raw[:, 2:, :].any() and not ua.share_raw[:, :, 2:].any()
            want_ab, want_ba = model.share(a.keys, a.inf, b.keys, b.inf), model.share(b.keys, b.inf, a.keys, a.inf)
            for k in range(3):
                assert np.array_equal(ab[k], want_ab[k]) and np.array_equal(ba[k], want_ba[k]), k
            # rows: members 0, 1; columns: members 2, 3
            assert ab[0].tolist() == [[1, 21], [21, 1]]
            assert ab[1].tolist() == [[1, 1], [21, 1]]
            assert ab[2].tolist() == [[1, 1], [1, 1]]
            assert ba[0].tolist() == [[1, 21], [21, 1]]
            assert ba[1].tolist() == [[1, 1], [21, 1]]          # of 3's informative keys (the shared one, pair[3]) 0 holds 21
            assert ba[2].tolist() == [[1, 1], [1, 1]]
            # the two directions agree
            assert np.array_equal(ab[0], ba[0].T) and np.array_equal(ab[2], ba[2].T)
            aa, bb = ua.share(), ub.share()
            _invariants(ab, aa[1])
            _invariants(ba, bb[1])
            _invariants_self(aa, a)
            _invariants_self(bb, b)
            assert np.array_equal(ua.share(ua)[0], aa[0])        # (b == a by handle: the same as NULL)
    finally:
        a.close()
        b.close()


def test_a_union_of_more_slots_than_one_pass_of_the_grid():
    """four random strains of 40 000 bases: about 160 000 rows, at the default load of 50 % a table of 524 288 slots -- four turns of
    the grid-stride loop of 131 072 threads (GRID_THREADS)"""
    rng = random.Random(77)
    base = _synth.rand_dna(rng, 40000)
    strains = [base, _mutate(rng, base, 0.01), _synth.rand_dna(rng, 40000), _synth.revcomp(base[10000:]) + _synth.rand_dna(rng, 10000)]
    with _Members([g + b"\n" for g in strains], _random_rows(rng)) as a, sk.KmerUnion(a.ctxs, 0, 2) as u:
        slots = 1024
        while slots * 50 < u.rows * 100:
            slots *= 2
        assert slots > GRID_THREADS, (slots, u.rows)
        _check_self(u, a)


def test_a_foreign_union_that_shares_nothing():
    rng = random.Random(78)
    with _Members([_synth.rand_dna(rng, 2000) + b"\n" for _ in range(3)], _random_rows(rng)) as a, \
            _Members([_synth.rand_dna(rng, 1500) + b"\n" for _ in range(2)], _random_rows(rng)) as b, \
            sk.KmerUnion(a.ctxs, 0, 2) as ua, sk.KmerUnion(b.ctxs, 0, 2) as ub:
        assert not set().union(*a.keys) & set().union(*b.keys)
        got = ua.share(ub)
        assert all(g.shape == (3, 2) for g in got) and not ua.share_raw.any()
        assert not ub.share(ua)[0].any() and not ub.share_raw.any()


def test_two_random_unions_in_both_directions():
    """share(other) and other.share(self): matrices 0 and 2 are transposes of each other, matrix 1 is bounded by its own side's
    diagonal; both against the model"""
    rng = random.Random(79)
    strains = _strains(rng, 0, 9)
    with _Members([g + b"\n" for g in strains[:5]], _random_rows(rng)) as a, _Members([g + b"\n" for g in strains[5:]], _random_rows(rng)) as b, \
            sk.KmerUnion(a.ctxs, 0, 2) as ua, sk.KmerUnion(b.ctxs, 0, 2) as ub:
        ab, ba = ua.share(ub), ub.share(ua)
        want_ab, want_ba = model.share(a.keys, a.inf, b.keys, b.inf), model.share(b.keys, b.inf, a.keys, a.inf)
        for k in range(3):
            assert ab[k].shape == (5, 4) and ba[k].shape == (4, 5)
            assert np.array_equal(ab[k], want_ab[k]) and np.array_equal(ba[k], want_ba[k]), k
        assert int(ab[0].sum()) > 0 and int(ab[2].sum()) > 0
        assert np.array_equal(ab[0], ba[0].T) and np.array_equal(ab[2], ba[2].T)
        _invariants(ab, ua.share()[1])
        _invariants(ba, ub.share()[1])


# ---------------------------------------------------------------------------------------------------------------------------------
# the programs
# ---------------------------------------------------------------------------------------------------------------------------------
def _read(path):
    with (gzip.open if str(path).endswith(".gz") else open)(path, "rb") as f:
        return f.read()


@pytest.fixture(scope="module")
def panel(tmp_path_factory):
    """five small strains (a strain, the same again, a mutated copy, an unrelated one, the other strand of a part with a repeat and
    an N), each with an informative list of k-mers on either strand, and three small targets; the model's table, computed once"""
    d = tmp_path_factory.mktemp("panel")
    rng = random.Random(5)
    base = _synth.rand_dna(rng, 3000)
    part = _synth.revcomp(base[1000:]) + base[200:500]
    genomes = [base, base, _mutate(rng, base, 0.01), _synth.rand_dna(rng, 2000), part[:50] + b"N" + part[51:] + _synth.rand_dna(rng, 400)]
    strains = []
    for s, g in enumerate(genomes):
        (d / f"g{s}.fa").write_bytes(b">g%d\n" % s + g[:len(g) // 2] + b"\n" + g[len(g) // 2:] + b"\n")
        words = [g[i:i + 31] for i in range(0, len(g) - 30, 3 + s) if b"N" not in g[i:i + 31]]
        words = [w if rng.random() < 0.5 else _synth.revcomp(w) for w in words] + [genomes[3][7:38]]
        (d / f"inf{s}.txt").write_bytes(b"#informative\n" + b"".join(w + b"\n" for w in words))
        strains.append((f"g{s}.fa", f"inf{s}.txt", f"Genus_species_{s}.kmer_hits.gz"))
    (d / "S.txt").write_text("".join("\t".join(l) + "\n" for l in strains))
    lines = []
    for t in range(3):
        recs = _synth.fuzz_stream(rng, genomes[(2 * t) % 5], 150, p_junk=0.01, min_len=20, max_len=180).split(b"\n")[:-1]
        (d / f"t{t}.fa").write_bytes(b"".join(b">r%d\n" % i + r.replace(b"\r", b"A") + b"\n" for i, r in enumerate(recs)))
        lines.append(f"SE\tt{t}.fa")
    (d / "T.txt").write_text("\n".join(lines) + "\n")
    want = model.table_from_files([tuple(str(d / f) for f in l) for l in strains])
    assert want.count(b"\n") == 26
    return d, strains, want


def _sd(d, out, extra, env):
    """strain_detect -S in `out` (a directory of its own: the outfiles' names are the same in every run)"""
    out.mkdir()
    for f in os.listdir(d):
        os.symlink(d / f, out / f)
    return subprocess.run([sk.cli_path("strain_detect"), "-S", "S.txt", "-B", "T.txt", "--coverage-depth"] + extra, cwd=str(out),
                          env=dict(os.environ, **env), capture_output=True, timeout=240)


@pytest.mark.parametrize("env", [{"SK_SD_GROUP": "2"}, {}, {"SK_DEVICES": "0,0"}, {"SK_DEVICES": "0,0", "SK_SD_GROUP": "2"}],
                         ids=["group2", "default", "devices00", "devices00_group2"])
def test_the_programs_table_and_nothing_else_changes(panel, tmp_path, env):
    """SK_SD_GROUP=2: unions of 2 + 2 + 1 strains, cross-group pairs and a one-member union; SK_DEVICES=0,0: two logical devices on
    one card.  The table is the model's byte for byte, and the hit lists, the coverage tables, stdout and stderr are what the run
    without the flag writes"""
    d, strains, want = panel
    on = _sd(d, tmp_path / "on", ["--panel-share=panel.tsv"], env)
    assert on.returncode == 0, on.stderr.decode()[-2000:]
    got = (tmp_path / "on" / "panel.tsv").read_bytes()
    assert got == want, (got[:600], want[:600])
    off = _sd(d, tmp_path / "off", [], env)
    assert off.returncode == 0, off.stderr.decode()[-2000:]
    assert on.stdout == off.stdout and on.stderr == off.stderr
    assert sorted(os.listdir(tmp_path / "on")) == sorted(os.listdir(tmp_path / "off") + ["panel.tsv"])
    for _, _, o in strains:
        assert _read(tmp_path / "on" / o) == _read(tmp_path / "off" / o), o
        cov = o[:-len(".kmer_hits.gz")] + ".coverage_depth"
        assert (tmp_path / "on" / cov).read_bytes() == (tmp_path / "off" / cov).read_bytes(), cov
    assert len(_read(tmp_path / "on" / strains[0][2])) > 0


def test_the_timing_line_and_a_panel_the_unions_cannot_hold(panel, tmp_path):
    """SK_SD_TIMING=1 adds one line (3 unions: 9 calls); SK_SD_NO_UNION=1 leaves no union tables, and the run fails with one line
    before any target is read"""
    d, strains, want = panel
    p = _sd(d, tmp_path / "t", ["--panel-share=panel.tsv"], {"SK_SD_GROUP": "2", "SK_SD_TIMING": "1"})
    assert p.returncode == 0 and (tmp_path / "t" / "panel.tsv").read_bytes() == want
    assert [l for l in p.stderr.decode().splitlines() if "panel share" in l and l.endswith("9 call(s) of sk_union_share")], p.stderr.decode()[-1500:]
    p = _sd(d, tmp_path / "n", ["--panel-share=panel.tsv"], {"SK_SD_NO_UNION": "1"})
    assert p.returncode != 0 and not os.path.exists(tmp_path / "n" / "panel.tsv")
    assert b"--panel-share: the strains cannot all be held in union tables" in p.stderr
    assert b"total_kmer_evaluated" not in b"".join(_read(tmp_path / "n" / o) for _, _, o in strains)


def test_a_panel_of_one_strain(panel, tmp_path):
    """-S with one line builds no union table for the scans; the table's one line comes from a union made for it alone"""
    d, strains, _ = panel
    out = tmp_path / "one"
    out.mkdir()
    for f in os.listdir(d):
        if f != "S.txt":
            os.symlink(d / f, out / f)
    (out / "S.txt").write_text("\t".join(strains[4]) + "\n")
    p = subprocess.run([sk.cli_path("strain_detect"), "-S", "S.txt", "-B", "T.txt", "--panel-share=panel.tsv"], cwd=str(out), capture_output=True, timeout=240)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    want = model.table_from_files([tuple(str(d / f) for f in strains[4])])
    assert (out / "panel.tsv").read_bytes() == want and want.count(b"\n") == 2
    assert b"total_kmer_evaluated" in _read(out / strains[4][2])


def test_the_fused_job(tmp_path):
    """kmer_scrub_count -S --scrub .. --detect .. --panel-share=FILE: the table equals the model's, computed from the informative
    lists the job itself wrote"""
    from test_scrub_multi_workflow_gpu import _drug_list, _fused, _targets, _world
    d = str(tmp_path)
    genomes, tail = _world(8, d, nstrains=4)
    _drug_list(d, genomes, 8)
    _targets(d, genomes, 8)
    p, lines = _fused(d, genomes, tail, ["-B", "T.txt", "--panel-share=panel.tsv"], env={"SK_SD_GROUP": "3"})
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    want = model.table_from_files([tuple(os.path.join(d, f) for f in l) for l in lines])
    got = open(os.path.join(d, "panel.tsv"), "rb").read()
    assert got == want, (got[:600], want[:600])
    rows = [l.split(b"\t") for l in got.split(b"\n")[1:-1]]
    assert len(rows) == 16 and any(int(r[3]) > 0 for r in rows) and any(r[0] != r[1] and int(r[4]) > 0 for r in rows)
