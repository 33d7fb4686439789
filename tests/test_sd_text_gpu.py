"""strain_detect's plain-text targets parsed on the device (opt-in: SK_DEVICE_PARSE=1 / option "device_parse").

1. sk_batch_fill_text against sk_batch_fill: a batch the device parsed out of text and a batch filled from the oracle's decode of the
   same text give the same tallies for every record and the same hit log, on one table and on a 2-member union; the record lengths
   derived from the returned starts are the oracle's.  The batch from text holds EVERY record (short and empty ones tally 0).
2. bin/strain_detect with the switch on: the golden cases at the default chunk size and with tiny pieces; files that decline (each
   with the output of the switch off); -S, SK_DEVICES=0,0, the fused kmer_scrub_count job; random plain worlds on against off and
   against tests/_tally_ref.py.
The texts of the must-accept set and the fuzz generator are those of tests/test_text_parse_host.py, whose model says -- without a GPU --
which of them the device forms accept."""
import gzip
import json
import os
import random
import re
import subprocess

import numpy as np
import pytest

import _sd_text_model as model
import _synth
import _tally_ref as tr
import strainer2_amd as sk
import test_text_parse_host as tph
from strainer2_amd.native import TallyBatch

pytestmark = pytest.mark.gpu
K = 31
EDGE = 32768                                  # bytes of the record stream per scan tile (tile_first's unit)
PIECES = re.compile(rb"text pieces parsed on the device: (\d+) taken, (\d+) declined")


# =====================================================================================================================
# 1. a batch from text against a batch from the host
# =====================================================================================================================
def _runs_of(text):
    """the runs of 31 or more A/C/G/T (either case) in the records of `text`: what a strain can be made of without byte-string keys"""
    m = tph.model_parse(text)
    return re.findall(rb"[ACGTacgt]{31,}", m["stream"]) if m else []


@pytest.fixture(scope="module")
def world():
    """two strains (a 2-member union) that share keys: random text, and samples of the records of every must-accept text and of the
    fuzz worlds, so that every text below has windows that hit, informative ones among them"""
    rng = random.Random(77)
    g = _synth.rand_dna(rng, 150_000)
    sample = []
    for name, text in sorted(tph.must_accept_texts().items()):
        recs = _runs_of(text)
        sample += [r[:300] for r in recs[::max(1, len(recs) // 12)]][:12]
    for seed in range(FUZZ_SEEDS):
        sample += [r[:200] for r in _runs_of(tph.plain_world(seed))][:2]
    strains = [g[:100_000] + b"\n" + b"\n".join(sample[::2]), g[60_000:] + b"\n" + b"\n".join(sample[1::2] + sample[::6])]
    ctxs, sets = [], []
    for s in strains:
        ks = sk.Keyset.from_stream(s + b"\n", default_val=1, incr=0)
        c = sk.KmerContext(0)
        c.load_keyset(ks, 6)
        t = np.ones(ks.nrows, dtype=np.uint32)
        t[rng.sample(range(ks.nrows), ks.nrows // 3)] = 2
        c.set_counts(0, t)
        ctxs.append(c)
        sets.append(ks)
    u = sk.KmerUnion(ctxs, 0, 2)
    bt, bh = TallyBatch(ctxs[0]), TallyBatch(ctxs[0])
    yield dict(g=g, ctxs=ctxs, u=u, bt=bt, bh=bh, rng=rng)
    bt.close()
    bh.close()
    u.close()
    for c in ctxs:
        c.close()
    for k in sets:
        k.close()


FUZZ_SEEDS = 60


def _sorted_hits(h):
    h = np.asarray(h, dtype=np.int64).reshape(-1, h.shape[1] if len(h) else 2)
    return h[np.lexsort(tuple(h[:, i] for i in range(h.shape[1] - 1, -1, -1)))] if len(h) else h


def _compare(w, tmp_path, text, is_eof=True, lookahead=b"", what=""):
    """fill one batch from `text` on the device and one from the oracle's decode of it; every record's tallies and the sorted hit
    logs must be equal, on each context and on the union.  Returns (starts, lengths, informative hits on context 0)."""
    data, nrec = tph.oracle_decode(tmp_path, text)
    recs = data.split(b"\n")[:-1]
    assert len(recs) == nrec and nrec > 0, what
    want_starts = tr.starts_of(recs)
    want_len = np.array([len(r) for r in recs], dtype=np.int64)
    info, starts = w["bt"].fill_text(text, is_eof, lookahead)
    assert info.status == 0, (what, "declined")
    assert info.consumed == len(text), (what, info.consumed, len(text))
    assert (info.nrecords, info.stream_bytes, info.bases) == (nrec, len(data), int(want_len.sum())), what
    assert np.array_equal(starts, want_starts), what
    got_len = np.diff(np.append(starts.astype(np.int64), info.stream_bytes)) - 1
    assert np.array_equal(got_len, want_len), what
    w["bh"].fill(data, want_starts)
    inf0 = None
    for s, c in enumerate(w["ctxs"]):
        c.tally_launch(w["bt"], 0, 2)
        t1, h1, n1 = c.tally_collect()
        c.tally_launch(w["bh"], 0, 2)
        t2, h2, n2 = c.tally_collect()
        assert n1 == len(h1) and n2 == len(h2)
        assert np.array_equal(t1, t2), (what, s, np.nonzero((t1 != t2).any(axis=1))[0][:10])
        assert np.array_equal(_sorted_hits(h1), _sorted_hits(h2)), (what, s)
        assert not t1[want_len < K].any(), (what, "a record without a window has a tally")
        if s == 0:
            inf0 = int(t1[:, 1].sum())
    ut1, uh1 = w["u"].tally_filled(w["bt"])
    ut2, uh2 = w["u"].tally_filled(w["bh"])
    assert np.array_equal(ut1, ut2) and np.array_equal(uh1, uh2), (what, "union")
    return starts, want_len, inf0


def _fasta(recs, width=None, eol=b"\n"):
    out = []
    for i, r in enumerate(recs):
        out.append(b">r%d" % i + eol + (tph._wrap(r, width, eol) if width else (r + eol if r else b"")))
    return b"".join(out)


def _fastq(recs, eol=b"\n"):
    return b"".join(b"@q%d" % i + eol + r + eol + b"+" + eol + b"I" * len(r) + eol for i, r in enumerate(recs))


def _piece(rng, g, n):
    a = rng.randrange(len(g) - n)
    s = g[a:a + n]
    return _synth.revcomp(s) if rng.random() < 0.5 else s


@pytest.mark.parametrize("name", sorted(tph.must_accept_texts()))
def test_must_accept_texts(world, tmp_path, name):
    text = tph.must_accept_texts()[name]
    _, lens, inf = _compare(world, tmp_path, text, what=name)
    if _runs_of(text):
        assert inf > 0, (name, "no informative hit: the comparison would be of zeros")


def test_fuzz_worlds(world, tmp_path):
    forms, hits = set(), 0
    for seed in range(FUZZ_SEEDS):
        text = tph.plain_world(seed)
        _, _, inf = _compare(world, tmp_path, text, what=seed)
        hits += inf
        forms.add((text[:1] == b"@" and b"\n+" in text, b"\r" in text, text.endswith(b"\n")))
    assert len(forms) == 8 and hits > 100


@pytest.mark.parametrize("form", ["fasta", "fastq"])
def test_records_of_0_1_30_31_32_bases_interleaved(world, tmp_path, form):
    rng, g = random.Random(1), world["g"]
    sizes = (0, 1, 30, 31, 32) if form == "fasta" else (1, 30, 31, 32, 33)       # (a FASTQ sequence line is never empty)
    recs = [_piece(rng, g, sizes[i % 5]) if sizes[i % 5] else b"" for i in range(4000)]
    _, lens, inf = _compare(world, tmp_path, _fasta(recs) if form == "fasta" else _fastq(recs), what=form)
    assert inf > 0 and (lens < K).sum() == (2400 if form == "fasta" else 1600)


def test_fastq_with_empty_sequence_lines_declines(world, strain, tmp_path):
    """records of 0, 1, 30, 31, 32 bases as FASTQ: an empty sequence line is legal for the reference, and outside the FASTQ4 form (its
    sequence line is non-empty), so the piece DECLINES -- the batch cannot be launched on -- and the program's output with the switch
    on is that of the switch off"""
    rng, g = random.Random(8), world["g"]
    recs = [_piece(rng, g, (0, 1, 30, 31, 32)[i % 5]) if i % 5 else b"" for i in range(400)]
    text = _fastq(recs)
    assert tph.model_parse(text) is None
    info, starts = world["bt"].fill_text(text)
    assert info.status == 1 and len(starts) == 0
    with pytest.raises(sk.SKError):
        world["ctxs"][0].tally_launch(world["bt"], 0, 2)
    (tmp_path / "r.fq").write_bytes(_fastq([_piece(rng, strain["g"], (0, 1, 30, 31, 32, 150)[i % 6]) if i % 6 else b"" for i in range(600)]))
    (taken, declined), hits = _on_off(strain, tmp_path, [tmp_path / "r.fq"], "SE")
    assert (taken, declined) == (0, 1) and hits.count(b"\n") > 20


def _fill_to(rng, g, target):
    """records of about 150 bases whose stream is exactly `target` bytes long"""
    recs, off = [], 0
    while target - off > 400:
        recs.append(_piece(rng, g, rng.randint(100, 200)))
        off += len(recs[-1]) + 1
    recs.append(_piece(rng, g, target - off - 1))
    return recs


@pytest.mark.parametrize("where", ["first", "last", "edge", "edge-1", "edge+1"])
def test_an_empty_record_first_last_and_at_a_tile_edge(world, tmp_path, where):
    rng, g = random.Random(2), world["g"]
    if where == "first":
        recs = [b""] + _fill_to(rng, g, 40_000)
    elif where == "last":
        recs = _fill_to(rng, g, 40_000) + [b""]
    else:
        at = EDGE + {"edge": 0, "edge-1": -1, "edge+1": 1}[where]
        recs = _fill_to(rng, g, at) + [b"", _piece(rng, g, 150), b"", b""] + _fill_to(rng, g, 3000)
    starts, lens, inf = _compare(world, tmp_path, _fasta(recs), what=where)
    assert inf > 0
    e = [i for i in range(len(recs)) if not recs[i]][0]
    assert lens[e] == 0 and (e + 1 == len(recs) or starts[e + 1] == starts[e] + 1)
    if where.startswith("edge"):
        assert int(starts[e]) == EDGE + {"edge": 0, "edge-1": -1, "edge+1": 1}[where]


def test_a_100_kb_record_of_60_column_lines_between_short_ones(world, tmp_path):
    rng, g = random.Random(3), world["g"]
    recs = [_piece(rng, g, 150) for _ in range(20)] + [_synth.mutate(rng, g[5000:105_000], 0.002)] + [_piece(rng, g, 150) for _ in range(20)]
    starts, lens, inf = _compare(world, tmp_path, _fasta(recs, 60), what="long record")
    first = np.searchsorted(starts, np.arange(6) << 15)                      # (tile_first as the scan reads it)
    assert lens[20] == 100_000 and len(set(first[1:4].tolist())) == 1 and inf > 1000


def test_1500_records_of_31_to_35_bases_inside_one_tile(world, tmp_path):
    rng, g = random.Random(4), world["g"]
    recs = [_piece(rng, g, rng.choice([31] * 8 + [33, 35])) for _ in range(1500)] + [g[1000:21_000]] + [_piece(rng, g, 31) for _ in range(900)]
    starts, _, inf = _compare(world, tmp_path, _fastq(recs), what="dense tile")
    assert np.bincount(starts >> 15).max() > 900 and inf > 0


@pytest.mark.parametrize("d", [-1, 0, 1])
def test_a_record_starting_on_a_tile_edge_and_one_byte_either_side(world, tmp_path, d):
    rng, g = random.Random(5 + d), world["g"]
    head = _fill_to(rng, g, EDGE + d)
    recs = head + [g[100:500]] + [_piece(rng, g, 20) for _ in range(3)] + [_piece(rng, g, 200) for _ in range(10)]
    starts, _, inf = _compare(world, tmp_path, _fasta(recs, 70), what=d)
    assert int(starts[len(head)]) == EDGE + d and inf > 0


@pytest.mark.parametrize("size", [EDGE - 1, EDGE, EDGE + 1, 2 * EDGE - 1, 2 * EDGE, 2 * EDGE + 1])
def test_a_stream_of_exactly_one_and_two_tiles_and_a_byte_either_side(world, tmp_path, size):
    rng, g = random.Random(size), world["g"]
    recs = _fill_to(rng, g, size)
    starts, lens, inf = _compare(world, tmp_path, _fastq(recs) if size % 2 else _fasta(recs), what=size)
    assert int(starts[-1] + lens[-1] + 1) == size and inf > 0


@pytest.mark.parametrize("form", ["fasta", "fastq"])
def test_cr_lf_lines(world, tmp_path, form):
    rng, g = random.Random(6), world["g"]
    recs = [_piece(rng, g, rng.choice((1, 30, 31, 150, 700))) for _ in range(600)]
    _, _, inf = _compare(world, tmp_path, _fasta(recs, 60, b"\r\n") if form == "fasta" else _fastq(recs, b"\r\n"), what=form)
    assert inf > 0


@pytest.mark.parametrize("form", ["fasta", "fastq", "fasta_wrapped"])
def test_a_piece_before_the_last_goes_with_one_byte_of_look_ahead(world, tmp_path, form):
    """is_eof 0: the piece ends at a record start of its file and the next piece's first byte goes with it; the device then consumes
    exactly the piece -- and the rest of the file, sent as the last piece, gives the rest of the records"""
    rng, g = random.Random(7), world["g"]
    recs = [_piece(rng, g, rng.choice((5, 31, 150, 300))) for _ in range(700)]
    text = {"fasta": _fasta(recs), "fastq": _fastq(recs), "fasta_wrapped": _fasta(recs, 50)}[form]
    head = b"\n@q" if form == "fastq" else b"\n>r"
    cut = text.index(head, len(text) // 2) + 1
    a, _, inf_a = _compare(world, tmp_path, text[:cut], is_eof=False, lookahead=text[cut:cut + 1], what=form)
    b, _, inf_b = _compare(world, tmp_path, text[cut:], what=form)
    assert len(a) + len(b) == len(recs) and inf_a > 0 and inf_b > 0
    # without the look-ahead byte the piece's last record is not shown whole by the FASTA form: one record fewer, and not all consumed
    info, starts = world["bt"].fill_text(text[:cut] + b"X", is_eof=False, lookahead=b"")
    if form != "fastq":
        assert info.status == 0 and info.consumed < cut and len(starts) == len(a) - 1


def test_a_declined_piece_and_too_many_records_leave_the_batch_unusable(world):
    c, bt = world["ctxs"][0], world["bt"]
    info, starts = bt.fill_text(b">a\nACGT\n+\nIIII\n")                      # a '+' line in FASTA
    assert info.status == 1 and len(starts) == 0
    with pytest.raises(sk.SKError):
        c.tally_launch(bt, 0, 2)
    info, starts = bt.fill_text(b">\n" * ((1 << 22) + 1))                     # one record more than a batch takes
    assert info.status == 1 and len(starts) == 0
    with pytest.raises(sk.SKError):
        c.tally_launch(bt, 0, 2)
    info, starts = bt.fill_text(b">\n" * (1 << 22))                           # ... and exactly as many as it takes: all empty
    assert info.status == 0 and info.nrecords == 1 << 22 and info.stream_bytes == 1 << 22
    assert np.array_equal(starts, np.arange(1 << 22, dtype=np.uint32))
    c.tally_launch(bt, 0, 2)
    t, h, n = c.tally_collect()
    assert n == 0 and not t.any()


# =====================================================================================================================
# 2. the program
# =====================================================================================================================
def _exe(name="strain_detect"):
    return sk.cli_path(name)


def _sd(argv, cwd, **env):
    e = dict(os.environ)
    e.pop("SK_DEVICE_PARSE", None)
    e.update(env)
    return subprocess.run([_exe()] + argv, cwd=cwd, env=e, capture_output=True)


def _pieces(stderr):
    m = PIECES.search(stderr)
    return (int(m.group(1)), int(m.group(2))) if m else None


def _quiet(stderr):
    return b"".join(ln for ln in stderr.splitlines(True) if not ln.startswith(b"strain_detect timing:"))


@pytest.mark.parametrize("chunk", [None, "64", "333", "2000"])
@pytest.mark.parametrize("name", ["batch", "cli_pe", "cli_pei", "cli_default"])
def test_golden_cases_with_the_switch_on(golden, name, chunk, tmp_path):
    """plain .fa targets (in `batch` next to a .gz one, which stays on the host path) at the default chunk size -- one piece per file
    -- and in pieces of 2000, 333 and 64 bytes: many pieces, mates in different pieces.  At 64 a file is taken up to its first record
    that does not fit a piece with its look-ahead byte; il.fa, the one plain file of cli_pei and cli_default, begins with a record of
    65 bytes, so exactly (0 taken, 1 declined) there and pieces taken in every other case.  The counts are those of the reader's
    model (tests/_sd_text_model.py); stdout, stderr and hits are the reference's."""
    d = os.path.join(golden, "sd_cases", name)
    meta = json.load(open(os.path.join(d, "case.json")))
    argv = list(meta["argv"])
    argv[argv.index("-o") + 1] = str(tmp_path / "o.gz")
    env = {"SK_DEVICE_PARSE": "1"}
    if chunk:
        env["SK_SD_CHUNK_BYTES"] = chunk
    p = _sd(argv, d, **env)
    assert p.returncode == meta["returncode"] == 0, p.stderr.decode()[-2000:]
    assert p.stdout == open(os.path.join(d, "expected.stdout"), "rb").read()
    assert p.stderr == open(os.path.join(d, "expected.stderr"), "rb").read()
    assert gzip.open(tmp_path / "o.gz", "rb").read() == open(os.path.join(d, "expected.hits"), "rb").read()
    q = _sd(argv, d, SK_SD_TIMING="1", **env)
    assert q.returncode == 0 and gzip.open(tmp_path / "o.gz", "rb").read() == open(os.path.join(d, "expected.hits"), "rb").read()
    taken, declined = _pieces(q.stderr)
    want = model.pieces_of_case(d, chunk)                    # (the reader's cuts and the device forms' verdicts, known without a GPU)
    assert (taken, declined) == want, ((taken, declined), want)
    if chunk is None:
        assert declined == 0
    if not (chunk == "64" and name in ("cli_pei", "cli_default")):
        assert taken > 0, "no text piece was taken: this case would test the decline path only"


@pytest.fixture(scope="module")
def strain(tmp_path_factory):
    """one strain with its informative list, and reads of it"""
    d = tmp_path_factory.mktemp("sdtext")
    rng = random.Random(99)
    g = _synth.rand_dna(rng, 30_000)
    (d / "s.fa").write_bytes(b">s\n" + g + b"\n")
    kms = sorted({max(g[i:i + K], _synth.revcomp(g[i:i + K])) for i in range(0, len(g) - K, 5)})
    (d / "s.inf").write_bytes(b"#informative\n" + b"\n".join(kms) + b"\n")
    other = _synth.rand_dna(rng, 30_000)
    (d / "t.fa").write_bytes(b">t\n" + g[:10_000] + other[:20_000] + b"\n")
    kms = sorted({max(other[i:i + K], _synth.revcomp(other[i:i + K])) for i in range(0, 19_000, 7)})
    (d / "t.inf").write_bytes(b"#informative\n" + b"\n".join(kms) + b"\n")
    return dict(d=d, g=g, other=other)


def _reads(rng, g, n, lo=20, hi=200):
    return [_piece(rng, g, rng.randint(lo, hi)) if rng.random() < 0.8 else _synth.rand_dna(rng, rng.randint(lo, hi)) for _ in range(n)]


def _on_off(strain, tmp_path, files, mode, chunk=None, extra_env=None):
    """strain_detect over `files` with the switch off and on: stdout, stderr, exit code and hits equal; returns the pieces (taken,
    declined) of the run with the switch on, and the hits"""
    d = strain["d"]
    argv = ["-r", str(d / "s.fa"), "-a", str(d / "s.inf"), "-b", str(files[0])] + (["-c", str(files[1])] if len(files) > 1 else []) + ["-t", mode]
    env = dict(extra_env or {})
    if chunk:
        env["SK_SD_CHUNK_BYTES"] = str(chunk)
    runs = []
    for on in (False, True):
        out = tmp_path / ("on.gz" if on else "off.gz")
        p = _sd(argv + ["-o", str(out)], str(tmp_path), SK_SD_TIMING="1", **(dict(env, SK_DEVICE_PARSE="1") if on else env))
        runs.append((p.returncode, p.stdout, _quiet(p.stderr), gzip.open(out, "rb").read() if os.path.exists(out) else None, _pieces(p.stderr)))
    assert runs[0][:4] == runs[1][:4], (runs[0][:3], runs[1][:3])
    assert runs[0][4] is None
    return runs[1][4], runs[1][3]


@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_decline_a_plus_line_in_fasta(strain, tmp_path, where):
    rng = random.Random(10)
    recs = _reads(rng, strain["g"], 300)
    at = {"first": 1, "middle": 150, "last": 299}[where]
    lines = [b">r%d\n%s\n" % (i, r) + (b"+\nIIII\n" if i == at else b"") for i, r in enumerate(recs)]
    (tmp_path / "r.fa").write_bytes(b"".join(lines))
    (taken, declined), hits = _on_off(strain, tmp_path, [tmp_path / "r.fa"], "SE", chunk=4000)
    assert declined == 1 and (taken > 0) == (where != "first") and hits.count(b"\n") > 20


def test_decline_multi_line_fastq_at_once(strain, tmp_path):
    rng = random.Random(11)
    recs = _reads(rng, strain["g"], 200, 80, 200)
    (tmp_path / "r.fq").write_bytes(b"".join(b"@r%d\n%s\n%s\n+\n%s\n%s\n" % (i, r[:40], r[40:], b"I" * 40, b"I" * (len(r) - 40)) for i, r in enumerate(recs)))
    (taken, declined), hits = _on_off(strain, tmp_path, [tmp_path / "r.fq"], "SE", chunk=5000)
    assert (taken, declined) == (0, 1) and hits.count(b"\n") > 20


def test_decline_a_quality_one_byte_short(strain, tmp_path):
    rng = random.Random(12)
    recs = _reads(rng, strain["g"], 200, 40, 200)
    (tmp_path / "r.fq").write_bytes(b"".join(b"@r%d\n%s\n+\n%s\n" % (i, r, b"I" * (len(r) - (i == 120))) for i, r in enumerate(recs)))
    (taken, declined), hits = _on_off(strain, tmp_path, [tmp_path / "r.fq"], "SE", chunk=5000)
    assert declined == 1 and taken > 0 and hits.count(b"\n") > 20


def test_quality_lines_starting_with_at_where_a_cut_is_guessed(strain, tmp_path):
    """every quality line starts with '@', so wherever a cut is looked for the first candidate is a quality line.  The guess wants
    a '+' line two lines on and steps over it (two lines on is the next record's sequence); nothing is trusted from it either way:
    the device must consume exactly the piece.  A second file has quality lines starting with '>' behind the '+' line.  Pieces are
    taken, and the outputs are those of the switch off."""
    rng = random.Random(13)
    recs = _reads(rng, strain["g"], 400, 40, 120)
    for lead in (b"@", b">"):
        (tmp_path / "r.fq").write_bytes(b"".join(b"@r%d\n%s\n+\n%s\n" % (i, r, lead + b"I" * (len(r) - 1)) for i, r in enumerate(recs)))
        (taken, declined), hits = _on_off(strain, tmp_path, [tmp_path / "r.fq"], "SE", chunk=3000)
        assert taken > 5 and declined == 0 and hits.count(b"\n") > 20


def test_decline_a_file_without_a_final_newline_and_an_empty_file(strain, tmp_path):
    rng = random.Random(14)
    recs = _reads(rng, strain["g"], 100)
    for form, text in (("fa", _fasta(recs)), ("fq", _fastq(recs))):
        (tmp_path / f"r.{form}").write_bytes(text[:-1])
        (taken, declined), hits = _on_off(strain, tmp_path, [tmp_path / f"r.{form}"], "SE", chunk=4000)
        assert declined == 1 and taken > 0 and hits.count(b"\n") > 10
    (tmp_path / "e.fa").write_bytes(b"")
    _on_off(strain, tmp_path, [tmp_path / "e.fa"], "SE")


def test_decline_one_record_longer_than_a_piece(strain, tmp_path):
    rng = random.Random(15)
    recs = _reads(rng, strain["g"], 60) + [strain["g"][2000:12_000]] + _reads(rng, strain["g"], 60)
    (tmp_path / "r.fa").write_bytes(_fasta(recs, 60))
    (taken, declined), hits = _on_off(strain, tmp_path, [tmp_path / "r.fa"], "SE", chunk=4000)
    assert declined == 1 and taken > 0 and hits.count(b"\n") > 1000


def test_records_longer_than_the_cut_search_tail_are_cut_earlier(strain, tmp_path):
    """contigs of 100 kb in pieces of at most 300,000 bytes: no record starts in a buffer's last 64 KiB, and the cut is found earlier in
    the buffer -- every piece is taken"""
    g = strain["g"]
    recs = [(g + _synth.revcomp(g) + g + g)[i * 1000:i * 1000 + 100_000] for i in range(12)]
    text = _fasta(recs, 80)
    (tmp_path / "contigs.fa").write_bytes(text)
    want = model.pieces_of_file(text, 300_000)
    (taken, declined), hits = _on_off(strain, tmp_path, [tmp_path / "contigs.fa"], "SE", chunk=300_000)
    assert (taken, declined) == want and declined == 0 and taken >= 6 and hits.count(b"\n") > 1000


def test_decline_the_second_file_of_a_pair(strain, tmp_path):
    rng = random.Random(16)
    recs = _reads(rng, strain["g"], 300, 40, 150)
    (tmp_path / "p1.fa").write_bytes(_fasta(recs))
    (tmp_path / "p2.fa").write_bytes(b"".join(b">m%d\n%s\n" % (i, _synth.revcomp(r)) + (b"+\nII\n" if i == 200 else b"") for i, r in enumerate(recs)))
    (taken, declined), hits = _on_off(strain, tmp_path, [tmp_path / "p1.fa", tmp_path / "p2.fa"], "PE", chunk=5000)
    assert declined == 1 and taken > 5 and hits.count(b"\n") > 20


def test_decline_more_records_than_a_batch_takes(strain, tmp_path):
    """6 MiB of '>' lines in one piece of 16 MiB: 3 M empty records are taken; 10 MiB of them, 5 M, are more than 1 << 22 and decline"""
    rng = random.Random(17)
    tail = _fasta(_reads(rng, strain["g"], 50))
    (tmp_path / "few.fa").write_bytes(b">\n" * (3 << 20) + tail)
    (taken, declined), _ = _on_off(strain, tmp_path, [tmp_path / "few.fa"], "SE", chunk=16 << 20)
    assert (taken, declined) == (1, 0)
    (tmp_path / "many.fa").write_bytes(b">\n" * (5 << 20) + tail)
    (taken, declined), _ = _on_off(strain, tmp_path, [tmp_path / "many.fa"], "SE", chunk=16 << 20)
    assert (taken, declined) == (0, 1)


# ---- breadth ----------------------------------------------------------------------------------------------------------------
def _two_strains(strain, tmp_path, env):
    d = strain["d"]
    rng = random.Random(18)
    recs = _reads(rng, strain["g"], 400) + _reads(rng, strain["other"], 400)
    rng.shuffle(recs)
    (tmp_path / "r.fa").write_bytes(_fasta(recs))
    (tmp_path / "r.fq").write_bytes(_fastq([r for r in recs if r]))
    (tmp_path / "B.txt").write_text(f"SE\t{tmp_path}/r.fa\nPEI\t{tmp_path}/r.fq\n")
    res = []
    for on in (False, True):
        (tmp_path / "S.txt").write_text(f"{d}/s.fa\t{d}/s.inf\t{tmp_path}/a{on:d}.gz\n{d}/t.fa\t{d}/t.inf\t{tmp_path}/b{on:d}.gz\n")
        p = _sd(["-S", str(tmp_path / "S.txt"), "-B", str(tmp_path / "B.txt")], str(tmp_path), SK_SD_TIMING="1", SK_SD_CHUNK_BYTES="20000",
                **(dict(env, SK_DEVICE_PARSE="1") if on else env))
        assert p.returncode == 0, p.stderr.decode()[-2000:]
        res.append((p.stdout, gzip.open(tmp_path / f"a{on:d}.gz").read(), gzip.open(tmp_path / f"b{on:d}.gz").read(), _pieces(p.stderr)))
    assert res[0][:3] == res[1][:3] and res[0][3] is None
    assert res[1][1].count(b"\n") > 50 and res[1][2].count(b"\n") > 50
    return res[1][3]


def test_two_strains_in_one_union(strain, tmp_path):
    taken, declined = _two_strains(strain, tmp_path, {})
    assert taken > 5 and declined == 0


def test_two_logical_devices(strain, tmp_path):
    taken, declined = _two_strains(strain, tmp_path, {"SK_DEVICES": "0,0", "SK_SD_GROUP": "1"})
    assert taken > 5 and declined == 0


def test_the_fused_scrub_and_detect_job(tmp_path):
    import test_scrub_multi_workflow_gpu as wf
    d = str(tmp_path)
    genomes, tail = wf._world(1, d, nstrains=5)
    wf._drug_list(d, genomes, 1)
    wf._targets(d, genomes, 1)                          # (plain FASTQ with junk and empty reads, a .gz, a pair of plain FASTA files)
    outs = []
    for on in (False, True):
        p, lines = wf._fused(d, genomes, tail, ["-B", "T.txt"], env={"SK_DEVICE_PARSE": "1" if on else "0", "SK_SD_TIMING": "1"}, prefix=f"f{on:d}_")
        assert p.returncode == 0, p.stderr.decode()[-2000:]
        # the detect step of the fused job reaches the text path: the pair of plain FASTA files is taken (two pieces), and the plain FASTQ
        # file, whose reads include empty ones, goes as far as the model says
        want = [model.pieces_of_file(wf._read(os.path.join(d, f)) if not f.endswith(".gz") else b"") for f in ("t0.fq", "pe_1.fa", "pe_2.fa")]
        assert _pieces(p.stderr) == ((sum(t for t, _ in want), sum(x for _, x in want)) if on else None), (_pieces(p.stderr), want)
        assert not on or sum(t for t, _ in want) >= 2
        outs.append([(wf._read(os.path.join(d, l[1])), wf._read(os.path.join(d, l[2]))) for l in lines])
    assert outs[0] == outs[1] and sum(len(h) for _, h in outs[1]) > 1000


# ---- fuzz: random plain worlds, on against off and against the references ---------------------------------------------------------
def test_fuzz_plain_worlds_on_against_off_and_the_reference(strain, tmp_path):
    """plain files of the generator of tests/test_text_parse_host.py behind reads of the strain, FASTA and FASTQ, SE and PEI: the
    switch on against off, against the CPU oracle's strain_detect, and against tests/_tally_ref.py (the k-mers of the hit lines are
    the keys of the reference's informative hits; the trailer's totals are those of the records).  The model of
    test_text_parse_host.py says which files the device forms accept; a file also needs its final newline to be taken whole.  At
    least half of the files must be TAKEN: a path that always declines would pass everything else here."""
    import _oracle
    g, d = strain["g"], strain["d"]
    o = tr.OracleStrain(g + b"\n", capacity=1 << 17)
    kms = {l for l in (d / "s.inf").read_bytes().split(b"\n")[1:] if l}
    informative = np.array([max(k, _synth.revcomp(k)) in kms for k in o.keys], dtype=bool)
    assert informative.sum() > 1000
    files = expect_taken = 0
    for seed in range(8):
        rng = random.Random(1000 + seed)
        tail = tph.plain_world(seed * 7 + 1)
        fq = tail[:1] == b"@" and b"\n+" in tail
        eol = b"\r\n" if b"\r\n" in tail else b"\n"
        extra = [_piece(rng, g, rng.randint(31, 250)) for _ in range(40)]
        mode = "PEI" if seed % 2 else "SE"
        if mode == "PEI" and tph.model_parse(tail)["nrecords"] % 2:
            extra.pop()                                                            # (interleaved: every read has its mate)
        text = (_fastq(extra, eol) if fq else _fasta(extra, None, eol)) + tail     # (the world's own ending is the file's)
        m = tph.model_parse(text)
        assert m is not None, seed
        whole = text.endswith(b"\n")
        (tmp_path / "w.txt").write_bytes(text)
        (taken, declined), hits = _on_off(strain, tmp_path, [tmp_path / "w.txt"], mode)
        files += 1
        expect_taken += whole
        assert (taken, declined) == ((1, 0) if whole else (0, 1)), (seed, taken, declined)
        ora = _oracle.run_sd_oracle_cli(["-r", str(d / "s.fa"), "-a", str(d / "s.inf"), "-b", str(tmp_path / "w.txt"), "-t", mode,
                                         "-o", str(tmp_path / "ora.gz")], str(tmp_path))
        assert ora.returncode == 0 and gzip.open(tmp_path / "ora.gz", "rb").read() == hits, seed
        recs = m["stream"].split(b"\n")[:-1]
        want, log = o.tally(m["stream"], tr.starts_of(recs), informative)
        lines = [l.split(b"\t") for l in hits.split(b"\n") if l]
        got_keys = {max(l[5], _synth.revcomp(l[5])) for l in lines if not l[0].startswith(b"#")}
        want_keys = {max(o.keys[row], _synth.revcomp(o.keys[row])) for (_r, row) in log}
        assert got_keys == want_keys and len(want_keys) > 10, seed
        totals = {l[1]: int(l[2]) for l in lines if l[0].startswith(b"#")}
        lens = np.array([len(r) for r in recs])
        if mode == "SE":
            assert totals[b"total_reads_evaluated"] == int((lens >= K).sum()) and totals[b"total_kmer_evaluated"] == int((lens[lens >= K] - (K - 1)).sum())
    assert expect_taken * 2 >= files, (expect_taken, files)
