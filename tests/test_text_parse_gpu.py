"""Plain FASTA/FASTQ text parsed on the device (sk_text_parse_device, sk_scan_text_pinned, option "device_parse"): the record stream,
record starts, `consumed` and the counts against the oracle's reader and the host path.  The texts, the piece cuts, the fuzz
generator and the model that validates them on the CPU come from tests/test_text_parse_host.py."""
import os
import random
import subprocess

import numpy as np
import pytest

import _oracle
import strainer2_amd as sk
from strainer2_amd import native
from test_text_parse_host import (HEAD, PLAIN, TILE, TILE_PADS, _strain_files, cut_lengths, model_parse, must_accept_texts, mutate,
                                  oracle_decode, plain_world, tile_boundary_text)

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, DECLINED = native.SK_TEXT_OK, native.SK_TEXT_DECLINED


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """the small strain and its three plain files (+ the special ones), a context with the strain resident"""
    d = str(tmp_path_factory.mktemp("text_gpu"))
    files = _strain_files(d)
    ks = sk.Keyset.from_file(os.path.join(d, "strain.fa"))
    ctx = sk.KmerContext(0)
    ctx.load_keyset(ks, 4)
    yield d, files, ks, ctx
    ctx.close()


def parse(ctx, text, is_eof=True):
    """-> (info, stream bytes, rec_start array); stream and starts only when the status is OK"""
    n = len(text)
    d_text = ctx.dev_alloc(n + 16)
    ctx.dev_upload(d_text, np.frombuffer(text, dtype=np.uint8))
    info, d_out, d_rs = ctx.parse_text_device(d_text, n, is_eof, want_rec_start=True)
    stream, rs = b"", np.zeros(0, dtype=np.uint32)
    if info.status == OK:
        assert info.stream_bytes <= n + 1 and info.nrecords <= n // 2 + 1
        if info.stream_bytes:
            stream = ctx.dev_download(d_out, info.stream_bytes).tobytes()
        if info.nrecords:
            rs = ctx.dev_download(d_rs, 4 * info.nrecords).view(np.uint32)
    for p in (d_text, d_out, d_rs):
        ctx.dev_free(p)
    return info, stream, rs


def starts_of(stream):
    at = np.flatnonzero(np.frombuffer(stream, dtype=np.uint8) == 10)
    return np.concatenate(([0], at[:-1] + 1)).astype(np.uint32) if len(at) else np.zeros(0, dtype=np.uint32)


def check_exact(ctx, tmp_path, text, is_eof=True):
    """accepted, and equal to the oracle for text[:consumed]"""
    info, stream, rs = parse(ctx, text, is_eof)
    assert info.status == OK
    if is_eof:
        assert info.consumed == len(text)
    data, nrec = oracle_decode(tmp_path, text[:info.consumed]) if info.consumed else (b"", 0)
    assert stream == data
    assert info.nrecords == nrec and info.bases == len(data) - nrec
    assert np.array_equal(rs, starts_of(data))
    return info


# ---- 1: the must-accept set ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(must_accept_texts()))
def test_must_accept(world, tmp_path, name):
    ctx = world[3]
    info = check_exact(ctx, tmp_path, must_accept_texts()[name])
    assert info.form == (native.SK_TEXT_FASTQ4 if name.startswith("fastq") else native.SK_TEXT_FASTA)
    assert info.nrecords > 300 or name in ("fasta_wrapped", "fasta_no_final_newline")


@pytest.mark.parametrize("form", ["fasta", "fastq"])
def test_line_ends_on_every_offset_around_a_tile_boundary(world, tmp_path, form):
    ctx = world[3]
    assert TILE == native.SK_TEXT_TILE
    for pad in TILE_PADS:                                  # each case one small parse; the sweep covers TILE - 40 .. TILE + 40 (host test)
        text = tile_boundary_text(form, pad)
        info, stream, rs = parse(ctx, text)
        m = model_parse(text)                              # (the model is the oracle on these texts: tests/test_text_parse_host.py)
        assert info.status == OK and stream == m["stream"] and info.nrecords == m["nrecords"], pad
        assert list(rs) == m["rec_start"], pad


# ---- 2: pieces -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(must_accept_texts()))
def test_pieces(world, tmp_path, name):
    ctx = world[3]
    text = must_accept_texts()[name]
    cuts = cut_lengths(text)
    assert len(cuts) == 10
    for cut in cuts:
        info = check_exact(ctx, tmp_path, text[:cut], is_eof=False)
        c = info.consumed
        assert c <= cut and (c == 0 or (text[c:c + 1] in HEAD and text[c - 1:c] == b"\n")), cut
    # feeding pieces onward with the carry reproduces the whole file's stream
    whole, _ = oracle_decode(tmp_path, text)
    piece, at, got = len(text) // 6 + 1, 0, []
    while at < len(text):
        size = piece
        while True:
            eof = at + size >= len(text)
            info, stream, _rs = parse(ctx, text[at:at + size], eof)
            assert info.status == OK
            if info.consumed or eof:
                break
            size *= 2
        got.append(stream)
        at += info.consumed
    assert b"".join(got) == whole


# ---- 3: must decline or be exact ---------------------------------------------------------------------------------------------------
def decline_cases():
    import _synth
    strain = _synth.rand_dna(random.Random(77), 6000)      # (the strain of _strain_files: these reads are counted)
    fq = lambda i, s, q=None: b"@r%d\n" % i + s + b"\n+\n" + (q if q is not None else b"I" * len(s)) + b"\n"
    seqs = [strain[(i * 53) % 5800:][:150] for i in range(700)]
    c = {}
    c["fastq_wrapped_sequence"] = b"".join(b"@r%d\n" % i + s[:80] + b"\n" + s[80:] + b"\n+\n" + b"I" * 150 + b"\n" for i, s in enumerate(seqs))
    c["fastq_blank_line"] = b"".join(fq(i, s) + (b"\n" if i == 350 else b"") for i, s in enumerate(seqs))
    c["fastq_quality_one_short"] = b"".join(fq(i, s, b"I" * (149 if i == 350 else 150)) for i, s in enumerate(seqs))
    c["fasta_plus_line"] = b"".join(b">r%d\n" % i + s + b"\n" + (b"+\n" if i == 350 else b"") for i, s in enumerate(seqs))
    c["junk_before_first_header"] = b"junk line\n" + b"".join(b">r%d\n" % i + s + b"\n" for i, s in enumerate(seqs))
    c["fastq_sequence_line_starts_with_gt"] = b"".join(fq(i, (b">" + s[1:]) if i == 350 else s) for i, s in enumerate(seqs))
    return c


@pytest.mark.parametrize("name", sorted(decline_cases()))
def test_declines_or_is_exact_and_the_counts_do_not_change(world, tmp_path, name):
    d, _files, _ks, ctx = world
    text = decline_cases()[name]
    assert 100_000 <= len(text) <= 400_000
    info, stream, rs = parse(ctx, text)
    if info.status == DECLINED:
        assert info.consumed == 0 and info.stream_bytes == 0 and info.nrecords == 0
    else:
        data, nrec = oracle_decode(tmp_path, text[:info.consumed])
        assert stream == data and info.nrecords == nrec
    path = os.path.join(str(tmp_path), name + ".txt")
    with open(path, "wb") as f:
        f.write(text)
    got = {}                                               # counts through scan_file, the switch off and on
    for on in (0, 1):
        ctx.set_option("device_parse", on)
        ctx.zero_counts(2)
        bases = ctx.scan_file(path, 2)
        got[on] = (bases, ctx.counts(2).copy())
    ctx.set_option("device_parse", 0)
    assert got[0][0] == got[1][0] and np.array_equal(got[0][1], got[1][1])
    assert int(got[0][1].sum()) > 1000


# ---- 4: end to end ---------------------------------------------------------------------------------------------------------------
def _list(d, names, name="list.txt"):
    p = os.path.join(d, name)
    with open(p, "w") as f:
        f.write("".join(os.path.join(d, n) + "\n" for n in names))
    return p


def _scan_list(ctx, d, lst, on, tag, others=None):
    ctx.set_option("device_parse", on)
    ctx.zero_counts(1)
    for o in others or []:
        o.zero_counts(1)
    if others:
        bases = ctx.scan_list_many(others, lst, 1)
        prog = err = b""
    else:
        pp, ep = os.path.join(d, tag + ".progress"), os.path.join(d, tag + ".err")
        bases = ctx.scan_list(lst, 1, progress_path=pp, err_path=ep)
        prog = b"\n".join(ln.split(b"\t")[0] for ln in open(pp, "rb").read().split(b"\n"))
        err = open(ep, "rb").read()
    ctx.set_option("device_parse", 0)
    return bases, ctx.counts(1).copy(), prog, err


@pytest.mark.parametrize("piece", ["64", "4096", None])
def test_scan_list_with_the_switch_equals_the_host_path_and_the_oracle(world, monkeypatch, piece):
    d, _files, ks, ctx = world
    lst = _list(d, PLAIN)
    monkeypatch.delenv("SK_TEXT_PIECE_BYTES", raising=False)
    off = _scan_list(ctx, d, lst, 0, "off")
    if piece:
        monkeypatch.setenv("SK_TEXT_PIECE_BYTES", piece)
    ctx.text_stats(reset=True)
    on = _scan_list(ctx, d, lst, 1, "on")
    pieces, declined = ctx.text_stats()
    assert pieces >= 3 and declined == 0                   # the device path was really taken, for every piece of the plain files
    if piece:
        assert pieces > 3
    assert on[0] == off[0] and np.array_equal(on[1], off[1]) and on[2] == off[2] and on[3] == off[3]
    t = _oracle.OracleTable()
    assert t.build_file(os.path.join(d, "strain.fa")) == 0
    for n in PLAIN:
        t.scan_file(os.path.join(d, n), 1)
    okeys, ocounts = t.rows()
    assert ks.keys() == okeys and np.array_equal(on[1], ocounts[:, 1]) and int(on[1].sum()) > 1000


def test_scan_list_many_with_two_contexts(world, monkeypatch):
    d, _files, ks, ctx = world
    lst = _list(d, PLAIN + ["short_quality.fq", "one_long_record.fa"], "many.txt")
    monkeypatch.setenv("SK_TEXT_PIECE_BYTES", "4096")
    with sk.KmerContext(0) as other:
        other.load_keyset(ks, 4)
        off = _scan_list(ctx, d, lst, 0, "m_off", [other])
        off_other = other.counts(1).copy()
        ctx.text_stats(reset=True)
        on = _scan_list(ctx, d, lst, 1, "m_on", [other])
        pieces, declined = ctx.text_stats()
        assert pieces > 5 and declined == 1                # (the short quality string declines its piece: the host finds where the reference stops)
        assert on[0] == off[0] and np.array_equal(on[1], off[1]) and np.array_equal(other.counts(1), off_other)
        assert np.array_equal(off[1], off_other) and int(off_other.sum()) > 1000


def test_the_program_prints_the_same_bytes_under_the_switch(world):
    d = world[0]
    a, b = _list(d, ["genome.fa"], "A.txt"), _list(d, ["reads.fa", "reads.fq"], "B.txt")
    outs = []
    for on in ("0", "1"):
        env = {k: v for k, v in os.environ.items() if not k.startswith("SK_")}
        env.update(SK_DEVICE_PARSE=on, SK_TEXT_PIECE_BYTES="4096")
        r = subprocess.run([native.cli_path(), "-r", os.path.join(d, "strain.fa"), "-A", a, "-B", b], env=env, stdout=subprocess.PIPE,
                           stderr=subprocess.PIPE, timeout=120)
        assert r.returncode == 0, r.stderr.decode()[-1000:]
        outs.append((r.stdout, r.stderr))
    assert outs[0] == outs[1] and outs[0][0].count(b"\n") > 1000


def test_scan_text_counts_what_scan_file_counts(world):
    d, files, _ks, ctx = world
    for name in PLAIN:
        ctx.set_option("device_parse", 0)
        ctx.zero_counts(3)
        bases = ctx.scan_file(os.path.join(d, name), 3)
        want = ctx.counts(3).copy()
        ctx.zero_counts(3)
        info = ctx.scan_text(files[name], 3)
        assert info.status == OK and info.bases == bases and info.consumed == len(files[name])
        assert np.array_equal(ctx.counts(3), want)


# ---- 5: fuzz -----------------------------------------------------------------------------------------------------------------------
def test_fuzz_plain_worlds_are_accepted_and_exact(world):
    ctx = world[3]
    for seed in range(200):
        text = plain_world(seed)
        m = model_parse(text)                              # (== the oracle on these worlds, asserted on the CPU: tests/test_text_parse_host.py)
        info, stream, rs = parse(ctx, text)
        assert info.status == OK and stream == m["stream"] and info.nrecords == m["nrecords"] and info.bases == m["bases"], seed
        assert list(rs) == m["rec_start"] and info.consumed == len(text), seed


def test_fuzz_mutated_worlds_are_exact_when_accepted_and_never_change_the_counts(world, tmp_path):
    d, files, _ks, ctx = world
    reads = files["reads.fa"][:3000]                       # (so that there is something to count)
    accepted = 0
    path = os.path.join(str(tmp_path), "m.txt")
    for seed in range(200):
        text = mutate(plain_world(seed), seed)
        info, stream, _rs = parse(ctx, text)
        if info.status == OK:
            accepted += 1
            data, nrec = oracle_decode(tmp_path, text)
            assert stream == data and info.nrecords == nrec and info.consumed == len(text), seed
        with open(path, "wb") as f:
            f.write(reads + text if text[:1] in HEAD else text + reads)
        got = []
        for on in (0, 1):
            ctx.set_option("device_parse", on)
            ctx.zero_counts(2)
            got.append((ctx.scan_file(path, 2), ctx.counts(2).copy()))
        ctx.set_option("device_parse", 0)
        assert got[0][0] == got[1][0] and np.array_equal(got[0][1], got[1][1]), seed
    assert accepted > 20
