"""Plain text parsed on the device, the half that needs no GPU.

1. A pure-Python model of the two device forms (FASTQ4, FASTA: include/strainer_kmer.h, sk_text_parse_device) is checked against
   the oracle's reader (_oracle.decode_file) on the must-accept set and on the plain fuzz worlds: the forms as written ARE the
   reference's grammar on those inputs, and the fuzz generator stays inside the forms -- known before a GPU sees either.
   tests/test_text_parse_gpu.py takes its texts from here.
2. The host layer's piece walk (sk_host.c: text_scan) against a CPU double of sk_scan_text_pinned built from sk_parser.h
   (tests/native/text_double.c), as a stand-alone program under -fsanitize=address,undefined: carry between pieces, growth of a
   piece that shows no whole record, a decline at the first, a middle and the last piece, a FASTQ record with a short quality, all
   giving the column and the base count of the run with the option off; and without the double's symbol SK_DEVICE_PARSE=1 is the
   host path."""
import os
import random
import subprocess

import pytest

import _oracle

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = 16384                       # SK_TEXT_TILE (include/strainer_kmer.h); test_tile_constant_matches_the_header pins it
HEAD = (b">", b"@")


# ---- the model: what the device forms make of a piece (None = declined) --------------------------------------------------
def _kept1(line):                                  # the CR rule for a line that is a record's whole sequence or quality
    return len(line) - (1 if len(line) > 1 and line.endswith(b"\r") else 0)


def model_parse(text, is_eof=True):
    """-> None (declined) or dict(form, consumed, stream, nrecords, bases, rec_start)"""
    n = len(text)
    if n == 0 or text[:1] not in HEAD:
        return None
    parts = text.split(b"\n")
    nl = len(parts) - 1                            # terminated lines
    lines = parts[:-1] + ([parts[-1]] if parts[-1] else [])
    T = len(lines)
    start = [0]
    for ln in lines:
        start.append(start[-1] + len(ln) + 1)
    recs = []
    if text[:1] == b"@" and nl >= 2 and T > 2 and lines[2][:1] == b"+":
        form, lim = "FASTQ4", (T if is_eof else nl & ~3)
        if is_eof and T % 4:
            return None
        for g in range(0, lim, 4):
            h, s, p, q = lines[g:g + 4]
            if h[:1] != b"@" or not s or s[:1] in HEAD + (b"+",) or p[:1] != b"+" or _kept1(q) != _kept1(s):
                return None
            recs.append(s[:_kept1(s)])
    else:
        form, heads, seqs = "FASTA", [], {}
        for i, ln in enumerate(lines):
            terminated = i < nl
            if not ln:
                continue
            if ln[:1] in HEAD:
                if not terminated and is_eof:
                    return None
                heads.append(i)
                seqs[i] = []
            elif not terminated and not is_eof:
                continue
            elif ln[:1] == b"+":
                return None
            else:
                k = len(ln)
                if ln.endswith(b"\r"):
                    if k > 1:
                        k -= 1
                    elif not terminated:
                        return None
                    else:
                        p = lines[i - 1]
                        if p and p[:1] not in HEAD + (b"+",) and p != b"\r":
                            k = 0
                        else:
                            return None
                seqs[heads[-1]].append(ln[:k])
        lim = T if is_eof else heads[-1]
        recs = [b"".join(seqs[h]) for h in heads if h < lim]
    consumed = n if lim == T else start[lim]
    stream = b"".join(r + b"\n" for r in recs)
    rs, at = [], 0
    for r in recs:
        rs.append(at)
        at += len(r) + 1
    return dict(form=form, consumed=consumed, stream=stream, nrecords=len(recs), bases=sum(map(len, recs)), rec_start=rs)


def oracle_decode(tmp_path, text, name="t.txt"):
    p = os.path.join(str(tmp_path), name)
    with open(p, "wb") as f:
        f.write(text)
    data, nrec, _st = _oracle.decode_file(p)
    return data, nrec


# ---- texts ---------------------------------------------------------------------------------------------------------------
def _dna(rng, n, alphabet=b"ACGT"):
    return bytes(rng.choice(alphabet) for _ in range(n))


def _wrap(seq, w, eol=b"\n"):
    return b"".join(seq[i:i + w] + eol for i in range(0, len(seq), w)) if seq else b""


def _fastq(rng, nrec, length=150, eol=b"\n", qfirst=b"@>+I"):
    out = []
    for r in range(nrec):
        s = _dna(rng, length if isinstance(length, int) else rng.randint(*length))
        q = bytes([qfirst[r % len(qfirst)]]) + bytes(rng.choice(b"FGHI#5:@>+") for _ in range(len(s) - 1))
        out.append(b"@r%d some comment" % r + eol + s + eol + b"+" + (b"r%d" % r if r % 3 == 0 else b"") + eol + q + eol)
    return b"".join(out)


def must_accept_texts():
    """name -> text; every one is inside the device forms (asserted by the model test below) and 100-400 KB, but the last two"""
    rng = random.Random(20260)
    t = {}
    t["fasta_reads"] = b"".join(b">read%d/1\n" % i + _dna(rng, 150) + b"\n" for i in range(1200))
    t["fasta_wrapped"] = b"".join(b">contig%d len\n" % i + _wrap(_dna(rng, 40000 if i == 3 else rng.randint(2000, 9000)), 60) for i in range(20))
    blank = []
    for i in range(600):
        s = _dna(rng, rng.randint(100, 400))
        blank.append(b">b%d\n" % i + (b"" if i % 7 == 3 else _wrap(s, 70).replace(b"\n", b"\n\n", 2) + (b"\n\n" if i % 5 == 0 else b"")))
    t["fasta_blank_lines_and_empty_records"] = b"".join(blank)
    t["fasta_records_of_0_1_30_31"] = b"".join(b">s%d\n" % i + (_dna(rng, (0, 1, 30, 31)[i % 4]) + b"\n" if i % 4 else b"") for i in range(9000))
    t["fastq_quality_starts_with_head_chars"] = _fastq(rng, 600)
    t["fasta_crlf"] = b"".join(b">c%d x\r\n" % i + _wrap(_dna(rng, rng.randint(1, 700)), 60, b"\r\n") + (b"\r\n" if i % 9 == 0 else b"") for i in range(500))
    t["fastq_crlf"] = _fastq(rng, 500, (1, 250), b"\r\n")
    t["fasta_no_final_newline"] = t["fasta_wrapped"][:150000].rstrip(b"\n")
    t["fastq_no_final_newline"] = _fastq(rng, 400)[:-1]
    allbytes = bytes(b for b in range(256) if b != 10)
    rows = []
    for i in range(700):
        body = _dna(rng, 40, b"ACGTacgtNnRYKMSWBDHVU") + allbytes[(i * 37) % 255:][:90] + _dna(rng, 30) + bytes([allbytes[i % 255]])
        rows.append(b">a%d\n" % i + b"A" + body + b"\n" + (b"c" + body[::-1] + b"G\n" if i % 2 else b""))
    t["fasta_every_byte_value"] = b"".join(rows)
    t["fastq_every_byte_value"] = b"".join(
        b"@q%d\n" % i + (s := b"T" + allbytes[(i * 41) % 255:][:100] + _dna(rng, 20, b"ACGTacgtNn")) + b"\n+\n" + b"I" * _kept1(s) + b"\n" for i in range(800))
    return t


def tile_boundary_text(form, pad):
    """a text of short lines that crosses offset SK_TEXT_TILE; its first header is padded to `pad` bytes, so sweeping `pad` over 81
    values moves every line end over 81 consecutive offsets (lines are at most 61 bytes apart: every offset TILE - 40 .. TILE + 40
    gets a line end in some case)"""
    rng = random.Random(5 + (form == "fastq"))            # (the same lines for every pad: the sweep shifts them byte by byte)
    if form == "fasta":
        out = b">" + b"h" * (pad - 2) + b"\n"
        i = 0
        while len(out) < TILE + 3000:
            i += 1
            out += (b">x%d\n" % i if i % 5 == 0 else b"") + _dna(rng, 1 + (i * 7) % 60) + b"\n"
        return out
    out = b""
    i = 0
    while len(out) < TILE + 3000:
        s = _dna(rng, 1 + (i * 5) % 61)
        out += b"@" + b"h" * (pad - 2 if i == 0 else i % 11) + b"\n" + s + b"\n+\n" + b"I" * len(s) + b"\n"
        i += 1
    return out


TILE_PADS = list(range(2, 2 + 81))


def plain_world(seed):
    """one small plain file inside the forms: form, line width, lengths, CRLF and the final newline vary"""
    rng = random.Random(seed)
    eol = b"\r\n" if rng.random() < 0.3 else b"\n"
    nrec = rng.randint(1, 60)
    if rng.random() < 0.5:
        text = _fastq(rng, nrec, (1, rng.choice((40, 300))), eol)
    else:
        w = rng.choice((1, 7, 60, 80, 10000))
        text = b"".join((b">" if rng.random() < 0.8 else b"@") + b"f%d d\t e" % i + eol +
                        _wrap(_dna(rng, rng.choice((0, 1, 29, 30, 31, 32, rng.randint(2, 900))), b"ACGTNacgt"), w, eol) +
                        (b"\n" if eol == b"\n" and rng.random() < 0.1 else b"") for i in range(nrec))
    if rng.random() < 0.4 and text.endswith(eol) and not text.endswith(b"\n" + eol) and not text.rsplit(b"\n", 2)[-2][:1] in HEAD:
        text = text[:-1]                           # the last line without its '\n' (never a header: that may be declined)
    return text


def mutate(text, seed):
    rng = random.Random(seed ^ 0x5EED)
    at = rng.randrange(len(text))
    kind = rng.random()
    b = bytes([rng.choice(b"\n\r+>@ACGT \t\0N") if rng.random() < 0.8 else rng.randrange(256)])
    if kind < 0.4:
        return text[:at] + b + text[at + 1:]
    if kind < 0.7:
        return text[:at] + b + text[at:]
    return text[:at] + text[at + 1:]


def cut_lengths(text):
    """ten cut lengths: inside a header, inside a sequence line, on a '\\n', behind one, between '+' and quality, and spread ones"""
    n = len(text)
    h = text.index(b"\n", n // 3)                          # a '\n' a third in
    head = max(text.rfind(b"\n>", 0, n // 2), text.rfind(b"\n@", 0, n // 2)) + 1
    cuts = {head + 2, h, h + 1, h + 2, n // 2 + 17, n // 7, (9 * n) // 10, n - 1, n - 2}
    p = text.find(b"\n+", n // 4)
    cuts.add(text.index(b"\n", p + 1) + 1 if p >= 0 else n // 5)   # FASTQ: the '+' line whole, no quality byte yet
    k = 3
    while len(cuts) < 10:
        cuts.add(n // k)
        k += 2
    return sorted(c for c in cuts if 0 < c < n)[:10]


# ---- 7: the model is the oracle's grammar on these inputs ------------------------------------------------------------------
def test_tile_constant_matches_the_header():
    with open(os.path.join(REPO, "include", "strainer_kmer.h")) as f:
        assert "#define SK_TEXT_TILE      %du" % TILE in f.read()


@pytest.mark.parametrize("name", sorted(must_accept_texts()))
def test_model_equals_oracle_on_the_must_accept_set(tmp_path, name):
    text = must_accept_texts()[name]
    assert name.endswith("value") or 100_000 <= len(text) <= 400_000
    m = model_parse(text)
    assert m is not None, "the model declines a must-accept text"
    data, nrec = oracle_decode(tmp_path, text)
    assert m["stream"] == data and m["nrecords"] == nrec and m["consumed"] == len(text)
    assert m["form"] == ("FASTQ4" if name.startswith("fastq") else "FASTA")


def test_model_equals_oracle_on_tile_boundary_texts(tmp_path):
    ends = {"fasta": set(), "fastq": set()}
    for form in ends:
        for pad in TILE_PADS:                              # every pad: the GPU test takes its expected values from the model on these texts
            text = tile_boundary_text(form, pad)
            m = model_parse(text)
            data, nrec = oracle_decode(tmp_path, text)
            assert m is not None and m["stream"] == data and m["nrecords"] == nrec
            # ... and the sweep puts a line end on every offset TILE - 40 .. TILE + 40
            ends[form] |= {i for i in range(TILE - 40, TILE + 41) if text[i] == 10}
        assert ends[form] == set(range(TILE - 40, TILE + 41)), sorted(set(range(TILE - 40, TILE + 41)) - ends[form])


def test_model_pieces_equal_oracle_of_the_consumed_prefix(tmp_path):
    for name, text in must_accept_texts().items():
        for cut in cut_lengths(text):
            m = model_parse(text[:cut], is_eof=False)
            assert m is not None, (name, cut)
            c = m["consumed"]
            assert c == 0 or (text[c:c + 1] in HEAD and text[c - 1:c] == b"\n")
            if c:
                data, nrec = oracle_decode(tmp_path, text[:c])
                assert (m["stream"], m["nrecords"]) == (data, nrec), (name, cut)
            else:
                assert m["nrecords"] == 0 and m["stream"] == b""


def test_plain_fuzz_worlds_are_inside_the_forms_and_exact(tmp_path):
    forms = set()
    for seed in range(200):
        text = plain_world(seed)
        m = model_parse(text)
        assert m is not None, seed
        data, nrec = oracle_decode(tmp_path, text)
        assert (m["stream"], m["nrecords"]) == (data, nrec), seed
        forms.add((m["form"], b"\r" in text, text.endswith(b"\n")))
    assert len(forms) == 8                                 # both forms, with and without CRLF, with and without the final newline


def test_model_accepted_mutants_are_exact(tmp_path):
    """any status is allowed for a mutated world; what the model accepts must be the oracle's"""
    accepted = 0
    for seed in range(200):
        text = mutate(plain_world(seed), seed)
        m = model_parse(text)
        if m is not None:
            accepted += 1
            data, nrec = oracle_decode(tmp_path, text)
            assert (m["stream"], m["nrecords"]) == (data, nrec), seed
    assert 20 < accepted < 200                             # (both outcomes occur)


# ---- 6: the host layer's piece walk against the CPU double ----------------------------------------------------------------
NATIVE = os.path.join(REPO, "tests", "native")
CSRC = os.path.join(REPO, "strainer2_amd", "csrc")


def _strain_files(d):
    """the three files of the end-to-end test (a wrapped FASTA genome, one-line FASTA reads, FASTQ reads) + the special ones"""
    import _synth
    rng = random.Random(77)
    strain = _synth.rand_dna(rng, 6000)
    other = _synth.rand_dna(rng, 4000)
    files = {}
    files["strain.fa"] = b">strain\n" + _wrap(strain, 60)
    files["genome.fa"] = b">g1 wrapped\n" + _wrap(strain[1000:4000] + other, 60) + b">g2\n" + _wrap(other[::-1] + strain[:500], 60)
    reads = [strain[i:i + 150] for i in range(0, 5800, 37)] + [other[i:i + 150] for i in range(0, 3800, 91)]
    files["reads.fa"] = b"".join(b">r%d\n" % i + r + b"\n" for i, r in enumerate(reads))
    files["reads.fq"] = b"".join(b"@q%d\n" % i + r + b"\n+\n" + b"@" * len(r) + b"\n" for i, r in enumerate(reads[::2]))
    bad = [b"@q%d\n" % i + r + b"\n+\n" + b"I" * (len(r) - (1 if i == 20 else 0)) + b"\n" for i, r in enumerate(reads[:40])]
    files["short_quality.fq"] = b"".join(bad)
    files["one_long_record.fa"] = b">long\n" + _wrap(strain + other + strain[::-1], 60) + b">tail\n" + strain[:100] + b"\n"
    for name, data in files.items():
        with open(os.path.join(d, name), "wb") as f:
            f.write(data)
    return files


@pytest.fixture(scope="module")
def text_host_program(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("text_host"))
    common = ["-std=gnu11", "-g", "-O1", "-fsanitize=address,undefined", "-static-libasan", "-fno-sanitize-recover=undefined", "-I", os.path.join(REPO, "include"), "-I", CSRC]
    common.append("-DDOUBLE_NO_MAIN")
    srcs = [os.path.join(NATIVE, "text_host_main.c"), os.path.join(NATIVE, "device_double.c")] + [os.path.join(CSRC, f) for f in ("sk_host.c", "sk_host_sd.c", "sk_host_cov.c")]
    libs = ["-lz", "-lpthread", "-ldl", "-lm"]
    with_double = os.path.join(d, "with_double")
    without = os.path.join(d, "without_double")
    subprocess.run(["gcc"] + common + ["-o", with_double] + srcs + [os.path.join(NATIVE, "text_double.c")] + libs, check=True)
    subprocess.run(["gcc"] + common + ["-o", without] + srcs + libs, check=True)
    _strain_files(d)
    return d, with_double, without


def _run(prog, d, files, env_extra):
    lst = os.path.join(d, "list.txt")
    with open(lst, "w") as f:
        f.write("".join(os.path.join(d, n) + "\n" for n in files))
    env = {k: v for k, v in os.environ.items() if not k.startswith("SK_")}
    env.update(ASAN_OPTIONS="detect_leaks=0", SK_THREADS="2")
    env.update(env_extra)
    r = subprocess.run([prog, os.path.join(d, "strain.fa"), lst], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert b"ERROR: AddressSanitizer" not in r.stderr and b"runtime error" not in r.stderr, r.stderr.decode()[-2000:]
    return r.stdout


PLAIN = ["genome.fa", "reads.fa", "reads.fq"]


@pytest.mark.parametrize("piece", [64, 257, 4096])
def test_piece_walk_gives_the_host_paths_column(text_host_program, piece):
    d, prog, _ = text_host_program
    files = PLAIN + ["short_quality.fq", "one_long_record.fa"]
    off = _run(prog, d, files, {})
    assert b"pieces=0 " in off and b"sum=0\n" not in off
    on = _run(prog, d, files, {"SK_DEVICE_PARSE": "1", "SK_TEXT_PIECE_BYTES": str(piece)})
    assert on.split(b"\n")[0] == off.split(b"\n")[0]                       # bases, column sum and digest
    assert b"pieces=0 " not in on
    if piece < 4096:
        assert b"grown=0" not in on                                        # one_long_record.fa: a piece had to grow


@pytest.mark.parametrize("at", ["0", "3", "last"])
def test_forced_decline_hands_the_rest_to_the_host(text_host_program, at):
    d, prog, _ = text_host_program
    off = _run(prog, d, PLAIN, {})
    on = _run(prog, d, PLAIN, {"SK_DEVICE_PARSE": "1", "SK_TEXT_PIECE_BYTES": "4096", "SK_THREADS": "1", "TEXT_DOUBLE_DECLINE_AT": at})
    assert on.split(b"\n")[0] == off.split(b"\n")[0]
    assert b"declined=0" not in on


def test_without_the_device_parser_the_switch_is_the_host_path(text_host_program):
    d, _, prog = text_host_program
    off = _run(prog, d, PLAIN, {})
    on = _run(prog, d, PLAIN, {"SK_DEVICE_PARSE": "1", "SK_TEXT_PIECE_BYTES": "64"})
    assert on == off
