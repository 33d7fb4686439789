"""The one plain-file reader and the one text cutter of both host scan paths (strainer2_amd/csrc/sk_input.h) on their own: the
comparison program (tests/native/input_check.c, which includes sk_parser.h and sk_input.h only) is built under AddressSanitizer +
UBSan and must find, for every span, way of reading and read block, the records and the parser's end state of ONE parser_feed of
the same bytes; and for every delivery size and both taking disciplines, segments that are the text, end where a record start is
guessed, and parse on their own into the text's records."""
import os
import random
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
ENV.pop("SK_READ_BLOCK", None)


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("inp") / "input_check")
    subprocess.run(["gcc"] + SAN + [os.path.join(REPO, "tests", "native", "input_check.c"), "-o", exe], check=True)
    return exe


def run(checker, what, path):
    p = subprocess.run([checker, what, str(path)], env=ENV, capture_output=True)
    assert b"runtime error" not in p.stderr and b"AddressSanitizer" not in p.stderr, p.stderr.decode()[-2000:]
    assert p.returncode == 0, (p.stdout.decode()[-3000:], p.stderr.decode()[-1000:])
    assert b"MISMATCH" not in p.stdout
    return p.stdout.decode()


def dna(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def fastq(rng, nbytes, eol="\n"):
    """reads of 30-150 bases; every third quality line begins with '@', every fifth with '+'"""
    out, i = [], 0
    while sum(map(len, out)) < nbytes:
        n = rng.randrange(30, 151)
        q = "".join(rng.choice("ABCDEFGHIJ@+>") for _ in range(n))
        if i % 3 == 0:
            q = "@" + q[1:]
        elif i % 5 == 0:
            q = "+" + q[1:]
        out.append(f"@read{i} x{eol}{dna(rng, n)}{eol}+{eol}{q}{eol}")
        i += 1
    return "".join(out).encode()


def fasta(rng, nbytes, long_record=0, eol="\n"):
    """records of 100-900 bases wrapped at 60 columns; long_record: one of that many bases on a single line, a few records in"""
    out, i = [], 0
    while sum(map(len, out)) < nbytes:
        if long_record and i == 3:
            out.append(f">long one{eol}{dna(rng, long_record)}{eol}")
        s = dna(rng, rng.randrange(100, 901))
        out.append(f">contig{i} y{eol}" + "".join(s[j:j + 60] + eol for j in range(0, len(s), 60)))
        i += 1
    return "".join(out).encode()


@pytest.mark.parametrize("size", [12305, 70001])
def test_a_span_fed_three_ways_is_one_parser_feed_of_its_bytes(checker, tmp_path, size):
    """files of a few pages and an odd remainder (spans start and end inside pages), cut off at exactly `size` bytes"""
    rng = random.Random(size)
    texts = {"reads.fq": fastq(rng, size + 200), "wrapped.fa": fasta(rng, size + 200), "crlf.fq": fastq(rng, size + 200, eol="\r\n")}
    for name, text in texts.items():
        f = tmp_path / name
        f.write_bytes(text[:size])
        assert f.stat().st_size == size
        out = run(checker, "span", f)
        # every span of the list went each of the three ways, and the populated way was really taken where the kernel has it
        assert "35 spans x 3 ways x 3 blocks" in out, out
        assert int(out.split("blocks, ")[1].split()[0]) in (0, 35 * 3), out


def test_the_cutter_hands_out_the_text_in_segments_that_parse_alone(checker, tmp_path):
    rng = random.Random(300)
    texts = {"reads.fq": fastq(rng, 20000), "wrapped.fa": fasta(rng, 20000), "long.fa": fasta(rng, 15000, long_record=5000)}
    for name, text in texts.items():
        f = tmp_path / name
        f.write_bytes(text)
        out = run(checker, "cut", f)
        gathered_on = int(out.split("kept gathering ")[1].split()[0])
        if name == "long.fa":
            assert gathered_on > 0, out          # no record start behind `want` bytes yet: the cutter went on gathering
