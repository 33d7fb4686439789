"""strain_detect's targets parsed on the device (SK_DEVICE_PARSE=1), the HOST side of it: the reader that queues pieces of text, the
main thread's accept / decline, the hand-over of a declined file's rest to the parser threads -- sk_host.c + sk_host_sd.c +
sk_host_cov.c with the CPU doubles tests/native/device_double.c and sd_text_double.c, as a stand-alone program under
-fsanitize=address,undefined and again under -fsanitize=thread.  No GPU."""
import gzip
import json
import os
import re
import subprocess

import pytest

import _sd_text_model as model

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(REPO, "tests", "native")
SD_DIR = os.path.join(REPO, "tests", "golden", "sd_cases")
HOST = [os.path.join(REPO, "strainer2_amd", "csrc", f) for f in ("sk_host.c", "sk_host_sd.c", "sk_host_cov.c")]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1", TSAN_OPTIONS="halt_on_error=1",
           SK_THREADS="4")
PLAIN = ["batch", "cli_pe", "cli_pei", "cli_default"]           # the cases whose targets are plain .fa files (batch: next to a .gz one)
NONE_FITS_64 = ("cli_pei", "cli_default")                      # (see test_text_pieces_give_the_golden_output)
PIECES = re.compile(rb"text pieces parsed on the device: (\d+) taken, (\d+) declined")


def _build(tmp, san, with_double):
    exe = str(tmp / ("sd_text_" + san.split(",")[0] + ("" if with_double else "_nodouble")))
    srcs = [os.path.join(NATIVE, "device_double.c")] + ([os.path.join(NATIVE, "sd_text_double.c")] if with_double else []) + HOST
    subprocess.run(["gcc", "-O1", "-g", "-fsanitize=" + san, "-fno-omit-frame-pointer"] + srcs + ["-lz", "-lpthread", "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module", params=["address,undefined", "thread"])
def exe(request, tmp_path_factory):
    return _build(tmp_path_factory.mktemp("sdtext"), request.param, True)


@pytest.fixture(scope="module")
def exe_nodouble(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("sdtext0"), "address,undefined", False)


def _run(prog, name, tmp_path, **env):
    """the golden case under `env` with SK_SD_TIMING=1: outputs checked against the golden files; returns (taken, declined) or None"""
    d = os.path.join(SD_DIR, name)
    meta = json.load(open(os.path.join(d, "case.json")))
    argv = list(meta["argv"])
    out = tmp_path / "o.kmer_hits.gz"
    argv[argv.index("-o") + 1] = str(out)
    p = subprocess.run([prog] + argv, cwd=d, env=dict(ENV, SK_SD_TIMING="1", **env), capture_output=True)
    for bad in (b"runtime error", b"AddressSanitizer", b"ThreadSanitizer"):
        assert bad not in p.stderr, p.stderr.decode()[-3000:]
    assert p.returncode == meta["returncode"] == 0, p.stderr.decode()[-2000:]
    assert p.stdout == open(os.path.join(d, "expected.stdout"), "rb").read()
    said = b"".join(ln for ln in p.stderr.splitlines(True) if not ln.startswith(b"strain_detect timing:"))
    assert said == open(os.path.join(d, "expected.stderr"), "rb").read()
    assert gzip.open(out, "rb").read() == open(os.path.join(d, "expected.hits"), "rb").read()
    m = PIECES.search(p.stderr)
    return (int(m.group(1)), int(m.group(2))) if m else None


@pytest.mark.parametrize("chunk", [None, "64", "333", "2000"])
@pytest.mark.parametrize("name", PLAIN)
def test_text_pieces_give_the_golden_output(exe, name, chunk, tmp_path):
    """the switch on: at the default chunk size every plain file is one piece; 2000 and 333 bytes give many pieces, with mates in
    different pieces; at 64 bytes a file is taken up to its first record that does not fit a piece with its look-ahead byte, and the
    host parses the rest.  il.fa, the one plain file of cli_pei and cli_default, begins with a record of 65 bytes, which no piece of
    at most 64 holds: exactly (0 taken, 1 declined) there, pieces taken everywhere else.  The counts are the model's, the outputs the
    reference's."""
    env = {"SK_DEVICE_PARSE": "1"}
    if chunk:
        env["SK_SD_CHUNK_BYTES"] = chunk
    taken, declined = _run(exe, name, tmp_path, **env)
    # the pieces the reader cuts and the first one of each file that is not taken, from the model of the reader (no device needed)
    want = model.pieces_of_case(os.path.join(SD_DIR, name), chunk)
    assert (taken, declined) == want, ((taken, declined), want)
    if chunk is None:
        assert declined == 0
    if not (chunk == "64" and name in NONE_FITS_64):
        assert taken > 0, "no text piece was taken: this case would test the decline path only"


@pytest.mark.parametrize("at", ["0", "1", "3", "last"])
@pytest.mark.parametrize("name", PLAIN)
def test_a_declined_piece_hands_the_rest_of_its_file_to_the_host(exe, name, at, tmp_path):
    """the double declines the run's first piece, a middle one, or every file's last: the file's rest goes to the parser threads from
    that piece's start, text read ahead is dropped, and the outputs are the golden ones"""
    taken, declined = _run(exe, name, tmp_path, SK_DEVICE_PARSE="1", SK_SD_CHUNK_BYTES="333", SD_TEXT_DOUBLE_DECLINE_AT=at)
    assert declined >= 1, (taken, declined)
    if at != "0":
        assert taken >= 1, (taken, declined)


@pytest.mark.parametrize("name", PLAIN)
def test_declines_with_one_parser_thread_and_with_the_packed_upload(exe, name, tmp_path):
    """SK_NO_SPLIT and SK_SD_PACK behave as without the switch: the serial host parser takes a declined file's rest; a packed upload
    does not apply to text"""
    _run(exe, name, tmp_path, SK_DEVICE_PARSE="1", SK_SD_CHUNK_BYTES="333", SD_TEXT_DOUBLE_DECLINE_AT="2", SK_NO_SPLIT="1")
    _run(exe, name, tmp_path, SK_DEVICE_PARSE="1", SK_SD_CHUNK_BYTES="2000", SD_TEXT_DOUBLE_DECLINE_AT="last", SK_SD_PACK="1")


@pytest.mark.parametrize("name", PLAIN)
def test_switch_off_takes_no_text_piece(exe, name, tmp_path):
    assert _run(exe, name, tmp_path, SK_SD_CHUNK_BYTES="333") is None


@pytest.mark.parametrize("name", PLAIN)
def test_without_the_entry_points_the_switch_is_the_host_path(exe_nodouble, name, tmp_path):
    """sk_host_sd.c links without sk_batch_fill_text / sk_batch_text_finish / sk_text_enabled (weak references), and SK_DEVICE_PARSE=1
    then changes nothing"""
    assert _run(exe_nodouble, name, tmp_path, SK_DEVICE_PARSE="1", SK_SD_CHUNK_BYTES="333") is None
