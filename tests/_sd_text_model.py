"""What strain_detect's text reader (sk_host_sd.c: sd_text_read, sd_text_cut, sd_text_resolve) makes of a plain file, in Python: where
the pieces are cut (parser_guess_start of sk_parser.h, restated), which piece is the first the device does not take, and so how many
text pieces a run takes and declines -- known before a GPU sees the file.  The device's verdict on a piece is the model of
tests/test_text_parse_host.py (model_parse).  TEST INFRASTRUCTURE, imported by the tests only."""
import json
import os

import test_text_parse_host as tph

PIECE_MAX = 256 << 20
RECS_MAX = 1 << 22
DEFAULT_CHUNK = 32 << 20


def guess_start(t, size, x, size_is_eof):
    """parser_guess_start: the first offset >= x of t[:size] at which a record may start"""
    if x == 0:
        return 0
    i = x
    while i < size:
        nl = t.find(b"\n", i - 1, size)
        if nl < 0:
            return size
        s = nl + 1
        if s >= size:
            return size
        if t[s] == 0x3E:                                   # '>': not behind a '+' line (a quality line that begins with '>')
            q = s - 2 if s >= 2 else 0
            while q > 0 and t[q] != 10:
                q -= 1
            first = 0 if (q == 0 and t[0] != 10) else q + 1
            if not (s >= 2 and t[first] == 0x2B):
                return s
        if t[s] == 0x40:                                   # '@': with a '+' line two lines on
            l1 = t.find(b"\n", s, size)
            l2 = t.find(b"\n", l1 + 1, size) if l1 >= 0 and l1 + 1 < size else -1
            if l2 < 0 or l2 + 1 >= size:
                return s if size_is_eof else size
            if t[l2 + 1] == 0x2B:
                return s
        i = s + 1
    return size


def text_cut(t, n, cap, tail):
    """sd_text_cut on a text of n > cap bytes (t: its first cap + tail at least): the end of its first piece, 0 = no cut within one buffer"""
    lim = min(n, cap + tail)
    x = cap - tail
    while True:
        g = guess_start(t, lim, x, lim == n)
        if g + 1 <= cap:
            return g
        if x <= 1:
            return 0
        x //= 2


def pieces_of_file(text, chunk=None):
    """(taken, declined) of one plain file read with SK_SD_CHUNK_BYTES=chunk: pieces are taken until the first that is not"""
    if not text or text[:2] == b"\x1f\x8b":
        return 0, 0                                        # (an empty file is not mapped, a gzip file is inflated: the host path)
    cap = min(chunk or DEFAULT_CHUNK, PIECE_MAX)
    tail = min(cap // 2, 64 << 10)
    at, taken, n = 0, 0, len(text)
    while at < n:
        cut = n if n - at <= cap else at + text_cut(text[at:at + cap + tail], n - at, cap, tail)
        if cut == at or (cut == n and text[-1:] != b"\n"):
            return taken, 1
        last = cut == n
        m = tph.model_parse(text[at:cut + (0 if last else 1)], is_eof=last)
        if m is None or m["consumed"] != cut - at or m["nrecords"] > RECS_MAX:
            return taken, 1
        taken += 1
        at = cut
    return taken, 0


def pieces_of_case(case_dir, chunk=None):
    """(taken, declined) summed over the target files of a golden sd_cases directory (-b/-c, or the lines of the -B list)"""
    argv = json.load(open(os.path.join(case_dir, "case.json")))["argv"]
    files = []
    for flag in ("-b", "-c"):
        if flag in argv:
            files.append(argv[argv.index(flag) + 1])
    if "-B" in argv:
        for line in open(os.path.join(case_dir, argv[argv.index("-B") + 1])):
            f = line.rstrip("\n").split("\t")
            if f[0] in ("SE", "PE", "PEI"):
                files += f[1:3 if f[0] == "PE" else 2]
    taken = declined = 0
    for name in files:
        p = os.path.join(case_dir, name)
        if os.path.exists(p):
            t, d = pieces_of_file(open(p, "rb").read(), int(chunk) if chunk else None)
            taken, declined = taken + t, declined + d
    return taken, declined
