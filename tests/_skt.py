"""strain_detect's target cache files (strainer2_amd/csrc/sk_pcache.h, version 2, .skt) read and damaged from Python, for the tests:
the segment table of a file, skpc_sum64, and the two kinds of damage the tests make -- a flipped payload byte, and a changed length
with the segment's sum made good again.  Also the golden-case runner the CPU and GPU tests share."""
import gzip
import json
import os
import re
import struct
import subprocess

M64 = (1 << 64) - 1
HEADER, SEG_HEADER = 128, 64
STATS = re.compile(rb"target cache: (.*): (\d+) files served, (\d+) written, (\d+) stale, (\d+) not cached; checksums [0-9.]+ s, "
                   rb"reading [0-9.]+ s, writing [0-9.]+ s, waiting for the device pack [0-9.]+ s\n")


def _rotl(x, r):
    return ((x << r) | (x >> (64 - r))) & M64


def sum64(data):
    """skpc_sum64"""
    m = 0xFF51AFD7ED558CCD
    a = [0x9E3779B97F4A7C15, 0xC2B2AE3D27D4EB4F, 0x165667B19E3779F9, 0x27D4EB2F165667C5]
    n, at = len(data), 0
    while n - at >= 32:
        for k, w in enumerate(struct.unpack_from("<4Q", data, at)):
            a[k] = (_rotl(a[k] ^ w, 31) * m) & M64
        at += 32
    while n - at >= 8:
        a[0] = (_rotl(a[0] ^ struct.unpack_from("<Q", data, at)[0], 31) * m) & M64
        at += 8
    if n - at:
        w = int.from_bytes(bytes(data[at:]) + bytes(8 - (n - at)), "little")
        a[1] = (_rotl(a[1] ^ w, 31) * m) & M64
    h = a[0] ^ _rotl(a[1], 17) ^ _rotl(a[2], 34) ^ _rotl(a[3], 51) ^ ((n * m) & M64)
    h ^= h >> 33
    h = (h * 0xC4CEB9FE1A85EC53) & M64
    h ^= h >> 29
    return h


def pad8(n):
    return (n + 7) & ~7


def segments(path):
    """(header dict, [segment dicts with their offsets]) of a .skt file; asserts what the format promises"""
    b = open(path, "rb").read()
    assert b[:8] == b"SKPCACHE" and struct.unpack_from("<Q", b, 120)[0] == sum64(b[:120])
    version, k = struct.unpack_from("<II", b, 8)
    cap, size, mtime, records, bases, nseg, payload = struct.unpack_from("<QQqQQQQ", b, 16)
    head = dict(version=version, k=k, chunk_cap=cap, src_size=size, src_mtime=mtime, records=records, bases=bases, segments=nseg, payload_bytes=payload)
    assert version == 2 and k == 31 and len(b) == HEADER + SEG_HEADER * nseg + payload
    segs, at = [], HEADER
    for i in range(nseg):
        kind, flags, slen, plen, s, nrec, np_, end_kind, zero, end_len, zero2 = struct.unpack_from("<IIQQQIIIIQQ", b, at)
        part = pad8((slen + 15) // 16 * 6 if kind == 1 else slen)
        assert kind in (1, 2) and zero == 0 and zero2 == 0 and plen == part + 4 * nrec and (flags == 1) == (i == nseg - 1)
        assert s == sum64(b[at + SEG_HEADER: at + SEG_HEADER + plen])
        lens = struct.unpack_from("<%dI" % nrec, b, at + SEG_HEADER + part)
        assert sum(l + 1 for l in lens if l >= 31) == slen and sum(l >= 31 for l in lens) == np_ and slen <= cap
        segs.append(dict(at=at, kind=kind, last=flags, stream_len=slen, payload_len=plen, nrec=nrec, np=np_, table=at + SEG_HEADER + part, lens=lens))
        at += SEG_HEADER + pad8(plen)
    assert at == len(b) and sum(s["nrec"] for s in segs) == records
    return head, segs


def flip_payload_byte(path, seg, offset=0):
    """one payload byte of segment `seg` flipped; size and mtime of the cache file do not matter to its reader"""
    _, segs = segments(path)
    b = bytearray(open(path, "rb").read())
    b[segs[seg]["at"] + SEG_HEADER + offset] ^= 0x20
    open(path, "wb").write(b)


def change_length(path, seg, rec, new_len):
    """record `rec` of segment `seg` given another length, and the segment's checksum recomputed: only the structure check can tell"""
    _, segs = segments(path)
    s = segs[seg]
    b = bytearray(open(path, "rb").read())
    struct.pack_into("<I", b, s["table"] + 4 * rec, new_len)
    struct.pack_into("<Q", b, s["at"] + 24, sum64(bytes(b[s["at"] + SEG_HEADER: s["at"] + SEG_HEADER + s["payload_len"]])))
    open(path, "wb").write(b)


def stats(stderr):
    """(served, written, stale, not cached) of the run's one `target cache:` line, or None when there is none"""
    m = STATS.findall(stderr)
    assert len(m) <= 1, stderr.decode()[-2000:]
    return tuple(int(x) for x in m[0][1:]) if m else None


def quiet(stderr):
    """stderr less the timing lines"""
    return b"".join(ln for ln in stderr.splitlines(True) if not ln.startswith((b"strain_detect timing:", b"target cache:")))


def no_temporaries(cache_dir):
    left = [f for f in os.listdir(cache_dir) if ".tmp." in f or not f.endswith(".skt")]
    assert not left, left


def run_case(prog, case_dir, tmp_path, cache=None, env=None, mode=None, by_env=False, check=True):
    """one golden sd_cases directory through `prog` (a list: the program and what goes before strain_detect's own arguments) with
    SK_SD_TIMING=1; cache: the target cache's directory, given by --target-cache or (by_env) by SK_TARGET_CACHE.  The outputs are
    compared with the golden files (check) and returned with the cache's counters: (returncode, stdout, quiet stderr, hits, stats)"""
    meta = json.load(open(os.path.join(case_dir, "case.json")))
    argv = list(meta["argv"])
    out = None
    if "-o" in argv:
        out = str(tmp_path / "o.kmer_hits.gz")
        if os.path.exists(out):
            os.remove(out)
        argv[argv.index("-o") + 1] = out
    e = dict(os.environ, SK_SD_TIMING="1")
    for k in ("SK_TARGET_CACHE", "SK_TARGET_CACHE_MODE"):
        e.pop(k, None)
    e.update(env or {})
    if cache and by_env:
        e["SK_TARGET_CACHE"] = str(cache)
    elif cache:
        argv += ["--target-cache", str(cache)]
    if mode:
        e["SK_TARGET_CACHE_MODE"] = mode
    p = subprocess.run(list(prog) + argv, cwd=case_dir, env=e, capture_output=True)
    for bad in (b"runtime error", b"AddressSanitizer", b"ThreadSanitizer"):
        assert bad not in p.stderr, p.stderr.decode()[-3000:]
    hits = None
    if out and os.path.exists(out):
        try:
            hits = gzip.open(out, "rb").read()
        except EOFError:
            hits = b""
    if check:
        assert p.returncode == meta["returncode"], p.stderr.decode()[-2000:]
        assert p.stdout == open(os.path.join(case_dir, "expected.stdout"), "rb").read()
        assert quiet(p.stderr) == open(os.path.join(case_dir, "expected.stderr"), "rb").read()
        if meta["returncode"] == 0:
            assert hits == open(os.path.join(case_dir, "expected.hits"), "rb").read()
    return p.returncode, p.stdout, quiet(p.stderr), hits, stats(p.stderr)


def off_filling_served(prog, case_dir, tmp_path, env=None):
    """the three runs of one case, each against the goldens; returns the counters of the filling and of the served run"""
    cache = tmp_path / "tcache"
    cache.mkdir()
    off = run_case(prog, case_dir, tmp_path, env=env)
    assert off[4] is None                                  # (no switch, no line)
    fill = run_case(prog, case_dir, tmp_path, cache=cache, env=env)
    no_temporaries(cache)
    files = sorted(os.listdir(cache))
    for f in files:
        segments(os.path.join(cache, f))
    served = run_case(prog, case_dir, tmp_path, cache=cache, env=env, by_env=True)
    no_temporaries(cache)
    assert off[:4] == fill[:4] == served[:4]
    if fill[4] is not None:                                # (an error case that ends before the run begins says nothing)
        assert fill[4][1] == len(files) and fill[4][2] == 0 and served[4][1] == 0 and served[4][2] == 0
        assert served[4][0] == fill[4][0] + fill[4][1], (fill[4], served[4])     # every file that was written (or served within the filling run) is served
        assert served[4][3] == fill[4][3]
        assert sorted(os.listdir(cache)) == files
    return fill[4], served[4]
