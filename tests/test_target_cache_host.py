"""strain_detect's target cache, the HOST side of it, without a GPU: sk_host_sd.c (the writer thread, the serving thread, the switch),
sk_host.c and sk_host_cov.c over tests/native/target_cache_double.c -- device_double.c with sk_batch_pack_home left absent, so the
writer packs with sk_pack_stream -- built as a stand-alone program under -fsanitize=address,undefined and again under
-fsanitize=thread.  The golden cases run off, filling and served at SK_SD_CHUNK_BYTES=64 (mates in different segments, state carried
across them); a C driver in the same program checks the version-2 reader and writer of sk_pcache.h on their own."""
import gzip
import os
import shutil
import subprocess

import pytest

import _skt

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(REPO, "tests", "native")
SD_DIR = os.path.join(REPO, "tests", "golden", "sd_cases")
HOST = [os.path.join(REPO, "strainer2_amd", "csrc", f) for f in ("sk_host.c", "sk_host_sd.c", "sk_host_cov.c")]
SAN_ENV = dict(ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1", TSAN_OPTIONS="halt_on_error=1", SK_THREADS="4")
SD_CASES = ["batch", "cli_se", "cli_pe", "cli_pei", "cli_default", "background", "err_missing", "err_type",
            "err_pe_one_file", "err_b_and_B", "err_no_inf", "err_no_read1"]


@pytest.fixture(scope="module", params=["address,undefined", "thread"])
def exe(request, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("tcache") / ("target_cache_" + request.param.split(",")[0]))
    subprocess.run(["gcc", "-O1", "-g", "-fsanitize=" + request.param, "-fno-omit-frame-pointer", os.path.join(NATIVE, "target_cache_double.c")] + HOST +
                   ["-lz", "-lpthread", "-o", out], check=True)
    return out


def _env(**kw):
    return dict(SAN_ENV, **kw)


def test_version_2_reader_and_writer(exe, tmp_path):
    """files cut at every segment boundary, inside a segment header and inside a payload; a wrong version; a .skp offered as a .skt and
    a .skt to the version-1 reader; an empty-stream segment round-trips; a flipped payload byte and a changed length are CORRUPT"""
    p = subprocess.run([exe, "--format-drive", str(tmp_path)], env=dict(os.environ, **SAN_ENV), capture_output=True)
    assert p.returncode == 0 and p.stdout == b"ok\n", p.stderr.decode()[-3000:]
    assert os.listdir(tmp_path) == []


@pytest.mark.parametrize("name", SD_CASES)
def test_goldens_off_filling_served_at_64_byte_chunks(exe, name, tmp_path):
    fill, served = _skt.off_filling_served([exe], os.path.join(SD_DIR, name), tmp_path, env=_env(SK_SD_CHUNK_BYTES="64"))
    if name == "cli_se":
        assert fill == (0, 1, 0, 0) and served == (1, 0, 0, 0)
    if name == "cli_pe":
        assert fill == (0, 2, 0, 0) and served == (2, 0, 0, 0)
    if name == "batch":                                    # (a target named twice is served the second time, within the filling run)
        assert fill[1] >= 4 and fill[0] >= 1


@pytest.mark.parametrize("name,env", [("batch", {}), ("cli_pe", {"SK_SD_PACK": "1"}), ("background", {"SK_NO_SPLIT": "1"}), ("cli_pei", {"SK_SD_CHUNK_BYTES": "4096"})])
def test_goldens_at_other_settings(exe, name, env, tmp_path):
    """the default chunk size (one segment per file), chunks the host packed already, the serial parser, 4096-byte chunks"""
    _skt.off_filling_served([exe], os.path.join(SD_DIR, name), tmp_path, env=_env(**env))


def _own_case(tmp_path, name, files, argv):
    """a copy of the cli_se case with other targets"""
    d = tmp_path / name
    shutil.copytree(os.path.join(SD_DIR, "cli_se"), d)
    for f, data in files.items():
        (d / f).write_bytes(data)
    return str(d), argv


def _three(exe, d, argv, tmp_path, env=None, rc=0):
    """off, filling, served of a strain_detect command line in directory d: identical stdout, stderr and hits; returns the runs"""
    cache = tmp_path / "tc"
    cache.mkdir(parents=True, exist_ok=True)
    runs = []
    for k in range(3):
        out = tmp_path / ("o%d.gz" % k)
        e = dict(os.environ, **_env(SK_SD_CHUNK_BYTES="64", SK_SD_TIMING="1", **(env or {})))
        p = subprocess.run([exe] + argv + ["-o", str(out)] + (["--target-cache", str(cache)] if k else []), cwd=d, env=e, capture_output=True)
        for bad in (b"runtime error", b"AddressSanitizer", b"ThreadSanitizer"):
            assert bad not in p.stderr, p.stderr.decode()[-3000:]
        assert p.returncode == rc, p.stderr.decode()[-2000:]
        runs.append((p.stdout, _skt.quiet(p.stderr), gzip.open(out, "rb").read() if os.path.exists(out) and rc == 0 else None, _skt.stats(p.stderr)))
        _skt.no_temporaries(cache)
    assert runs[0][:3] == runs[1][:3] == runs[2][:3]
    return runs, cache


def _reads(seed, n, lo, hi, alphabet=b"ACGT"):
    import random
    rnd = random.Random(seed)
    return [bytes(rnd.choice(alphabet) for _ in range(rnd.randint(lo, hi))) for _ in range(n)]


def _strain_reads(d, n, seed):
    """reads cut from the case's strain, so that they hit"""
    import random
    rnd = random.Random(seed)
    g = b"".join(ln.strip() for ln in open(os.path.join(d, "strain.fa"), "rb") if not ln.startswith(b">"))
    out = []
    for _ in range(n):
        a = rnd.randrange(0, max(1, len(g) - 90))
        out.append(g[a: a + rnd.randint(20, 90)])
    return out


BASE = ["-r", "strain.fa", "-a", "inf.txt.gz"]


def test_odd_bytes_short_and_empty_records(exe, tmp_path):
    """a target with IUPAC letters, U and a CR (its segments kept as bytes), records shorter than k and empty ones"""
    src = os.path.join(SD_DIR, "cli_se")
    reads = _strain_reads(src, 40, 5)
    reads[3] = reads[3][:10] + b"R" + reads[3][11:]
    reads[7] = b""
    reads[8] = b"ACGT"
    reads[20] = reads[20].replace(b"T", b"U")
    fa = b"".join(b">r%d\n%s\n" % (i, r) for i, r in enumerate(reads)) + b">cr\r\n" + reads[1] + b"\r\n"
    d, argv = _own_case(tmp_path, "odd", {"odd.fa": fa, "odd.fa.gz": gzip.compress(fa)}, BASE + ["-t", "SE"])
    for f in ("odd.fa", "odd.fa.gz"):
        runs, cache = _three(exe, d, argv + ["-b", f], tmp_path / f.replace(".", "_"))
        assert runs[1][3] == (0, 1, 0, 0) and runs[2][3] == (1, 0, 0, 0)
        _, segs = _skt.segments(os.path.join(cache, os.listdir(cache)[0]))
        assert any(s["kind"] == 2 for s in segs) and any(s["kind"] == 1 and s["np"] for s in segs) and any(s["stream_len"] == 0 for s in segs)


def test_truncated_fastq_is_written_with_its_ending(exe, tmp_path):
    src = os.path.join(SD_DIR, "cli_se")
    reads = _strain_reads(src, 12, 9)
    fq = b"".join(b"@r%d\n%s\n+\n%s\n" % (i, r, b"I" * len(r)) for i, r in enumerate(reads)) + b"@last\n" + reads[0] + b"\n+\nII"
    d, argv = _own_case(tmp_path, "trunc", {"t.fq": fq}, BASE + ["-t", "SE", "-b", "t.fq"])
    runs, cache = _three(exe, d, argv, tmp_path / "w")
    assert runs[1][3] == (0, 1, 0, 0) and runs[2][3] == (1, 0, 0, 0)


def test_pe2_ends_before_pe1_leaves_nothing_for_pe1(exe, tmp_path):
    src = os.path.join(SD_DIR, "cli_se")
    r1, r2 = _strain_reads(src, 30, 1), _strain_reads(src, 30, 2)
    r2 = [r + b"ACGTACGTACGTACGTACGTACGTACGTACGT" for r in r2[:11]]      # (its last record reads as a read: the reference's message)
    fq = lambda rs: b"".join(b"@r%d\n%s\n+\n%s\n" % (i, r, b"I" * len(r)) for i, r in enumerate(rs))
    d, argv = _own_case(tmp_path, "short2", {"a_1.fq": fq(r1), "a_2.fq": fq(r2)}, BASE + ["-t", "PE", "-b", "a_1.fq", "-c", "a_2.fq"])
    runs, cache = _three(exe, d, argv, tmp_path / "w", rc=1)
    assert b"reached end of PE2" in runs[0][1]
    assert runs[1][3] == (0, 1, 0, 1) and runs[2][3] == (1, 0, 0, 1)
    assert [f.split(".")[0] for f in os.listdir(cache)] == ["a_2"]


def test_validity_stale_ro_and_damage(exe, tmp_path):
    d = os.path.join(SD_DIR, "cli_se")
    work = tmp_path / "case"
    shutil.copytree(d, work)
    cache = tmp_path / "tc"
    cache.mkdir()
    env = _env(SK_SD_CHUNK_BYTES="64")
    # ro on an empty directory writes nothing
    assert _skt.run_case([exe], str(work), tmp_path, cache=cache, env=env, mode="ro")[4] == (0, 0, 0, 0)
    assert os.listdir(cache) == []
    assert _skt.run_case([exe], str(work), tmp_path, cache=cache, env=env)[4] == (0, 1, 0, 0)
    (f,) = os.listdir(cache)
    path = os.path.join(cache, f)
    good = open(path, "rb").read()
    head, segs = _skt.segments(path)
    assert len(segs) > 3
    # the source touched: stale; left alone in ro, re-parsed and rewritten in rw
    target = [a for a in __import__("json").load(open(work / "case.json"))["argv"] if (work / a).is_file() and a.endswith((".fa", ".fq", ".gz")) and "inf" not in a and "strain" not in a][0]
    st = os.stat(work / target)
    os.utime(work / target, ns=(st.st_atime_ns, st.st_mtime_ns + 1_000_000_000))
    assert _skt.run_case([exe], str(work), tmp_path, cache=cache, env=env, mode="ro")[4] == (0, 0, 1, 0)
    assert open(path, "rb").read() == good
    assert _skt.run_case([exe], str(work), tmp_path, cache=cache, env=env)[4] == (0, 1, 1, 0)
    assert open(path, "rb").read() != good
    assert _skt.run_case([exe], str(work), tmp_path, cache=cache, env=env)[4] == (1, 0, 0, 0)
    good = open(path, "rb").read()
    # one payload byte flipped in the second segment: the run fails and names the file
    _skt.flip_payload_byte(path, [i for i, s in enumerate(segs) if s["payload_len"]][1])
    rc, _, err, _, _ = _skt.run_case([exe], str(work), tmp_path, cache=cache, env=env, check=False)
    assert rc != 0 and path.encode() in err
    # one length changed, the sum recomputed: rejected as corrupt, not tallied
    open(path, "wb").write(good)
    i = [k for k, s in enumerate(segs) if s["np"]][0]
    r = [k for k, l in enumerate(segs[i]["lens"]) if l >= 31][0]
    _skt.change_length(path, i, r, segs[i]["lens"][r] - 1)
    rc, _, err, _, _ = _skt.run_case([exe], str(work), tmp_path, cache=cache, env=env, check=False)
    assert rc != 0 and path.encode() in err
    # a directory that cannot be used: one warning, the run goes on uncached
    rc, out, err, hits, st = _skt.run_case([exe], str(work), tmp_path, cache=tmp_path / "nowhere", env=env, check=False)
    assert rc == 0 and err.count(b"cannot be used") == 1 and st is None and hits == open(work / "expected.hits", "rb").read()
