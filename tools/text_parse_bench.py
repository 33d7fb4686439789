#!/usr/bin/env python3
"""Plain text parsed on the device: what it costs and what it buys (one MI355X).

(a) sk_text_parse_device alone on resident text -- 64 MiB of wrapped FASTA, of one-line FASTA reads and of FASTQ: device
    milliseconds (HIP events around the passes, sk_text_timing) and GB/s of text, median of --runs runs after a preheat (as
    tools/exp_grid.py --preheat-ms), next to the 0.66 ms a 32 MiB piece needs over the 51 GB/s link.
(b) skh_scan_list over a plain-text list in the page cache, three alternating runs each of SK_DEVICE_PARSE=0 and 1: a list of
    5 Mbp wrapped-FASTA genomes and a FASTQ list of the same base count.  Wall time of the scan, CPU-seconds of the process, the
    columns compared in the run.  The baseline is the =0 leg of the same run on the same box, never a stored figure.

    python tools/text_parse_bench.py [--mib 64] [--gbases 2] [--out profiles/text_parse_bench.txt]
"""
import argparse
import os
import resource
import statistics
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
LINK_MS_PER_32MIB = 0.66          # 32 MiB over the 51 GB/s host link


def dna(rng, n):
    return np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n, dtype=np.uint8)]


def wrapped_fasta(rng, nbases, width=60, name=b">genome"):
    rows = nbases // width                                  # (whole lines)
    body = np.full((rows, width + 1), 10, dtype=np.uint8)
    body[:, :width] = dna(rng, rows * width).reshape(rows, width)
    return name + b" 5 Mbp\n" + body.tobytes()


def reads_text(rng, nreads, fastq, length=150):
    seq = dna(rng, nreads * length).reshape(nreads, length)
    head = np.frombuffer((b"@" if fastq else b">") + b"read.0000000/1", dtype=np.uint8)
    cols = [np.broadcast_to(head, (nreads, head.size)), np.full((nreads, 1), 10, np.uint8), seq, np.full((nreads, 1), 10, np.uint8)]
    if fastq:
        cols += [np.full((nreads, 1), ord("+"), np.uint8), np.full((nreads, 1), 10, np.uint8), np.full((nreads, length), ord("I"), np.uint8),
                 np.full((nreads, 1), 10, np.uint8)]
    return np.concatenate(cols, axis=1).tobytes()


def leg_a(sk, ctx, say, mib, runs, preheat_ms):
    rng = np.random.default_rng(1)
    n = mib << 20
    texts = {"wrapped FASTA (60 columns, 5 Mbp records)": b"".join(wrapped_fasta(rng, 5_000_000) for _ in range(n // 5_083_000 + 1)),
             "FASTA reads (150 bases, one line)": reads_text(rng, n // 167 + 1, False),
             "FASTQ reads (150 bases)": reads_text(rng, n // 320 + 1, True)}
    say(f"(a) sk_text_parse_device on {mib} MiB of resident text, median of {runs} runs after {preheat_ms:.0f} ms of preheat; "
        f"the link needs {LINK_MS_PER_32MIB * mib / 32:.2f} ms for as many bytes")
    for name, text in texts.items():
        text = text[:n]
        text = text[: text.rfind(b"\n>" if text[:1] == b">" else b"\n@") + 1]       # whole records
        d_text = ctx.dev_alloc(len(text) + 16)
        ctx.dev_upload(d_text, np.frombuffer(text, dtype=np.uint8))

        def once():
            info, d_out, _ = ctx.parse_text_device(d_text, len(text), True)
            ms = ctx.text_timing()
            ctx.dev_free(d_out)
            return info, ms
        t0 = time.perf_counter()
        while (time.perf_counter() - t0) * 1e3 < preheat_ms:
            once()
        got = [once() for _ in range(runs)]
        info = got[0][0]
        ms = statistics.median(m for _, m in got)
        say(f"    {name:44s} {len(text) / 2**20:6.1f} MiB  {ms:7.3f} ms  {len(text) / ms / 1e6:7.1f} GB/s of text   "
            f"status {info.status} form {info.form} records {info.nrecords} bases {info.bases}")
        ctx.dev_free(d_text)


def leg_b(sk, say, gbases, tmp):
    rng = np.random.default_rng(2)
    strain = dna(rng, 2_000_000).tobytes()
    spath = os.path.join(tmp, "strain.fa")
    with open(spath, "wb") as f:
        f.write(b">strain\n" + strain + b"\n")
    ks = sk.Keyset.from_file(spath)
    lists = {}
    ngen = max(int(gbases * 1e9 / 5e6), 2)
    names = []
    for i in range(ngen):
        p = os.path.join(tmp, f"g{i}.fa")
        with open(p, "wb") as f:
            f.write(wrapped_fasta(rng, 5_000_000))
        names.append(p)
    lists["wrapped-FASTA genomes"] = names
    names = []
    per = 2_000_000                                         # reads per FASTQ file (0.3 Gbase)
    for i in range(max(int(gbases * 1e9 / (per * 150)), 1)):
        p = os.path.join(tmp, f"r{i}.fq")
        with open(p, "wb") as f:
            f.write(reads_text(rng, per, True))
        names.append(p)
    lists["FASTQ reads"] = names
    say(f"(b) skh_scan_list, plain text in the page cache, alternating SK_DEVICE_PARSE=0 / 1, three runs each ({os.cpu_count()} CPUs seen, "
        f"SK_THREADS={os.environ.get('SK_THREADS', 'default')})")
    with sk.KmerContext(0) as ctx:
        ctx.load_keyset(ks, 4)
        for lname, files in lists.items():
            lst = os.path.join(tmp, "list.txt")
            with open(lst, "w") as f:
                f.write("".join(p + "\n" for p in files))
            raw = sum(os.path.getsize(p) for p in files)
            for p in files:                                  # warm page cache
                with open(p, "rb") as f:
                    while f.read(1 << 24):
                        pass
            res = {0: [], 1: []}
            cols = {}
            for rep in range(3):
                for on in (0, 1):
                    ctx.set_option("device_parse", on)
                    ctx.zero_counts(1)
                    ctx.sync()
                    ctx.text_stats(reset=True)
                    r0 = resource.getrusage(resource.RUSAGE_SELF)
                    t0 = time.perf_counter()
                    bases = ctx.scan_list(lst, 1)
                    ctx.sync()
                    dt = time.perf_counter() - t0
                    r1 = resource.getrusage(resource.RUSAGE_SELF)
                    cpu = (r1.ru_utime + r1.ru_stime) - (r0.ru_utime + r0.ru_stime)
                    col = ctx.counts(1)
                    if on in cols:
                        assert np.array_equal(cols[on], col)
                    cols[on] = col
                    res[on].append((dt, cpu, bases, ctx.text_stats()))
            assert np.array_equal(cols[0], cols[1]) and res[0][0][2] == res[1][0][2], "the two legs differ"
            say(f"    {lname}: {len(files)} files, {raw / 1e9:.2f} GB of text, {res[0][0][2] / 1e9:.2f} Gbase, columns equal")
            for on in (0, 1):
                dts = [r[0] for r in res[on]]
                cpus = [r[1] for r in res[on]]
                say(f"        SK_DEVICE_PARSE={on}: wall {' '.join(f'{x:.3f}' for x in dts)} s (median {statistics.median(dts):.3f} s, "
                    f"{res[on][0][2] / statistics.median(dts) / 1e9:.1f} Gbase/s), CPU-seconds {' '.join(f'{x:.2f}' for x in cpus)}, "
                    f"pieces on the device {res[on][-1][3][0]}, declined {res[on][-1][3][1]}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=64)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--preheat-ms", type=float, default=300.0)
    ap.add_argument("--gbases", type=float, default=2.0, help="bases per list of leg (b)")
    ap.add_argument("--skip-b", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--tmp", default="/dev/shm" if os.path.isdir("/dev/shm") else None)
    args = ap.parse_args()
    import strainer2_amd as sk
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    with sk.KmerContext(0) as ctx:
        leg_a(sk, ctx, say, args.mib, max(args.runs, 5), args.preheat_ms)
    if not args.skip_b:
        with tempfile.TemporaryDirectory(dir=args.tmp) as tmp:
            leg_b(sk, say, args.gbases, tmp)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
