#!/usr/bin/env python3
"""strain_detect with the targets parsed on the device (SK_DEVICE_PARSE=1) against the host parser threads (=0), one MI355X.

The workload is BASELINE configs[4]'s share of one GPU at a smaller size (strainer2_amd/cfg5.py): `strain_detect -S` with 32 strains
of 5 Mbp resident, over plain FASTA reads and over the same reads as plain FASTQ, each file listed --repeat times in the -B list.
The files are written once and read once before the timed runs: they are in the page cache.  Per form: one untimed run, then
SK_DEVICE_PARSE 0 and 1 ALTERNATE, --runs runs each, in this one invocation on this one box -- the comparison is the =0 leg of the
same run, never a figure from another day.  Every strain's hit file is hashed after every run and compared between the settings.

Reported per setting: wall time of the process (each run and the median), the time outside the pass (opening 32 strains: printed
on its own so that start-up does not hide the effect) and the pass itself, the main thread's wait for the decode side, the CPU
seconds of the process and of its parser and reader threads (all from SK_SD_TIMING=1), and the text pieces taken and declined.

    python tools/sd_text_ab.py [--reads 20000000] [--repeat 4] [--runs 3] [--out profiles/sd_text_parse_ab.txt]
"""
import argparse
import hashlib
import os
import re
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

NUM = r"([0-9]+\.?[0-9]*)"
PATTERNS = {
    "setup_s": re.compile(r"strain_detect timing: setup " + NUM + " s"),
    "wait_s": re.compile(r"waiting for the decode thread " + NUM + " s"),
    "total_s": re.compile(r"total before close " + NUM + " s"),
    "cpu_user_s": re.compile(r"CPU time of the process: user " + NUM + " s"),
    "cpu_sys_s": re.compile(r"CPU time of the process: user [0-9.]+ s \+ system " + NUM + " s"),
    "cpu_parsers_s": re.compile(r"of it parser threads " + NUM + " s"),
    "cpu_readers_s": re.compile(r"reader threads " + NUM + " s"),
    "taken": re.compile(r"text pieces parsed on the device: ([0-9]+) taken"),
    "declined": re.compile(r"taken, ([0-9]+) declined"),
}


def fasta_to_fastq(src, dst, rec, read_len, block=1 << 20):
    """reads.fa (records of `rec` bytes: ">r\\n" + bases + "\\n") as four-line FASTQ with a constant quality"""
    out_rec = 3 + read_len + 3 + read_len + 1
    with open(src, "rb") as f, open(dst, "wb") as g:
        while True:
            fa = np.frombuffer(f.read(block * rec), dtype=np.uint8)
            if not fa.size:
                break
            fa = fa.reshape(-1, rec)
            fq = np.full((fa.shape[0], out_rec), ord("I"), dtype=np.uint8)
            fq[:, :3] = np.frombuffer(b"@r\n", dtype=np.uint8)
            fq[:, 3:3 + read_len] = fa[:, 3:3 + read_len]
            fq[:, 3 + read_len:6 + read_len] = np.frombuffer(b"\n+\n", dtype=np.uint8)
            fq[:, -1] = 10
            g.write(fq.tobytes())


def run_once(exe, d, blist, setting):
    env = dict(os.environ, SK_SD_TIMING="1", SK_DEVICE_PARSE=str(setting))
    t0 = time.perf_counter()
    p = subprocess.run([exe, "-S", "strains.txt", "-B", blist], cwd=d, env=env, capture_output=True, timeout=600)
    wall = time.perf_counter() - t0
    err = p.stderr.decode(errors="replace")
    if p.returncode != 0:
        raise SystemExit(f"strain_detect failed ({p.returncode}) with SK_DEVICE_PARSE={setting}:\n{err[-3000:]}")
    r = {"wall_s": wall}
    for k, pat in PATTERNS.items():
        m = pat.search(err)
        r[k] = float(m.group(1)) if m else 0.0
    r["pass_s"] = r["total_s"] - r["setup_s"]
    r["cpu_s"] = r["cpu_user_s"] + r["cpu_sys_s"]
    return r


def hit_digests(d, n):
    out = []
    for s in range(n):
        with open(os.path.join(d, f"multi{s}.gz"), "rb") as f:
            import gzip
            out.append(hashlib.md5(gzip.decompress(f.read())).hexdigest())
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reads", type=int, default=20_000_000, help="reads of 150 bp in each file")
    ap.add_argument("--repeat", type=int, default=4, help="times each file is listed in the -B list")
    ap.add_argument("--runs", type=int, default=3, help="timed runs per setting (they alternate)")
    ap.add_argument("--dir", default=None, help="where the files go (default: a temporary directory, removed at the end)")
    ap.add_argument("--out", default=None, help="also write the report here")
    args = ap.parse_args()
    if args.runs < 3:
        raise SystemExit("at least three runs per setting")

    from strainer2_amd import cfg5                      # (writes the files with forked workers: before anything touches the GPU)
    import strainer2_amd as sk
    exe = sk.cli_path("strain_detect")
    d = args.dir or tempfile.mkdtemp(prefix="sd_text_ab_")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    try:
        t0 = time.perf_counter()
        cfg5.write_all(d, procs=min(16, os.cpu_count() or 1), reads=args.reads, prefix_reads=1,
                       progress=lambda n, m: print(f"writing the files: {n}/{m}", file=sys.stderr, flush=True))
        fasta_to_fastq(os.path.join(d, "reads.fa"), os.path.join(d, "reads.fq"), cfg5.REC, cfg5.READ_LEN)
        for form in ("fa", "fq"):
            with open(os.path.join(d, f"B_{form}.txt"), "w") as f:
                f.write(f"SE\treads.{form}\n" * args.repeat)
        gbase = args.reads * cfg5.READ_LEN * args.repeat / 1e9
        say(f"strain_detect -S, {cfg5.NSTRAINS} strains of {cfg5.STRAIN_BP / 1e6:.0f} Mbp resident, {args.reads} reads of {cfg5.READ_LEN} bp per file, "
            f"each file listed {args.repeat} times: {gbase:.1f} Gbase per run; files written in {time.perf_counter() - t0:.0f} s and in the page cache")
        say(f"SK_DEVICE_PARSE 0 and 1 alternate, {args.runs} timed runs each after one untimed run per form; same box, same invocation")
        for form, raw in (("fa", cfg5.REC / cfg5.READ_LEN), ("fq", (2 * cfg5.READ_LEN + 7) / cfg5.READ_LEN)):
            blist = f"B_{form}.txt"
            say()
            say(f"== plain {'FASTA' if form == 'fa' else 'FASTQ'} reads ({raw:.2f} raw bytes per base, {os.path.getsize(os.path.join(d, 'reads.' + form)) / 2**30:.2f} GiB per file)")
            run_once(exe, d, blist, 0)                   # untimed: page cache, code objects
            want = hit_digests(d, cfg5.NSTRAINS)
            res = {0: [], 1: []}
            for i in range(args.runs):
                for setting in (0, 1):
                    r = run_once(exe, d, blist, setting)
                    if hit_digests(d, cfg5.NSTRAINS) != want:
                        raise SystemExit(f"hit files differ between the settings ({form}, run {i}, SK_DEVICE_PARSE={setting})")
                    res[setting].append(r)
            say(f"   every one of the {cfg5.NSTRAINS} hit files equal in all {2 * args.runs + 1} runs")
            med = {}
            for setting in (0, 1):
                rs = res[setting]
                med[setting] = {k: statistics.median(r[k] for r in rs) for k in rs[0]}
                m = med[setting]
                say(f"   SK_DEVICE_PARSE={setting}: wall " + " ".join(f"{r['wall_s']:.2f}" for r in rs) + f" s, median {m['wall_s']:.2f} s")
                say(f"      outside the pass (strains opened) {m['setup_s']:.2f} s; the pass {m['pass_s']:.2f} s = {gbase / m['pass_s']:.1f} Gbase/s "
                    f"(runs: " + " ".join(f"{r['pass_s']:.2f}" for r in rs) + ")")
                say(f"      main thread waiting for the decode side {m['wait_s']:.2f} s (runs: " + " ".join(f"{r['wait_s']:.2f}" for r in rs) + ")")
                say(f"      CPU-seconds of the process {m['cpu_s']:.1f} (parser threads {m['cpu_parsers_s']:.1f}, reader threads {m['cpu_readers_s']:.1f})")
                say(f"      text pieces taken {int(m['taken'])}, declined {int(m['declined'])}")
            say(f"   the pass with the device parser: {med[1]['pass_s'] / med[0]['pass_s']:.2f} x the host parsers' time; "
                f"CPU-seconds {med[1]['cpu_s'] / med[0]['cpu_s']:.2f} x")
    finally:
        if not args.dir:
            shutil.rmtree(d, ignore_errors=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
