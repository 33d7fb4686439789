#!/usr/bin/env python3
"""The list scan's packed input cache, measured end to end (one MI355X): kmer_scrub_count over a .gz FASTQ list and over a plain FASTQ
list of --gbases each in /dev/shm, with the cache off, being filled, and served from -- the three alternating in one invocation,
three rounds, every round filling a fresh directory and serving from it, the tables compared (MD5 of stdout) inside the run.
The filling run has SK_NO_SPLIT=1: a big plain file that the plan would cut into byte ranges is not written otherwise, and then
nothing of the plain list would be served; off and served run with the plan's own cuts.

Every GPU step is one run of the program under `timeout` of its own; the first step that fails, or whose table differs, ends the
whole measurement.  Per step: wall time of the process, the list phase (the program's own "scans" figure, SK_TIMING), CPU-seconds
(user + system of the child), what the cache says it served and wrote, and the checksum's share of the decode threads' time.
Cache off is today's path and the yardstick; --parent-exe names kmer_scrub_count of a build of the parent commit, run three times
more with the cache off, to see that "off" has not moved.

    python tools/pack_cache_bench.py [--gbases 2] [--parent-exe PATH] [--out profiles/pack_cache_bench.txt]
"""
import argparse
import hashlib
import os
import re
import resource
import shutil
import statistics
import subprocess
import sys
import tempfile
import time
import zlib

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from text_parse_bench import dna, reads_text  # noqa: E402  (the generators of the other list-scan measurements)

EXE = os.path.join(REPO, "strainer2_amd", "bin", "kmer_scrub_count")
SCANS = re.compile(rb"timing: key set [^\n]*? scans ([0-9.]+) s")
CACHE = re.compile(rb"pack cache: (\S+): (\d+) items served, (\d+) written, (\d+) stale, (\d+) not cached; ([0-9.]+) MB of cache files; "
                   rb"summed over the threads: checksums ([0-9.]+) s, reading ([0-9.]+) s, writing ([0-9.]+) s")
ITEMS = re.compile(rb"timing: (\S+): \d+ decode threads, \d+ items, \d+ chunks; summed over the threads: in items ([0-9.]+) s")


class StepFailed(Exception):
    pass


def row(rs, key, spec):
    return " ".join(format(r[key], spec) for r in rs)


def step(exe, argv, env, limit, table_path):
    """one run of the program under its own time limit -> measurements; raises StepFailed (nothing more is started then)"""
    r0 = resource.getrusage(resource.RUSAGE_CHILDREN)
    t0 = time.perf_counter()
    with open(table_path, "wb") as out:
        p = subprocess.run(["timeout", "-k", "10", str(limit), exe] + argv, env=env, stdout=out, stderr=subprocess.PIPE)
    wall = time.perf_counter() - t0
    r1 = resource.getrusage(resource.RUSAGE_CHILDREN)
    if p.returncode != 0:
        raise StepFailed(f"exit status {p.returncode}: {p.stderr.decode(errors='replace')[-1500:]}")
    h = hashlib.md5()
    with open(table_path, "rb") as f:
        for blk in iter(lambda: f.read(1 << 24), b""):
            h.update(blk)
    m = SCANS.search(p.stderr)
    big = {c[0]: c for c in CACHE.findall(p.stderr)}
    items = {c[0]: float(c[1]) for c in ITEMS.findall(p.stderr)}
    return dict(wall=wall, cpu=(r1.ru_utime + r1.ru_stime) - (r0.ru_utime + r0.ru_stime), scans=float(m.group(1)) if m else float("nan"),
                md5=h.hexdigest(), cache=big, items=items)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gbases", type=float, default=2.0, help="bases per list")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--limit", type=int, default=120, help="seconds one run of the program may take")
    ap.add_argument("--parent-exe", default=None, help="kmer_scrub_count of a build of the parent commit")
    ap.add_argument("--out", default=None)
    ap.add_argument("--tmp", default="/dev/shm" if os.path.isdir("/dev/shm") else None)
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    env = {k: v for k, v in os.environ.items() if not k.startswith("SK_") or k in ("SK_THREADS", "SK_DEVICE")}
    env["SK_TIMING"] = "1"
    ok = True
    with tempfile.TemporaryDirectory(dir=args.tmp) as tmp:
        rng = np.random.default_rng(7)
        strain = dna(rng, 500_000).tobytes()
        with open(os.path.join(tmp, "strain.fa"), "wb") as f:
            f.write(b">strain\n" + strain + b"\n")
        with open(os.path.join(tmp, "tiny.fa"), "wb") as f:
            f.write(b">t\n" + strain[:5000] + b"\n")
        with open(os.path.join(tmp, "A.txt"), "w") as f:
            f.write(os.path.join(tmp, "tiny.fa") + "\n")
        per = 500_000                                            # reads per file (0.075 Gbase); one text, one deflate, many names
        text = bytearray(reads_text(rng, per, True))
        seq = np.frombuffer(text, dtype=np.uint8).reshape(per, -1)
        src = np.frombuffer(strain, dtype=np.uint8)
        for i in range(0, per, 50):                              # (every 50th read is the strain's: the table has something in it)
            a = int(rng.integers(0, len(strain) - 150))
            seq[i, 16:166] = src[a:a + 150]
        text = bytes(text)
        nfiles = max(int(args.gbases * 1e9 / (per * 150)), 2)
        co = zlib.compressobj(6, zlib.DEFLATED, 31)
        gz = co.compress(text) + co.flush()
        lists = {}
        for kind, blob, ext in (("FASTQ .gz", gz, ".fq.gz"), ("plain FASTQ", text, ".fq")):
            names = []
            for i in range(nfiles):
                p = os.path.join(tmp, f"r{i}{ext}")
                with open(p, "wb") as f:
                    f.write(blob)
                names.append(p)
            lst = os.path.join(tmp, "B" + ext + ".txt")
            with open(lst, "w") as f:
                f.write("".join(p + "\n" for p in names))
            lists[kind] = (lst, len(blob) * nfiles)
        gbase = nfiles * per * 150 / 1e9
        say(f"kmer_scrub_count -r <0.5 Mbp strain> -A <one small file> -B <list>, {nfiles} files of {per} 150-base FASTQ reads per list "
            f"({gbase:.2f} Gbase), in {tmp}; {os.cpu_count()} CPUs seen, SK_THREADS={env.get('SK_THREADS', 'default')}; "
            f"modes alternate, {args.rounds} rounds, a fresh cache directory every round; filling runs with SK_NO_SPLIT=1")
        try:
            for kind, (lst, raw) in lists.items():
                argv = ["-r", os.path.join(tmp, "strain.fa"), "-A", os.path.join(tmp, "A.txt"), "-B", lst]
                res = {"off": [], "filling": [], "served": []}
                md5 = None
                for rnd in range(args.rounds):
                    cache = os.path.join(tmp, f"cache_{rnd}")
                    for mode in ("off", "filling", "served"):
                        e = dict(env) if mode == "off" else dict(env, SK_PACK_CACHE=cache)
                        if mode == "filling":                    # (items cut into byte ranges are not written: the fill leaves big plain files whole)
                            e["SK_NO_SPLIT"] = "1"
                        r = step(EXE, argv, e, args.limit, os.path.join(tmp, "table.tsv"))
                        md5 = md5 or r["md5"]
                        if r["md5"] != md5:
                            raise StepFailed(f"{kind}, round {rnd}, {mode}: the table differs from the first run's")
                        res[mode].append(r)
                    shutil.rmtree(cache, ignore_errors=True)
                say(f"{kind}: {raw / 1e9:.2f} GB on disk, tables equal in all {3 * args.rounds} runs (MD5 {md5})")
                for mode in ("off", "filling", "served"):
                    rs = res[mode]
                    c = [r["cache"].get(lst.encode()) for r in rs]
                    extra = ""
                    if c[0]:
                        share = [float(x[6]) / r["items"].get(lst.encode(), float("nan")) for x, r in zip(c, rs)]
                        extra = (f"; items served {' '.join(x[1].decode() for x in c)}, written {' '.join(x[2].decode() for x in c)}; cache files "
                                 f"{float(c[0][5]):.0f} MB; checksums {' '.join(x[6].decode() for x in c)} s summed over the threads = "
                                 f"{' '.join(f'{100 * s:.1f}' for s in share)} % of their time in items; reading {' '.join(x[7].decode() for x in c)} s, "
                                 f"writing {' '.join(x[8].decode() for x in c)} s")
                    say(f"    {mode:8s} wall {row(rs, 'wall', '.3f')} s; list phase (scans) {row(rs, 'scans', '.2f')} s "
                        f"= {gbase / statistics.median(r['scans'] for r in rs):.1f} Gbase/s at the median; CPU-seconds {row(rs, 'cpu', '.1f')}{extra}")
                wins = [s["scans"] < o["scans"] and s["wall"] < o["wall"] for s, o in zip(res["served"], res["off"])]
                say(f"    served beats off in {sum(wins)} of {len(wins)} rounds (list phase and wall); filling costs "
                    f"{statistics.median(r['wall'] for r in res['filling']) / statistics.median(r['wall'] for r in res['off']):.2f}x off's wall time at the median")
                if kind == "FASTQ .gz" and not all(wins):
                    ok = False
                    say("    SERVED DOES NOT BEAT OFF ON THE .gz LIST IN EVERY ROUND")
                if args.parent_exe:
                    rs = [step(args.parent_exe, argv, dict(env), args.limit, os.path.join(tmp, "table.tsv")) for _ in range(3)]
                    if any(r["md5"] != md5 for r in rs):
                        raise StepFailed(f"{kind}: the parent build prints another table")
                    lo, hi = min(r["scans"] for r in rs), max(r["scans"] for r in rs)
                    mine = statistics.median(r["scans"] for r in res["off"])
                    say(f"    parent build, cache off x3: wall {row(rs, 'wall', '.3f')} s; list phase {row(rs, 'scans', '.2f')} s; "
                        f"this build's off median {mine:.2f} s is {'inside' if lo <= mine <= hi else 'OUTSIDE'} that spread [{lo:.2f}, {hi:.2f}]")
        except StepFailed as x:
            ok = False
            say(f"STOPPED: {x}")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
