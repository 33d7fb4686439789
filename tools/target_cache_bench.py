#!/usr/bin/env python3
"""strain_detect's target cache, measured end to end (one MI355X): `strain_detect -S` with 8 strains of strainer2_amd/cfg5.py over a -B
list of 150-base FASTQ targets of --gbases in /dev/shm, once as .gz files and once plain, with the cache off, being filled, and
served from -- the three alternating in one invocation, three rounds, every round filling a fresh directory and serving from it; the
MD5 of every strain's decompressed output is compared inside the run.

Every GPU step is one run of the program under `timeout` of its own; the first step that fails, or whose outputs differ, ends the
whole measurement.  Per step: the pass (the program's own "total before close" less "setup", SK_SD_TIMING), wall time of the process,
CPU-seconds (user + system of the child) and the cache's own line.  Cache off is the parent's path and the yardstick; --parent-exe
names strain_detect of a build of the parent commit, run three times more, to see that "off" has not moved.

    python tools/target_cache_bench.py [--gbases 1.5] [--parent-exe PATH] [--out profiles/target_cache_bench.txt]
"""
import argparse
import gzip
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
from strainer2_amd import cfg5  # noqa: E402
from text_parse_bench import reads_text  # noqa: E402  (the generator of the other ingest measurements)

EXE = os.path.join(REPO, "strainer2_amd", "bin", "strain_detect")
NSTRAINS = 8
PASS = re.compile(rb"strain_detect timing: setup ([0-9.]+) s,.*?total before close ([0-9.]+) s")
CACHE = re.compile(rb"target cache: \S+: (\d+) files served, (\d+) written, (\d+) stale, (\d+) not cached; checksums ([0-9.]+) s, reading ([0-9.]+) s, "
                   rb"writing ([0-9.]+) s, waiting for the device pack ([0-9.]+) s")


class StepFailed(Exception):
    pass


def row(rs, key, spec):
    return " ".join(format(r[key], spec) for r in rs)


def step(exe, argv, env, limit, cwd):
    """one run of the program under its own time limit -> measurements; raises StepFailed (nothing more is started then)"""
    r0 = resource.getrusage(resource.RUSAGE_CHILDREN)
    t0 = time.perf_counter()
    p = subprocess.run(["timeout", "-k", "10", str(limit), exe] + argv, env=env, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    wall = time.perf_counter() - t0
    r1 = resource.getrusage(resource.RUSAGE_CHILDREN)
    if p.returncode != 0:
        raise StepFailed(f"exit status {p.returncode}: {p.stderr.decode(errors='replace')[-1500:]}")
    h = hashlib.md5(p.stdout)
    for s in range(NSTRAINS):
        with gzip.open(os.path.join(cwd, f"out{s}.gz"), "rb") as f:
            for blk in iter(lambda: f.read(1 << 24), b""):
                h.update(blk)
    m = PASS.search(p.stderr)
    c = CACHE.search(p.stderr)
    return dict(wall=wall, cpu=(r1.ru_utime + r1.ru_stime) - (r0.ru_utime + r0.ru_stime), md5=h.hexdigest(),
                passed=float(m.group(2)) - float(m.group(1)) if m else float("nan"), cache=c.groups() if c else None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gbases", type=float, default=1.5, help="bases per list")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--limit", type=int, default=120, help="seconds one run of the program may take")
    ap.add_argument("--parent-exe", default=None, help="strain_detect of a build of the parent commit")
    ap.add_argument("--out", default=None)
    ap.add_argument("--tmp", default="/dev/shm" if os.path.isdir("/dev/shm") else None)
    args = ap.parse_args()
    if args.parent_exe:
        args.parent_exe = os.path.abspath(args.parent_exe)     # (the runs' working directory is the data's)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    env = {k: v for k, v in os.environ.items() if not k.startswith("SK_") or k in ("SK_THREADS", "SK_DEVICE")}
    env["SK_SD_TIMING"] = "1"
    ok = True
    with tempfile.TemporaryDirectory(dir=args.tmp) as tmp:
        rng = np.random.default_rng(11)
        genome = []
        for s in range(NSTRAINS):
            cfg5.write_strain(tmp, s)
            genome.append(cfg5.strain(s))
        with open(os.path.join(tmp, "S.txt"), "w") as f:
            f.write("".join(f"s{s}.fa\ts{s}.inf\tout{s}.gz\n" for s in range(NSTRAINS)))
        per = 500_000                                            # reads per file (0.075 Gbase); one text, one deflate, many names
        text = bytearray(reads_text(rng, per, True))
        seq = np.frombuffer(text, dtype=np.uint8).reshape(per, -1)
        for i in range(0, per, 50):                              # (2 % of the reads are a strain's, as in cfg5)
            g = genome[int(rng.integers(0, NSTRAINS))]
            a = int(rng.integers(0, g.size - 150))
            seq[i, 16:166] = g[a:a + 150]
        text = bytes(text)
        nfiles = max(int(args.gbases * 1e9 / (per * 150)), 2)
        co = zlib.compressobj(6, zlib.DEFLATED, 31)
        gz = co.compress(text) + co.flush()
        lists = {}
        for kind, blob, ext in (("FASTQ .gz", gz, ".fq.gz"), ("plain FASTQ", text, ".fq")):
            for i in range(nfiles):
                with open(os.path.join(tmp, f"r{i}{ext}"), "wb") as f:
                    f.write(blob)
            lst = "B" + ext + ".txt"
            with open(os.path.join(tmp, lst), "w") as f:
                f.write("".join(f"SE\tr{i}{ext}\n" for i in range(nfiles)))
            lists[kind] = (lst, len(blob) * nfiles)
        gbase = nfiles * per * 150 / 1e9
        say(f"strain_detect -S <{NSTRAINS} cfg5 strains of {cfg5.STRAIN_BP} bp> -B <list>, {nfiles} files of {per} 150-base FASTQ reads per list "
            f"({gbase:.2f} Gbase), in {tmp}; {os.cpu_count()} CPUs seen, SK_THREADS={env.get('SK_THREADS', 'default')}; "
            f"modes alternate, {args.rounds} rounds, a fresh cache directory every round")
        try:
            for kind, (lst, raw) in lists.items():
                argv = ["-S", "S.txt", "-B", lst]
                res = {"off": [], "filling": [], "served": []}
                md5 = None
                for rnd in range(args.rounds):
                    cache = os.path.join(tmp, f"cache_{rnd}")
                    os.makedirs(cache)
                    for mode in ("off", "filling", "served"):
                        r = step(EXE, argv + ([] if mode == "off" else ["--target-cache", cache]), dict(env), args.limit, tmp)
                        md5 = md5 or r["md5"]
                        if r["md5"] != md5:
                            raise StepFailed(f"{kind}, round {rnd}, {mode}: the outputs differ from the first run's")
                        want = {"off": None, "filling": (0, nfiles), "served": (nfiles, 0)}[mode]
                        got = (int(r["cache"][0]), int(r["cache"][1])) if r["cache"] else None
                        if got != want:
                            raise StepFailed(f"{kind}, round {rnd}, {mode}: the cache says (served, written) = {got}, expected {want}")
                        res[mode].append(r)
                    mb = sum(os.path.getsize(os.path.join(cache, f)) for f in os.listdir(cache)) / 1e6
                    shutil.rmtree(cache, ignore_errors=True)
                say(f"{kind}: {raw / 1e9:.2f} GB on disk, {mb:.0f} MB of cache files; outputs equal in all {3 * args.rounds} runs (MD5 over stdout and the "
                    f"{NSTRAINS} decompressed -o files {md5})")
                for mode in ("off", "filling", "served"):
                    rs = res[mode]
                    extra = ""
                    if rs[0]["cache"]:
                        c = [r["cache"] for r in rs]
                        extra = (f"; checksums {' '.join(x[4].decode() for x in c)} s, reading {' '.join(x[5].decode() for x in c)} s, "
                                 f"writing {' '.join(x[6].decode() for x in c)} s, waiting for the device pack {' '.join(x[7].decode() for x in c)} s")
                    say(f"    {mode:8s} pass {row(rs, 'passed', '.2f')} s = {gbase / statistics.median(r['passed'] for r in rs):.2f} Gbase/s at the median; "
                        f"wall {row(rs, 'wall', '.2f')} s; CPU-seconds {row(rs, 'cpu', '.1f')}{extra}")
                wins = [s["passed"] < o["passed"] and s["wall"] < o["wall"] for s, o in zip(res["served"], res["off"])]
                say(f"    served beats off in {sum(wins)} of {len(wins)} rounds (pass and wall); filling costs "
                    f"{statistics.median(r['wall'] for r in res['filling']) / statistics.median(r['wall'] for r in res['off']):.2f}x off's wall time at the median")
                if args.parent_exe:
                    rs = [step(args.parent_exe, argv, dict(env), args.limit, tmp) for _ in range(3)]
                    if any(r["md5"] != md5 for r in rs):
                        raise StepFailed(f"{kind}: the parent build writes other outputs")
                    lo, hi = min(r["passed"] for r in rs), max(r["passed"] for r in rs)
                    mine = statistics.median(r["passed"] for r in res["off"])
                    say(f"    parent build x3: pass {row(rs, 'passed', '.2f')} s; wall {row(rs, 'wall', '.2f')} s; CPU-seconds {row(rs, 'cpu', '.1f')}; "
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
