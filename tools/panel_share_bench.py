#!/usr/bin/env python3
"""strain_detect -S --panel-share=FILE, measured end to end (one MI355X): the strains of strainer2_amd/cfg5.py (5 Mbp each, 1 % of
the 31-mers informative) as a panel of 32 (one union table, one call of sk_union_share) and of 64 (two union tables, four calls),
against a short -B list of 150-base FASTA reads in /dev/shm.  Runs without the flag, with it and (--parent-exe) of the parent build alternate, --rounds rounds.

Per run: the panel-share line of SK_SD_TIMING=1 (milliseconds from before the first call to after the last, and the number of
calls), the union tables' build time from the same log, the pass (the program's own "total before close" less "setup") and the wall
time of the process.  The coverage tables' MD5 is compared inside the measurement: every run must write the same bytes, and every
run with the flag the same panel table.  --parent-exe names strain_detect of a build of the parent commit, which runs without the
flag in the same rounds: the claim to support is "flag off: the parent's time within the parent's own run-to-run spread".

Every GPU step is one run of the program under `timeout` of its own; the first step that fails, or whose tables differ, ends the
whole measurement.

    python tools/panel_share_bench.py [--rounds 3] [--strains 32,64] [--parent-exe PATH] [--out profiles/panel_share_bench.txt]
"""
import argparse
import hashlib
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from strainer2_amd import cfg5, synth  # noqa: E402

EXE = os.path.join(REPO, "strainer2_amd", "bin", "strain_detect")
PASS = re.compile(rb"strain_detect timing: setup ([0-9.]+) s,.*?total before close ([0-9.]+) s")
SHARE = re.compile(rb"strain_detect timing: panel share ([0-9.]+) ms, (\d+) call")
UNIONS = re.compile(rb"strain_detect timing: (\d+) union table\(s\) for \d+ strains in ([0-9.]+) s")


class StepFailed(Exception):
    pass


def row(rs, key, spec):
    return " ".join(format(r[key], spec) for r in rs)


def step(exe, argv, env, limit, cwd, ns):
    """one run of the program under its own time limit -> measurements; raises StepFailed (nothing more is started then)"""
    for f in [f"out{s}.coverage_depth" for s in range(ns)] + ["panel.tsv"]:
        if os.path.exists(os.path.join(cwd, f)):
            os.remove(os.path.join(cwd, f))
    t0 = time.perf_counter()
    p = subprocess.run(["timeout", "-k", "10", str(limit), exe] + argv, env=env, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    wall = time.perf_counter() - t0
    if p.returncode != 0:
        raise StepFailed(f"exit status {p.returncode}: {p.stderr.decode(errors='replace')[-1500:]}")
    h = hashlib.md5()
    for s in range(ns):
        with open(os.path.join(cwd, f"out{s}.coverage_depth"), "rb") as f:
            h.update(f.read())
    panel = None
    if os.path.exists(os.path.join(cwd, "panel.tsv")):
        with open(os.path.join(cwd, "panel.tsv"), "rb") as f:
            panel = f.read()
    m, sh, un = PASS.search(p.stderr), SHARE.search(p.stderr), UNIONS.search(p.stderr)
    return dict(wall=wall, md5=h.hexdigest(), panel=panel, passed=float(m.group(2)) - float(m.group(1)) if m else float("nan"),
                setup=float(m.group(1)) if m else float("nan"), share_ms=float(sh.group(1)) if sh else float("nan"), calls=int(sh.group(2)) if sh else 0,
                unions=int(un.group(1)) if un else 0, unions_s=float(un.group(2)) if un else float("nan"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--strains", default="32,64")
    ap.add_argument("--reads", type=int, default=1_000_000, help="150-base reads of the one target (2 %% of them a strain's)")
    ap.add_argument("--limit", type=int, default=150, help="seconds one run of the program may take")
    ap.add_argument("--parent-exe", default=None, help="strain_detect of a build of the parent commit")
    ap.add_argument("--out", default=None)
    ap.add_argument("--tmp", default="/dev/shm" if os.path.isdir("/dev/shm") else None)
    args = ap.parse_args()
    if args.parent_exe:
        args.parent_exe = os.path.abspath(args.parent_exe)     # (the runs' working directory is the data's)
    counts = [int(x) for x in args.strains.split(",")]
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    env = {k: v for k, v in os.environ.items() if not k.startswith("SK_") or k in ("SK_THREADS", "SK_DEVICE")}
    env["SK_SD_TIMING"] = "1"
    ok = True
    with tempfile.TemporaryDirectory(dir=args.tmp) as tmp:
        rng = np.random.default_rng(12)
        genome = []
        for s in range(max(counts)):
            cfg5.write_strain(tmp, s)
            if s < min(counts):
                genome.append(cfg5.strain(s))
        for ns in counts:
            with open(os.path.join(tmp, f"S{ns}.txt"), "w") as f:
                f.write("".join(f"s{s}.fa\ts{s}.inf\tout{s}.kmer_hits.gz\n" for s in range(ns)))
        blk = synth._rand_bases(rng, args.reads * 150).reshape(args.reads, 150)
        for i in range(0, args.reads, 50):
            g = genome[int(rng.integers(0, len(genome)))]
            a = int(rng.integers(0, g.size - 150))
            blk[i] = g[a:a + 150]
        fa = np.empty((args.reads, 154), dtype=np.uint8)
        fa[:, :3] = np.frombuffer(b">r\n", dtype=np.uint8)
        fa[:, 3:153] = blk
        fa[:, 153] = 10
        with open(os.path.join(tmp, "reads.fa"), "wb") as f:
            f.write(fa.tobytes())
        with open(os.path.join(tmp, "B.txt"), "w") as f:
            f.write("SE\treads.fa\n")
        say(f"strain_detect -S <cfg5 strains of {cfg5.STRAIN_BP} bp> -B <one file of {args.reads} 150-base FASTA reads> --coverage-only "
            f"[--panel-share=panel.tsv], in {tmp}; {os.cpu_count()} CPUs seen, SK_THREADS={env.get('SK_THREADS', 'default')}; "
            f"flag off, flag on{' and the parent build' if args.parent_exe else ''} alternate, {args.rounds} rounds")
        try:
            for ns in counts:
                argv = ["-S", f"S{ns}.txt", "-B", "B.txt", "--coverage-only"]
                res = {"off": [], "on": [], "parent": []}
                md5 = panel = None
                for rnd in range(args.rounds):
                    for tag, flags in (("off", []), ("on", ["--panel-share=panel.tsv"]), ("parent", [])):
                        if tag == "parent" and not args.parent_exe:
                            continue
                        r = step(args.parent_exe if tag == "parent" else EXE, argv + flags, dict(env), args.limit, tmp, ns)
                        md5 = md5 or r["md5"]
                        if r["md5"] != md5:
                            raise StepFailed(f"{ns} strains, round {rnd}, {tag}: the coverage tables differ from the first run's")
                        if (r["panel"] is not None) != (tag == "on"):
                            raise StepFailed(f"{ns} strains, round {rnd}, {tag}: panel.tsv {'is missing' if tag == 'on' else 'was written'}")
                        if tag == "on":
                            panel = panel or r["panel"]
                            if r["panel"] != panel:
                                raise StepFailed(f"{ns} strains, round {rnd}: the panel table differs from the first run's")
                        res[tag].append(r)
                on = res["on"]
                rows = [ln.split(b"\t") for ln in panel.split(b"\n")[1:-1]]
                cross = sum(int(r[4]) for r in rows if r[0] != r[1])
                say(f"{ns} strains: {on[0]['unions']} union table(s); the coverage tables are the same bytes in all runs (MD5 {md5}), the panel table "
                    f"in all {args.rounds} (MD5 {hashlib.md5(panel).hexdigest()}, {len(rows)} pairs, kmers_a of the first strain {int(rows[0][2])}, "
                    f"informative_a {int(rows[0][3])}, shared k-mers summed over the pairs a != b {cross})")
                say(f"    panel share: {row(on, 'share_ms', '.3f')} ms, {on[0]['calls']} call(s) of sk_union_share; the union tables' build in the same "
                    f"runs: {row(on, 'unions_s', '.2f')} s")
                names = {"off": "flag off", "on": "--panel-share=panel.tsv", "parent": "parent build, flag off"}
                for tag, rs in res.items():
                    if rs:
                        say(f"    {names[tag]}: pass {row(rs, 'passed', '.2f')} s; setup {row(rs, 'setup', '.2f')} s; wall {row(rs, 'wall', '.2f')} s")
                med = {t: {k: statistics.median(r[k] for r in rs) for k in ("passed", "wall")} for t, rs in res.items() if rs}
                if statistics.median(r["share_ms"] for r in on) > 1e3 * statistics.median(r["unions_s"] for r in on):
                    say("    NOTE: the panel share takes longer than the union tables' build")
                if res["parent"]:                                    # the yardstick: the parent's medians; the margin: its own spread
                    for k in ("passed", "wall"):
                        spread = max(r[k] for r in res["parent"]) - min(r[k] for r in res["parent"])
                        for tag in ("off", "on"):
                            diff = med[tag][k] - med["parent"][k]
                            say(f"    {k}: {names[tag]} median {med[tag][k]:.3f} s against the parent's {med['parent'][k]:.3f} s ({diff:+.3f}; the parent's "
                                f"spread over {args.rounds} rounds is {spread:.3f}): {'within' if diff <= spread else 'BEYOND'} it")
        except StepFailed as x:
            ok = False
            say(f"STOPPED: {x}")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
