#!/usr/bin/env python3
"""kmer_scrub_count --prevalence on one MI355X: what the flag costs when it is off, and what it costs when it is on.

The job is strainer2_amd/cfg3.py cut down: N_GENOMES (200) genomes of 5 Mbp in -A, N_B (20) plain FASTQ files of READS_PER_FILE
(200,000) x 150 bp in -B (0.6 Gbase), the five-line -C list.  ROUNDS (5) alternating rounds of
  parent      the parent commit's program (--parent-exe), as it is
  off         this build, no flag
  on          this build, --prevalence --prevalence-items
  uncut       this build, no flag, SK_NO_SPLIT=1: the uncut plan alone
  off_A/on_A  -A alone (the -B list is one tiny file), off_B/on_B  -B alone (the -A list is one tiny file): a list's phase
each under its own `timeout -k 10`; the first failure ends the tool.  --legs parent,off,uncut --rotate --rounds 9: those runs alone,
every round starting one run later (no run always follows the same one).  Per run: wall seconds and the list phase ("scans" of the
program's SK_TIMING line); with the flag on also the folds' device time from HIP events and the HBM the slots take (the
"prevalence:" lines of SK_TIMING).  The count tables of parent, off and on are compared by md5 in every round.

Prints one JSON line; --out FILE also writes the table a person reads.  Environment: WORK (/tmp/sk_prevalence_bench)."""
import argparse
import hashlib
import json
import os
import re
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from strainer2_amd import cfg3  # noqa: E402

WORK = os.environ.get("WORK", "/tmp/sk_prevalence_bench")
SCANS = re.compile(r"table load [0-9.]+ s, scans ([0-9.]+) s")
FOLDS = re.compile(r"prevalence: (\S+): (\d+) item folds, ([0-9.]+) ms on the device")
SLOTS = re.compile(r"prevalence: (\S+): (\d+) item slots take ([0-9.]+) MB")


def run(exe, argv, env, what, limit_s=600):
    e = dict(os.environ, SK_TIMING="1")
    e.update(env)
    t = time.time()
    p = subprocess.run(["timeout", "-k", "10", str(limit_s), exe] + argv, cwd=WORK, env=e, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    wall = time.time() - t
    err = p.stderr.decode("latin-1")
    if p.returncode != 0:
        sys.stderr.write(f"{what} failed with status {p.returncode}:\n{err[-3000:]}\n")
        sys.exit(1)
    m = SCANS.search(err)
    r = {"wall_s": round(wall, 3), "list_phase_s": float(m.group(1)) if m else None, "md5": hashlib.md5(p.stdout).hexdigest()}
    folds = FOLDS.findall(err)
    if folds:
        r["folds"] = {os.path.basename(f[0]): {"items": int(f[1]), "device_ms": float(f[2])} for f in folds}
        r["slots_mb"] = max(float(s[2]) for s in SLOTS.findall(err))
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-exe", help="the parent commit's kmer_scrub_count (left out: no parent runs)")
    ap.add_argument("--exe", default=os.path.join(REPO, "strainer2_amd", "bin", "kmer_scrub_count"))
    ap.add_argument("--rounds", type=int, default=int(os.environ.get("ROUNDS", "5")))
    ap.add_argument("--genomes", type=int, default=int(os.environ.get("N_GENOMES", "200")))
    ap.add_argument("--b-files", type=int, default=int(os.environ.get("N_B", "20")))
    ap.add_argument("--reads-per-file", type=int, default=int(os.environ.get("READS_PER_FILE", "200000")))
    ap.add_argument("--procs", type=int, default=16)
    ap.add_argument("--legs", help="comma-separated subset of the runs, e.g. parent,off,uncut (default: all)")
    ap.add_argument("--rotate", action="store_true", help="every round starts one run later in the list: no run always follows the same one")
    ap.add_argument("--out")
    a = ap.parse_args()
    os.makedirs(WORK, exist_ok=True)
    t0 = time.time()
    argv = cfg3.write_all(WORK, procs=a.procs, n_genomes=a.genomes, n_b=a.b_files, reads_per_file=a.reads_per_file, repeat=1,
                          progress=lambda n, of: (sys.stderr.write("inputs: %d of %d files\n" % (n, of)), sys.stderr.flush()))
    argv = argv[:argv.index("-p")]                         # (no progress file: the runs share the directory)
    with open(os.path.join(WORK, "tiny.fa"), "w") as f:
        f.write(">t\n" + "ACGT" * 20 + "\n")
    with open(os.path.join(WORK, "tiny.txt"), "w") as f:
        f.write("tiny.fa\n")
    only_a = ["-r", "strain.fa", "-A", "A.txt", "-B", "tiny.txt"]
    only_b = ["-r", "strain.fa", "-A", "tiny.txt", "-B", "B.txt"]
    on = ["--prevalence=prev.tsv", "--prevalence-items=items.tsv"]
    legs = []
    if a.parent_exe:
        legs.append(("parent", a.parent_exe, argv, {}))
    legs += [("off", a.exe, argv, {}), ("on", a.exe, argv + on, {}), ("uncut", a.exe, argv, {"SK_NO_SPLIT": "1"}),
             ("off_A", a.exe, only_a, {}), ("on_A", a.exe, only_a + on, {}), ("off_B", a.exe, only_b, {}), ("on_B", a.exe, only_b + on, {})]
    if a.legs:
        legs = [leg for leg in legs if leg[0] in a.legs.split(",")]
    res = {"genomes": a.genomes, "b_files": a.b_files, "reads_per_file": a.reads_per_file, "rounds": a.rounds,
           "inputs_s": round(time.time() - t0, 1), "runs": {name: [] for name, *_ in legs}}
    for rnd in range(a.rounds):
        k = rnd % len(legs) if a.rotate else 0
        for name, exe, av, env in legs[k:] + legs[:k]:
            res["runs"][name].append(run(exe, av, env, f"{name} (round {rnd})"))
            sys.stderr.write("round %d %s: wall %.2f s, list phase %s s\n" % (rnd, name, res["runs"][name][-1]["wall_s"], res["runs"][name][-1]["list_phase_s"]))
            sys.stderr.flush()
        tables = {res["runs"][n][-1]["md5"] for n in ("parent", "off", "on", "uncut") if n in res["runs"]}
        if len(tables) != 1:
            sys.stderr.write(f"round {rnd}: the count tables differ\n")
            sys.exit(1)
    lines = ["kmer_scrub_count --prevalence: %d genomes in -A, %d x %d reads of 150 bp in -B, %d alternating rounds; the count tables of "
             "parent, off, on and uncut are identical (md5) in every round" % (a.genomes, a.b_files, a.reads_per_file, a.rounds), "",
             "%-8s %-28s %-28s" % ("run", "list phase s: median [min, max]", "wall s: median [min, max]")]
    summary = {}
    for name, *_ in legs:
        lp = [r["list_phase_s"] for r in res["runs"][name] if r["list_phase_s"] is not None]
        wl = [r["wall_s"] for r in res["runs"][name]]
        summary[name] = {"list_phase_s": [statistics.median(lp), min(lp), max(lp)] if lp else None, "wall_s": [statistics.median(wl), min(wl), max(wl)]}
        lines.append("%-8s %-28s %-28s" % (name, "%.2f [%.2f, %.2f]" % tuple(summary[name]["list_phase_s"]) if lp else "-",
                                           "%.2f [%.2f, %.2f]" % tuple(summary[name]["wall_s"])))
    folds = {}
    for r in res["runs"].get("on", []):
        for lst, f in r.get("folds", {}).items():
            folds.setdefault(lst, []).append(1e3 * f["device_ms"] / max(f["items"], 1))
    lines += ["", "item folds, device time from HIP events, us per item (median over the rounds): " +
              ", ".join("%s %.1f" % (k, statistics.median(v)) for k, v in sorted(folds.items())),
              "HBM the item slots take: %.1f MB" % max([r.get("slots_mb", 0.0) for r in res["runs"].get("on", [])] or [0.0])]
    res["summary"], res["fold_us_per_item"] = summary, {k: statistics.median(v) for k, v in folds.items()}
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n\n" + json.dumps(res) + "\n")
    sys.stderr.write("\n".join(lines) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
