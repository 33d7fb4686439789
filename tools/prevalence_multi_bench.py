#!/usr/bin/env python3
"""kmer_scrub_count -S --prevalence=SUFFIX on one MI355X: what the flag costs when it is off, and whether the one pass beats what users
do today when it is on.

  flag off   `-S` of this build against the parent commit's program (--parent-exe) on the end-to-end inputs of
             tools/scrub_multi_bench.py: E2E_STRAINS (8) cfg5 strains, -A one genome, -B one plain FASTQ of READS (10,000,000) x 150 bp
             reads.  OFF_ROUNDS (9) rounds, every round starting one run later (no run always follows the same one).  Per run: wall
             seconds and the list phase (the passes' seconds of the program's SK_TIMING line); the outfiles of the two are compared by
             md5 in the first round.
  flag on    PANELS ("8,32") cfg5 strains over the lists of tools/prevalence_bench.py (strainer2_amd/cfg3.py: N_GENOMES (200) genomes
             of 5 Mbp in -A, N_B (20) plain FASTQ files of READS_PER_FILE (200,000) x 150 bp in -B), PANEL_ROUNDS (2) rounds of
               S_off   `-S`, no flag
               S_on    `-S --prevalence=.prev.tsv --prevalence-items=.items.tsv`
               chain   what users do today: the N `-r <strain> --prevalence=F --prevalence-items=G` runs in sequence (stdout discarded)
             Per run: wall seconds, the list phase; for S_on the union folds' device time from HIP events and the HBM the slots take
             (the `prevalence:` line of SK_TIMING).  Every strain's prevalence table of S_on is compared with the chain's by md5 in
             the first round.  The ratio chain / S_on is reported, not asserted.

Each program runs under its own `timeout -k 10`; the first failure ends the tool.  Prints one JSON line; --out FILE also writes the
table a person reads.  Environment: WORK (/tmp/sk_prevalence_multi_bench)."""
import argparse
import hashlib
import json
import os
import re
import statistics
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from strainer2_amd import cfg3, cfg5, synth  # noqa: E402

WORK = os.environ.get("WORK", "/tmp/sk_prevalence_multi_bench")
PASSES = re.compile(r"(\d+) union pass\(es\) \+ (\d+) single pass\(es\) ([0-9.]+) s")
SCANS = re.compile(r"table load [0-9.]+ s, scans ([0-9.]+) s")
FOLDS = re.compile(r"prevalence: (\d+) union\(s\) with (\d+) item slot\(s\) each take ([0-9.]+) MB of HBM; (\d+) union folds, ([0-9.]+) ms on the device")


def md5(path):
    h = hashlib.md5()
    with open(path, "rb") as f:
        for blk in iter(lambda: f.read(1 << 24), b""):
            h.update(blk)
    return h.hexdigest()


def say(text):
    sys.stderr.write(text + "\n")
    sys.stderr.flush()


def run(exe, argv, cwd, what, limit_s=600, stdout=subprocess.DEVNULL):
    t = time.time()
    p = subprocess.run(["timeout", "-k", "10", str(limit_s), exe] + argv, cwd=cwd, env=dict(os.environ, SK_TIMING="1"), stdout=stdout, stderr=subprocess.PIPE)
    wall = time.time() - t
    err = p.stderr.decode("latin-1")
    if p.returncode != 0:
        say(f"{what} failed with status {p.returncode}:\n{err[-3000:]}")
        sys.exit(1)
    return wall, err


def run_S(exe, argv, cwd, what):
    wall, err = run(exe, argv, cwd, what)
    m = PASSES.search(err)
    r = {"wall_s": round(wall, 3), "list_phase_s": float(m.group(3)) if m else None, "unions": int(m.group(1)) if m else None}
    f = FOLDS.findall(err)
    if f:
        r["slots_mb"] = sum(float(x[2]) for x in f)
        r["slots_per_union"] = int(f[0][1])
        r["folds"] = sum(int(x[3]) for x in f)
        r["fold_device_ms"] = round(sum(float(x[4]) for x in f), 3)
    return r


def spread(v):
    return [round(statistics.median(v), 3), round(min(v), 3), round(max(v), 3)]


def fmt(v):
    return "%.2f [%.2f, %.2f]" % tuple(v) if v else "-"


def write_strains(n):
    paths = []
    for s in range(n):
        p = os.path.join(WORK, f"s{s}.fa")
        if not os.path.exists(p):
            with open(p, "wb") as f:
                f.write(b">s%d\n" % s + cfg5.strain(s).tobytes() + b"\n")
        paths.append(p)
    return paths


def flag_off(a, lines, res):
    reads = int(os.environ.get("READS", "10000000"))
    e2e = int(os.environ.get("E2E_STRAINS", "8"))
    t0 = time.time()
    paths = write_strains(e2e)
    stream, _ = synth.make_reads([cfg5.strain(s) for s in range(32)], reads)
    fq = os.path.join(WORK, "reads.fq")
    r2 = stream.reshape(-1, 151)[:, :150]
    with open(fq, "wb") as f:                              # (the FASTQ of tools/scrub_multi_bench.py's end-to-end leg)
        for lo in range(0, r2.shape[0], 500_000):
            blk = r2[lo:lo + 500_000]
            rec = np.empty((blk.shape[0], 4 + 151 + 2 + 151), dtype=np.uint8)
            rec[:, 0:4] = np.frombuffer(b"@rd\n", dtype=np.uint8)
            rec[:, 4:154] = blk
            rec[:, 154] = 10
            rec[:, 155:157] = np.frombuffer(b"+\n", dtype=np.uint8)
            rec[:, 157:307] = ord("I")
            rec[:, 307] = 10
            f.write(rec.tobytes())
    del stream, r2
    with open(os.path.join(WORK, "A1.txt"), "w") as f:
        f.write(paths[e2e - 1] + "\n")
    with open(os.path.join(WORK, "B1.txt"), "w") as f:
        f.write(fq + "\n")
    legs = [("parent", a.parent_exe), ("off", a.exe)]
    for name, _ in legs:
        with open(os.path.join(WORK, f"S_{name}.txt"), "w") as f:
            f.write("".join(f"{p}\t{WORK}/{name}{s}.tsv\n" for s, p in enumerate(paths)))
    say("flag off: inputs in %.1f s" % (time.time() - t0))
    runs = {name: [] for name, _ in legs}
    for rnd in range(a.off_rounds):
        k = rnd % len(legs)
        for name, exe in legs[k:] + legs[:k]:
            runs[name].append(run_S(exe, ["-S", f"S_{name}.txt", "-A", "A1.txt", "-B", "B1.txt"], WORK, f"{name} (round {rnd})"))
            say("round %d %s: wall %.2f s, list phase %s s" % (rnd, name, runs[name][-1]["wall_s"], runs[name][-1]["list_phase_s"]))
        if rnd == 0:
            for s in range(e2e):
                if md5(f"{WORK}/parent{s}.tsv") != md5(f"{WORK}/off{s}.tsv"):
                    say(f"flag off: outfile {s} differs from the parent's")
                    sys.exit(1)
    for name, _ in legs:
        for s in range(e2e):
            os.unlink(f"{WORK}/{name}{s}.tsv")
    os.unlink(fq)
    out = {name: {"list_phase_s": spread([r["list_phase_s"] for r in runs[name]]), "wall_s": spread([r["wall_s"] for r in runs[name]])} for name in runs}
    res["flag_off"] = {"strains": e2e, "reads": reads, "rounds": a.off_rounds, "summary": out, "runs": runs}
    lines += ["flag off: -S, %d cfg5 strains, -A one genome, -B one plain FASTQ of %d x 150 bp; %d rotated rounds; outfiles identical to the parent's (md5)"
              % (e2e, reads, a.off_rounds), "%-8s %-32s %-32s" % ("run", "list phase s: median [min, max]", "wall s: median [min, max]")]
    lines += ["%-8s %-32s %-32s" % (n, fmt(out[n]["list_phase_s"]), fmt(out[n]["wall_s"])) for n in out] + [""]


def panel(a, n, ldir, lines, res):
    paths = write_strains(n)
    for tag in ("off", "on"):
        with open(os.path.join(WORK, f"P{n}_{tag}.txt"), "w") as f:
            f.write("".join(f"{p}\t{WORK}/p{tag}{s}.tsv\n" for s, p in enumerate(paths)))
    lists = ["-A", "A.txt", "-B", "B.txt"]
    on = ["--prevalence=.prev.tsv", "--prevalence-items=.items.tsv"]
    runs = {"S_off": [], "S_on": [], "chain": []}
    for rnd in range(a.panel_rounds):
        runs["S_off"].append(run_S(a.exe, ["-S", os.path.join(WORK, f"P{n}_off.txt")] + lists, ldir, f"S_off {n} (round {rnd})"))
        say("panel %d round %d S_off: %s" % (n, rnd, runs["S_off"][-1]))
        runs["S_on"].append(run_S(a.exe, ["-S", os.path.join(WORK, f"P{n}_on.txt")] + lists + on, ldir, f"S_on {n} (round {rnd})"))
        say("panel %d round %d S_on: %s" % (n, rnd, runs["S_on"][-1]))
        wall, phase = 0.0, 0.0
        for s, p in enumerate(paths):
            w, err = run(a.exe, ["-r", p] + lists + [f"--prevalence={WORK}/chain.prev.tsv", f"--prevalence-items={WORK}/chain.items.tsv"], ldir, f"chain {n}/{s} (round {rnd})")
            m = SCANS.search(err)
            wall += w
            phase += float(m.group(1)) if m else 0.0
            if rnd == 0 and md5(f"{WORK}/chain.prev.tsv") != md5(f"{WORK}/pon{s}.tsv.prev.tsv"):
                say(f"panel {n}: strain {s}'s prevalence table differs from the single run's")
                sys.exit(1)
            if rnd == 0 and md5(f"{WORK}/chain.items.tsv") != md5(f"{WORK}/pon{s}.tsv.items.tsv"):
                say(f"panel {n}: strain {s}'s item records differ from the single run's")
                sys.exit(1)
        runs["chain"].append({"wall_s": round(wall, 3), "list_phase_s": round(phase, 3)})
        say("panel %d round %d chain: %s" % (n, rnd, runs["chain"][-1]))
    for s in range(n):
        for f in (f"poff{s}.tsv", f"pon{s}.tsv", f"pon{s}.tsv.prev.tsv", f"pon{s}.tsv.items.tsv"):
            os.unlink(os.path.join(WORK, f))
    out = {k: {"list_phase_s": spread([r["list_phase_s"] for r in v]), "wall_s": spread([r["wall_s"] for r in v])} for k, v in runs.items()}
    last = runs["S_on"][-1]
    ratio = out["chain"]["wall_s"][0] / out["S_on"]["wall_s"][0]
    fold_us = 1e3 * statistics.median(r["fold_device_ms"] for r in runs["S_on"]) / max(last.get("folds", 1), 1)
    res["panels"][str(n)] = {"rounds": a.panel_rounds, "summary": out, "ratio_chain_over_S_on_wall": round(ratio, 2), "fold_us": round(fold_us, 1),
                             "folds": last.get("folds"), "fold_device_ms": [r.get("fold_device_ms") for r in runs["S_on"]],
                             "slots_mb": last.get("slots_mb"), "slots_per_union": last.get("slots_per_union"), "unions": last.get("unions"), "runs": runs}
    lines += ["flag on: %d cfg5 strains over %d genomes in -A and %d x %d reads in -B; %d rounds; every prevalence table and items file of S_on equals the single run's (md5)"
              % (n, a.genomes, a.b_files, a.reads_per_file, a.panel_rounds), "%-8s %-32s %-32s" % ("run", "list phase s: median [min, max]", "wall s: median [min, max]")]
    lines += ["%-8s %-32s %-32s" % (k, fmt(out[k]["list_phase_s"]), fmt(out[k]["wall_s"])) for k in ("S_off", "S_on", "chain")]
    lines += ["chain / S_on (wall): %.2f;  %s union folds in %s union(s), device time %.1f ms in all, %.1f us each;  item slots: %s per union, %.0f MB of HBM"
              % (ratio, last.get("folds"), last.get("unions"), statistics.median(r["fold_device_ms"] for r in runs["S_on"]), fold_us,
                 last.get("slots_per_union"), last.get("slots_mb") or 0.0), ""]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-exe", help="the parent commit's kmer_scrub_count (left out: no flag-off comparison)")
    ap.add_argument("--exe", default=os.path.join(REPO, "strainer2_amd", "bin", "kmer_scrub_count"))
    ap.add_argument("--off-rounds", type=int, default=int(os.environ.get("OFF_ROUNDS", "9")))
    ap.add_argument("--panels", default=os.environ.get("PANELS", "8,32"), help="comma-separated panel sizes; empty: no flag-on runs")
    ap.add_argument("--panel-rounds", type=int, default=int(os.environ.get("PANEL_ROUNDS", "2")))
    ap.add_argument("--genomes", type=int, default=int(os.environ.get("N_GENOMES", "200")))
    ap.add_argument("--b-files", type=int, default=int(os.environ.get("N_B", "20")))
    ap.add_argument("--reads-per-file", type=int, default=int(os.environ.get("READS_PER_FILE", "200000")))
    ap.add_argument("--procs", type=int, default=16)
    ap.add_argument("--out")
    a = ap.parse_args()
    a.exe = os.path.abspath(a.exe)                         # (the programs run in the inputs' directories)
    a.parent_exe = os.path.abspath(a.parent_exe) if a.parent_exe else None
    os.makedirs(WORK, exist_ok=True)
    res, lines = {"panels": {}}, ["kmer_scrub_count -S --prevalence=SUFFIX (tools/prevalence_multi_bench.py)", ""]
    sizes = [int(x) for x in a.panels.split(",") if x]
    if sizes:                                              # (the lists first: cfg3.write_all forks its workers)
        t0 = time.time()
        ldir = os.path.join(WORK, "lists")
        cfg3.write_all(ldir, procs=a.procs, n_genomes=a.genomes, n_b=a.b_files, reads_per_file=a.reads_per_file, repeat=1)
        say("lists in %.1f s" % (time.time() - t0))
    if a.parent_exe:
        flag_off(a, lines, res)
    for n in sizes:
        panel(a, n, ldir, lines, res)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n" + json.dumps(res) + "\n")
    say("\n".join(lines))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
