#!/usr/bin/env python3
"""strain_detect --coverage-only against --coverage-depth, measured end to end (one MI355X): `strain_detect -S` with 8 and with 32
strains of strainer2_amd/cfg5.py over a -B list of 150-base FASTQ targets of --gbases in /dev/shm (the targets of
tools/target_cache_bench.py), once as .gz files and once plain; the two flags alternate, three rounds.  The MD5 of the strains'
tables is compared inside the run: both flags must write the same bytes, and --coverage-only no hit list.

Every GPU step is one run of the program under `timeout` of its own; the first step that fails, or whose tables differ, ends the
whole measurement.  Per step: the pass (the program's own "total before close" less "setup", SK_SD_TIMING), wall time of the
process, CPU-seconds (user + system of the child) and the bytes of scan results copied from the device (SK_SD_RESULT_BYTES).
--parent-exe names strain_detect of a build of the parent commit, which runs --coverage-depth three times per case: the figures the
new flag is to be set against.

--regions W measures --coverage-regions instead: --coverage-only without and with `--coverage-regions --region-window W` alternate
(the coverage tables must be the same bytes, and every run with the flag must write the same region tables), --parent-exe runs plain
--coverage-only, and each line also carries the accumulators' device time -- their folds and their target sweeps, summed over the
run (SK_SD_TIMING; the parent build does not report it).

--spectrum D measures --coverage-spectrum in the same way: --coverage-only without and with `--coverage-spectrum --spectrum-max D`
alternate, the parent build's plain --coverage-only runs behind them, and the summary sets the new build's plain runs and the runs
with the flag against the parent's medians and the parent's own run-to-run spread (max - min over its rounds).

--recurrence measures --coverage-recurrence --recurrence-pairs in the same way (the samples are the list's files), and each line
with the flag also carries the device time of the marks (summed over the targets) and of the one finish, histogram and pair table
apart.

    python tools/coverage_only_bench.py [--gbases 1.5] [--parent-exe PATH] [--out profiles/coverage_only_bench.txt]
    python tools/coverage_only_bench.py --regions 100000 --rounds 5 [--parent-exe PATH] [--out profiles/coverage_regions_bench.txt]
    python tools/coverage_only_bench.py --spectrum 255 --rounds 5 --parent-exe PATH [--out profiles/coverage_spectrum_bench.txt]
    python tools/coverage_only_bench.py --recurrence --rounds 5 --parent-exe PATH [--out profiles/coverage_recurrence_bench.txt]
    python tools/coverage_only_bench.py --thresholds [--threshold-list 0,1,2] --rounds 3 --parent-exe PATH [--out profiles/coverage_thresholds_bench.txt]
    python tools/coverage_only_bench.py --scrub-sweep --rounds 3 --parent-exe PATH [--out profiles/coverage_scrub_sweep_bench.txt]
    python tools/coverage_only_bench.py --support [--pairs] --rounds 3 --parent-exe PATH [--out profiles/coverage_support_bench.txt]
    python tools/coverage_only_bench.py --background --rounds 3 --parent-exe PATH [--out profiles/coverage_background_bench.txt]
    python tools/coverage_only_bench.py --rarefaction --rounds 3 --parent-exe PATH [--out profiles/coverage_rarefaction_bench.txt]

--rarefaction measures --coverage-rarefaction (the default list of six fractions) like --thresholds; each line with the flag also
carries the device time of the classifying passes and pair counts (a part of the folds), the same per fold in microseconds (a fold: one
unit's share of one run counted on the device) and the finishing passes of all targets.
--kinds plain (or gz) keeps one kind of target: a second measurement of one case over more rounds.

--support measures --coverage-support (--pairs: with --support-pairs=FILE) like --thresholds: the parent's plain --coverage-only runs in
turn with this build's plain runs and its runs with the flag; each line with the flag also carries the device time of the takes (a
part of the folds) and of the finishes.

--background measures --coverage-background --background-spectrum like --thresholds; every run of this build also reports the scan
kernels' summed device time (SK_SD_SCAN_TIMING=1: TALLY alone without the flag, TALLY and the COUNT scans with it -- the difference is
what the count scans add), and each line with the flag the finishing sweeps of all targets (wall time of the calls).

--scrub-sweep measures --coverage-scrub-sweep like --thresholds (class files of 8 fractions are made up for the strains' lists: the
class pass does not care where the classes come from), then step 2 alone at 8 fractions against 1 (kmer_scrub_filter over one
strain's count table) and one fused kmer_scrub_count -S --scrub <8 fractions> --detect run against 8 fused runs of one fraction
each, whose coverage tables must carry the sweep table's numbers.
"""
import argparse
import hashlib
import os
import re
import resource
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
PASS = re.compile(rb"strain_detect timing: setup ([0-9.]+) s,.*?total before close ([0-9.]+) s")
ACC = re.compile(rb"coverage accumulators on the device: folds ([0-9.]+) ms, target sweeps ([0-9.]+) ms")
REC = re.compile(rb"recurrence on the device: marks ([0-9.]+) ms \((\d+) targets\), finish: histogram ([0-9.]+) ms, pairs ([0-9.]+) ms")
THR = re.compile(rb"thresholds on the device: (\d+) thresholds, finishing passes ([0-9.]+) ms")
SUPT = re.compile(rb"support on the device: takes ([0-9.]+) ms \(inside the folds above\), finishes ([0-9.]+) ms")
BGT = re.compile(rb"background: (\d+) count scans beside the TALLY launches, finishing sweeps ([0-9.]+) ms")
SCN = re.compile(rb"scan kernels on the device: ([0-9.]+) ms in (\d+) launches")
RAR = re.compile(rb"rarefaction on the device: (\d+) fractions, classifying passes ([0-9.]+) ms \(inside the folds above\), finishing passes ([0-9.]+) ms")
SWP = re.compile(rb"scrub sweep on the device: class passes ([0-9.]+) ms")
SWEEP_LIST = "0.5,0.4,0.3,0.2,0.1,0.05,0.02,0.01"
BYTES = re.compile(rb"scan results copied from the device: (\d+) bytes; --coverage-only: (\d+) runs counted on the device, (\d+) replayed")


STDERR_DIR = None


class StepFailed(Exception):
    pass


def row(rs, key, spec):
    return " ".join(format(r[key], spec) for r in rs)


def step(exe, argv, env, limit, cwd, ns, hit_lists):
    """one run of the program under its own time limit -> measurements; raises StepFailed (nothing more is started then)"""
    for s in range(ns):
        for f in (f"out{s}.gz", f"out{s}.gz.coverage_depth", f"out{s}.gz.coverage_regions", f"out{s}.gz.coverage_spectrum",
                  f"out{s}.gz.coverage_recurrence", f"out{s}.gz.coverage_recurrence_pairs", f"out{s}.gz.coverage_thresholds",
                  f"out{s}.gz.coverage_scrub_sweep", f"out{s}.gz.coverage_support", f"out{s}.gz.coverage_background", f"out{s}.gz.coverage_background_spectrum",
                  f"out{s}.gz.coverage_rarefaction"):
            if os.path.exists(os.path.join(cwd, f)):
                os.remove(os.path.join(cwd, f))
    r0 = resource.getrusage(resource.RUSAGE_CHILDREN)
    t0 = time.perf_counter()
    p = subprocess.run(["timeout", "-k", "10", str(limit), exe] + argv, env=env, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    wall = time.perf_counter() - t0
    r1 = resource.getrusage(resource.RUSAGE_CHILDREN)
    if STDERR_DIR:                                           # (--stderr-dir: every run's timing lines, for a closer look)
        with open(os.path.join(STDERR_DIR, f"run{len(os.listdir(STDERR_DIR)):03d}.err"), "wb") as f:
            f.write((" ".join([exe] + argv) + "\n").encode() + p.stderr)
    if p.returncode != 0:
        raise StepFailed(f"exit status {p.returncode}: {p.stderr.decode(errors='replace')[-1500:]}")
    h = hashlib.md5()
    for s in range(ns):
        if os.path.exists(os.path.join(cwd, f"out{s}.gz")) != hit_lists:
            raise StepFailed(f"out{s}.gz {'is missing' if hit_lists else 'was written'}")
        with open(os.path.join(cwd, f"out{s}.gz.coverage_depth"), "rb") as f:
            h.update(f.read())
    hr = hashlib.md5()
    for s in range(ns):
        for ext in ("coverage_regions", "coverage_spectrum", "coverage_recurrence", "coverage_recurrence_pairs", "coverage_thresholds", "coverage_scrub_sweep", "coverage_support", "coverage_background", "coverage_background_spectrum", "coverage_rarefaction"):    # (the table beside the coverage table, whichever the run wrote)
            if os.path.exists(os.path.join(cwd, f"out{s}.gz.{ext}")):
                with open(os.path.join(cwd, f"out{s}.gz.{ext}"), "rb") as f:
                    hr.update(f.read())
    m = PASS.search(p.stderr)
    b = BYTES.search(p.stderr)
    a = ACC.search(p.stderr)
    rc = REC.search(p.stderr)
    th = THR.search(p.stderr)
    sw = SWP.search(p.stderr)
    su = SUPT.search(p.stderr)
    bg = BGT.search(p.stderr)
    sc = SCN.search(p.stderr)
    ra = RAR.search(p.stderr)
    return dict(rarcls=float(ra.group(2)) if ra else float("nan"), rarfin=float(ra.group(3)) if ra else float("nan"),
                bgscans=int(bg.group(1)) if bg else -1, bgsweep=float(bg.group(2)) if bg else float("nan"), scan=float(sc.group(1)) if sc else float("nan"),
                launches=int(sc.group(2)) if sc else -1,
                take=float(su.group(1)) if su else float("nan"), supfin=float(su.group(2)) if su else float("nan"), cls=float(sw.group(1)) if sw else float("nan"), thr=float(th.group(2)) if th else float("nan"), mark=float(rc.group(1)) if rc else float("nan"), hist=float(rc.group(3)) if rc else float("nan"), gram=float(rc.group(4)) if rc else float("nan"),
                fold=float(a.group(1)) if a else float("nan"), sweep=float(a.group(2)) if a else float("nan"), md5r=hr.hexdigest(), wall=wall, cpu=(r1.ru_utime + r1.ru_stime) - (r0.ru_utime + r0.ru_stime), md5=h.hexdigest(),
                passed=float(m.group(2)) - float(m.group(1)) if m else float("nan"),
                d2h=int(b.group(1)) if b else -1, dev=int(b.group(2)) if b else -1, replayed=int(b.group(3)) if b else -1)


def regions_case(say, args, env, tmp, ns, kind, argv):
    """--coverage-only without and with --coverage-regions, alternating; the parent build's plain --coverage-only behind them"""
    with_rg = ["--coverage-only", "--coverage-regions", "--region-window", str(args.regions)]
    res = {"plain": [], "regions": []}
    md5 = md5r = None
    for rnd in range(args.rounds):
        for tag, flags in (("plain", ["--coverage-only"]), ("regions", with_rg)):
            r = step(EXE, argv + flags, dict(env), args.limit, tmp, ns, False)
            md5 = md5 or r["md5"]
            if r["md5"] != md5:
                raise StepFailed(f"{ns} strains, {kind}, round {rnd}, {tag}: the coverage tables differ from the first run's")
            if tag == "regions":
                md5r = md5r or r["md5r"]
                if r["md5r"] != md5r:
                    raise StepFailed(f"{ns} strains, {kind}, round {rnd}: the region tables differ from the first run's")
            res[tag].append(r)
    say(f"{ns} strains, {kind}: the {ns} coverage tables are the same bytes in all {2 * args.rounds} runs (MD5 {md5}), "
        f"the region tables in all {args.rounds} (MD5 {md5r})")
    names = {"plain": "--coverage-only", "regions": f"... --coverage-regions --region-window {args.regions}"}
    for tag, rs in res.items():
        say(f"    {names[tag]}: pass {row(rs, 'passed', '.2f')} s; wall {row(rs, 'wall', '.2f')} s; accumulators on the device: folds "
            f"{row(rs, 'fold', '.2f')} ms, target sweeps {row(rs, 'sweep', '.3f')} ms; runs on the device {rs[0]['dev']}, replayed {rs[0]['replayed']}")
    med = {t: {k: statistics.median(r[k] for r in rs) for k in ("passed", "wall", "fold", "sweep")} for t, rs in res.items()}
    say("    with regions / without at the medians: pass %.2f, wall %.2f, folds %.2f, target sweeps %.2f" %
        tuple(med["regions"][k] / med["plain"][k] if med["plain"][k] else float("nan") for k in ("passed", "wall", "fold", "sweep")))
    if args.parent_exe:
        rs = [step(args.parent_exe, argv + ["--coverage-only"], dict(env), args.limit, tmp, ns, False) for _ in range(args.rounds)]
        if any(r["md5"] != md5 for r in rs):
            raise StepFailed(f"{ns} strains, {kind}: the parent build writes other tables")
        say(f"    parent build, --coverage-only x{args.rounds}: pass {row(rs, 'passed', '.2f')} s; wall {row(rs, 'wall', '.2f')} s (same tables)")


def spectrum_case(say, args, env, tmp, ns, kind, argv, recurrence=False, thresholds=False, sweep=False, support=False, background=False,
                  rarefaction=False):
    """--coverage-only without and with --coverage-spectrum (recurrence: --coverage-recurrence --recurrence-pairs; thresholds:
    --coverage-thresholds [--threshold-list ..]), alternating; the parent build's plain --coverage-only behind them -- with
    thresholds: in turn with them, round by round -- and the new build's medians set against the parent's"""
    with_sp = ["--coverage-only", "--coverage-spectrum", "--spectrum-max", str(args.spectrum)]
    word, label = "spectrum", f"... --coverage-spectrum --spectrum-max {args.spectrum}"
    if recurrence:
        with_sp = ["--coverage-only", "--coverage-recurrence", "--recurrence-pairs"]
        word, label = "recurrence", "... --coverage-recurrence --recurrence-pairs"
    if thresholds:
        with_sp = ["--coverage-only", "--coverage-thresholds"] + (["--threshold-list", args.threshold_list] if args.threshold_list else [])
        word, label = "thresholds", "... " + " ".join(with_sp[1:])
    if sweep:                                                # (measured like the thresholds: the parent's runs in turn, folds compared too)
        with_sp = ["--coverage-only", "--coverage-scrub-sweep"]
        word, label = "scrub sweep", "... --coverage-scrub-sweep"
        thresholds = True
    if support:                                              # (measured like the thresholds: the parent's runs in turn, folds compared too)
        with_sp = ["--coverage-only", "--coverage-support"] + (["--support-pairs=" + os.path.join(tmp, "support_pairs.tsv")] if args.pairs else [])
        word, label = "support", "... --coverage-support" + (" --support-pairs=FILE" if args.pairs else "")
        thresholds = True
    if background:                                           # (measured like the thresholds: the parent's runs in turn, folds compared too)
        with_sp = ["--coverage-only", "--coverage-background", "--background-spectrum"]
        word, label = "background", "... --coverage-background --background-spectrum"
        thresholds = True
        env = dict(env, SK_SD_SCAN_TIMING="1")
    if rarefaction:                                          # (measured like the thresholds: the parent's runs in turn, folds compared too)
        with_sp = ["--coverage-only", "--coverage-rarefaction"]
        word, label = "rarefaction", "... --coverage-rarefaction"
        thresholds = True
    res = {"plain": [], "spectrum": [], "parent": []}
    md5 = md5s = None
    for rnd in range(args.rounds):
        turns = [("plain", ["--coverage-only"]), ("spectrum", with_sp)]
        if thresholds and args.parent_exe:
            turns.append(("parent", ["--coverage-only"]))
        for tag, flags in turns:
            r = step(args.parent_exe if tag == "parent" else EXE, argv + flags, dict(env), args.limit, tmp, ns, False)
            md5 = md5 or r["md5"]
            if r["md5"] != md5:
                raise StepFailed(f"{ns} strains, {kind}, round {rnd}, {tag}: the coverage tables differ from the first run's")
            if tag == "spectrum":
                md5s = md5s or r["md5r"]
                if r["md5r"] != md5s:
                    raise StepFailed(f"{ns} strains, {kind}, round {rnd}: the {word} tables differ from the first run's")
            res[tag].append(r)
    if args.parent_exe and not thresholds:
        res["parent"] = [step(args.parent_exe, argv + ["--coverage-only"], dict(env), args.limit, tmp, ns, False) for _ in range(args.rounds)]
        if any(r["md5"] != md5 for r in res["parent"]):
            raise StepFailed(f"{ns} strains, {kind}: the parent build writes other tables")
    say(f"{ns} strains, {kind}: the {ns} coverage tables are the same bytes in all runs (MD5 {md5}), the {word} tables in all "
        f"{args.rounds} (MD5 {md5s})")
    names = {"plain": "--coverage-only", "spectrum": label, "parent": "parent build, --coverage-only"}
    for tag, rs in res.items():
        if rs:
            say(f"    {names[tag]}: pass {row(rs, 'passed', '.2f')} s; wall {row(rs, 'wall', '.2f')} s; accumulators on the device: folds "
                f"{row(rs, 'fold', '.2f')} ms, target sweeps {row(rs, 'sweep', '.3f')} ms; runs on the device {rs[0]['dev']}, replayed {rs[0]['replayed']}")
            if background and tag != "parent":
                say(f"        scan kernels on the device: {row(rs, 'scan', '.3f')} ms in {rs[0]['launches']} launches" +
                    (f"; background: {rs[0]['bgscans']} count scans, finishing sweeps of all targets {row(rs, 'bgsweep', '.3f')} ms" if tag == "spectrum" else ""))
            elif rarefaction and tag == "spectrum":
                folds = rs[0]["dev"] * ((ns + 31) // 32)
                say(f"        rarefaction on the device: classifying passes and pair counts of all folds {row(rs, 'rarcls', '.3f')} ms (a part of the folds "
                    f"above): {' '.join(format(1e3 * r['rarcls'] / folds if folds else float('nan'), '.1f') for r in rs)} us per fold over {folds} folds; "
                    f"finishing passes of all targets {row(rs, 'rarfin', '.3f')} ms")
            elif support and tag == "spectrum":
                say(f"        support on the device: takes of all folds {row(rs, 'take', '.3f')} ms (a part of the folds above), finishes of all targets "
                    f"{row(rs, 'supfin', '.3f')} ms")
            elif sweep and tag == "spectrum":
                say(f"        scrub sweep on the device: class passes of all targets {row(rs, 'cls', '.3f')} ms")
            elif thresholds and tag == "spectrum":
                say(f"        thresholds on the device: finishing passes of all targets {row(rs, 'thr', '.3f')} ms (the folds above classify as well)")
            if recurrence and tag == "spectrum":
                say(f"        recurrence on the device: marks of all targets {row(rs, 'mark', '.3f')} ms; the one finish: histogram "
                    f"{row(rs, 'hist', '.3f')} ms, pair table {row(rs, 'gram', '.3f')} ms")
    keys = ("passed", "wall", "fold", "sweep")
    med = {t: {k: statistics.median(r[k] for r in rs) for k in keys} for t, rs in res.items() if rs}
    say(f"    with the {word} / without at the medians: pass %.2f, wall %.2f, folds %.2f, target sweeps %.2f" %
        tuple(med["spectrum"][k] / med["plain"][k] if med["plain"][k] else float("nan") for k in keys))
    if background:
        ms = {t: statistics.median(r["scan"] for r in res[t]) for t in ("plain", "spectrum")}
        extra = res["spectrum"][0]["launches"] - res["plain"][0]["launches"]
        say(f"    the count scans add {ms['spectrum'] - ms['plain']:.3f} ms of scan kernel time at the medians ({ms['plain']:.3f} -> {ms['spectrum']:.3f} ms) in "
            f"{extra} launches: {1e3 * (ms['spectrum'] - ms['plain']) / extra if extra else float('nan'):.1f} us per count scan")
    if res["parent"]:                                        # the yardstick: the parent's medians; the margin: its own spread
        for k, unit in (("passed", "s"), ("fold", "ms"), ("sweep", "ms")) if thresholds else (("passed", "s"), ("sweep", "ms")):
            spread = max(r[k] for r in res["parent"]) - min(r[k] for r in res["parent"])
            for tag in ("plain", "spectrum"):
                diff = med[tag][k] - med["parent"][k]
                say(f"    {k}: {names[tag]} median {med[tag][k]:.3f} {unit} against the parent's {med['parent'][k]:.3f} {unit} "
                    f"({diff:+.3f}; the parent's spread over {args.rounds} rounds is {spread:.3f}): {'within' if diff <= spread else 'BEYOND'} it, "
                    f"ratio {med[tag][k] / med['parent'][k] if med['parent'][k] else float('nan'):.3f}")


def timed(argv, env, limit, cwd, stdout=None):
    """one run of a program under its own time limit -> wall seconds; raises StepFailed"""
    t0 = time.perf_counter()
    p = subprocess.run(["timeout", "-k", "10", str(limit)] + argv, env=env, cwd=cwd, stdout=stdout or subprocess.DEVNULL, stderr=subprocess.PIPE)
    if p.returncode != 0:
        raise StepFailed(f"{' '.join(argv[:3])} ...: exit status {p.returncode}: {p.stderr.decode(errors='replace')[-800:]}")
    return time.perf_counter() - t0


def sweep_steps(say, args, env, tmp, target_list, nfiles):
    """step 2 alone at 8 fractions against 1, and one fused run at 8 fractions against 8 fused runs of one"""
    count = os.path.join(REPO, "strainer2_amd", "bin", "kmer_scrub_count")
    filt = os.path.join(REPO, "strainer2_amd", "bin", "kmer_scrub_filter")
    fr = SWEEP_LIST.split(",")
    if not os.path.exists(os.path.join(tmp, "s15.fa")):
        raise StepFailed("the fused measurement scrubs strains 0..7 against strains 8..15: --strains needs a count of 16 or more")
    with open(os.path.join(tmp, "A.txt"), "w") as f:
        f.write("".join(f"s{s}.fa\n" for s in range(8, 16)))
    with open(os.path.join(tmp, "Bs.txt"), "w") as f:
        f.write("".join(f"r{i}.fq\n" for i in range(min(nfiles, 4))))
    with open(os.path.join(tmp, "table.txt"), "wb") as f:
        timed([count, "-r", "s0.fa", "-A", "A.txt", "-B", "Bs.txt"], env, args.limit, tmp, stdout=f)
    one = [timed([filt, "-s", "table.txt", "-m", fr[0]], env, args.limit, tmp) for _ in range(args.rounds)]
    many = [timed([filt, "-s", "table.txt", "--min_fraction_list", SWEEP_LIST, "--classes_out", "table.classes"], env, args.limit, tmp) for _ in range(args.rounds)]
    say(f"step 2 alone, kmer_scrub_filter over one strain's count table ({os.path.getsize(os.path.join(tmp, 'table.txt')) >> 20} MiB of text): wall "
        f"{' '.join(format(x, '.2f') for x in one)} s at F = 1 (-m {fr[0]}), {' '.join(format(x, '.2f') for x in many)} s at F = 8 "
        f"({SWEEP_LIST}); medians {statistics.median(one):.2f} and {statistics.median(many):.2f} s")
    with open(os.path.join(tmp, "Sf.txt"), "w") as f:
        f.write("".join(f"s{s}.fa\tf{s}.inf\tfo{s}.gz\n" for s in range(8)))
    front = [count, "-S", "Sf.txt", "-A", "A.txt", "-B", "Bs.txt"]
    back = ["--detect", "-B", target_list, "--coverage-only"]
    w8 = timed(front + ["--scrub", SWEEP_LIST] + back + ["--coverage-scrub-sweep"], env, args.limit, tmp)
    sweep = {}
    for s in range(8):
        with open(os.path.join(tmp, f"fo{s}.gz.coverage_scrub_sweep"), "rb") as f:
            for ln in f.read().split(b"\n")[1:]:
                if ln:
                    c = ln.split(b"\t")
                    sweep[(s, c[1], c[2].decode())] = (int(c[3]), int(c[4]), int(c[5]))
    w1, wrong, rows = [], 0, 0
    for q in fr:
        w1.append(timed(front + ["--scrub", q] + back, env, args.limit, tmp))
        for s in range(8):
            with open(os.path.join(tmp, f"fo{s}.gz.coverage_depth"), "rb") as f:
                for ln in f.read().split(b"\n")[1:]:
                    if ln:
                        c = ln.split(b"\t")
                        rows += 1
                        wrong += sweep.get((s, c[5], q)) != (int(c[4]), max(int(c[8]), 0), int(c[9]))
    if wrong or rows != len(sweep):
        raise StepFailed(f"fused: {wrong} of {rows} coverage-table rows of the 8 single-fraction runs differ from the sweep table ({len(sweep)} rows)")
    say(f"fused, 8 strains, kmer_scrub_count -S --scrub .. --detect -B {target_list} --coverage-only: one run at 8 fractions with "
        f"--coverage-scrub-sweep, wall {w8:.2f} s; 8 runs at one fraction each, wall {' '.join(format(x, '.2f') for x in w1)} s, together "
        f"{sum(w1):.2f} s: {sum(w1) / w8:.2f} x; all {rows} coverage-table rows of the 8 runs carry the sweep table's numbers")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gbases", type=float, default=1.5, help="bases per list")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--strains", default="8,32")
    ap.add_argument("--limit", type=int, default=150, help="seconds one run of the program may take")
    ap.add_argument("--parent-exe", default=None, help="strain_detect of a build of the parent commit")
    ap.add_argument("--regions", type=int, default=None, help="measure --coverage-regions with this --region-window")
    ap.add_argument("--spectrum", type=int, default=None, help="measure --coverage-spectrum with this --spectrum-max")
    ap.add_argument("--recurrence", action="store_true", help="measure --coverage-recurrence --recurrence-pairs")
    ap.add_argument("--thresholds", action="store_true", help="measure --coverage-thresholds, the parent build's runs in turn with this build's")
    ap.add_argument("--threshold-list", default=None, help="... with this --threshold-list (default: the program's)")
    ap.add_argument("--scrub-sweep", action="store_true", help="measure --coverage-scrub-sweep, step 2 at 8 fractions and the fused form")
    ap.add_argument("--support", action="store_true", help="measure --coverage-support, the parent build's runs in turn with this build's")
    ap.add_argument("--background", action="store_true", help="measure --coverage-background --background-spectrum, the parent build's runs in turn with this build's")
    ap.add_argument("--rarefaction", action="store_true", help="measure --coverage-rarefaction, the parent build's runs in turn with this build's")
    ap.add_argument("--kinds", default="plain,gz", help="the targets' kinds to measure: plain, gz or both")
    ap.add_argument("--pairs", action="store_true", help="... with --support-pairs=FILE as well")
    ap.add_argument("--stderr-dir", default=None, help="keep every run's stderr (the SK_SD_TIMING lines) in this directory")
    ap.add_argument("--out", default=None)
    ap.add_argument("--tmp", default="/dev/shm" if os.path.isdir("/dev/shm") else None)
    args = ap.parse_args()
    if args.stderr_dir:
        global STDERR_DIR
        STDERR_DIR = os.path.abspath(args.stderr_dir)
        os.makedirs(STDERR_DIR, exist_ok=True)
    if args.parent_exe:
        args.parent_exe = os.path.abspath(args.parent_exe)     # (the runs' working directory is the data's)
    counts = [int(x) for x in args.strains.split(",")]
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    env = {k: v for k, v in os.environ.items() if not k.startswith("SK_") or k in ("SK_THREADS", "SK_DEVICE")}
    env["SK_SD_TIMING"] = "1"
    env["SK_SD_RESULT_BYTES"] = "1"
    ok = True
    with tempfile.TemporaryDirectory(dir=args.tmp) as tmp:
        rng = np.random.default_rng(11)
        genome = []
        for s in range(max(counts)):
            cfg5.write_strain(tmp, s)
            genome.append(cfg5.strain(s))
            if args.scrub_sweep:                                 # a class file of 8 fractions for the strain's list: line i has class i % 8 + 1
                with open(os.path.join(tmp, f"s{s}.inf"), "rb") as f:
                    kms = [ln for ln in f.read().split(b"\n") if ln and not ln.startswith(b"#")]
                with open(os.path.join(tmp, f"s{s}.inf.classes"), "wb") as f:
                    f.write(b"#min_fractions\t" + SWEEP_LIST.encode() + b"\n#post_scrub_kmers\t" +
                            ",".join(str(sum(1 for i in range(len(kms)) if i % 8 + 1 >= q + 1)) for q in range(8)).encode() + b"\n" +
                            b"".join(b"%s\t%d\n" % (k, i % 8 + 1) for i, k in enumerate(kms)))
        for ns in counts:
            with open(os.path.join(tmp, f"S{ns}.txt"), "w") as f:
                f.write("".join(f"s{s}.fa\ts{s}.inf\tout{s}.gz\n" for s in range(ns)))
        per = 500_000                                            # reads per file (0.075 Gbase); one text, one deflate, many names
        text = bytearray(reads_text(rng, per, True))
        seq = np.frombuffer(text, dtype=np.uint8).reshape(per, -1)
        for i in range(0, per, 50):                              # (2 % of the reads are a strain's, as in cfg5)
            g = genome[int(rng.integers(0, min(counts)))]
            a = int(rng.integers(0, g.size - 150))
            seq[i, 16:166] = g[a:a + 150]
        text = bytes(text)
        nfiles = max(int(args.gbases * 1e9 / (per * 150)), 2)
        co = zlib.compressobj(6, zlib.DEFLATED, 31)
        gz = co.compress(text) + co.flush()
        lists = {}
        for kind, blob, ext in (("plain FASTQ", text, ".fq"), ("FASTQ .gz", gz, ".fq.gz")):
            for i in range(nfiles):
                with open(os.path.join(tmp, f"r{i}{ext}"), "wb") as f:
                    f.write(blob)
            lst = "B" + ext + ".txt"
            with open(os.path.join(tmp, lst), "w") as f:
                f.write("".join(f"SE\tr{i}{ext}\n" for i in range(nfiles)))
            lists[kind] = lst
        gbase = nfiles * per * 150 / 1e9
        say(f"strain_detect -S <cfg5 strains of {cfg5.STRAIN_BP} bp> -B <list>, {nfiles} files of {per} 150-base FASTQ reads per list "
            f"({gbase:.2f} Gbase), in {tmp}; {os.cpu_count()} CPUs seen, SK_THREADS={env.get('SK_THREADS', 'default')}; "
            f"the flags alternate, {args.rounds} rounds")
        try:
            for ns in counts:
                for kind, lst in lists.items():
                    if ("gz" if kind.endswith(".gz") else "plain") not in args.kinds.split(","):
                        continue
                    argv = ["-S", f"S{ns}.txt", "-B", lst]
                    if args.spectrum is not None or args.recurrence or args.thresholds or args.scrub_sweep or args.support or args.background or args.rarefaction:
                        spectrum_case(say, args, env, tmp, ns, kind, argv, args.recurrence, args.thresholds, args.scrub_sweep, args.support, args.background,
                                      args.rarefaction)
                        continue
                    if args.regions is not None:
                        regions_case(say, args, env, tmp, ns, kind, argv)
                        continue
                    res = {"--coverage-depth": [], "--coverage-only": []}
                    md5 = None
                    for rnd in range(args.rounds):
                        for flag in res:
                            r = step(EXE, argv + [flag], dict(env), args.limit, tmp, ns, flag == "--coverage-depth")
                            md5 = md5 or r["md5"]
                            if r["md5"] != md5:
                                raise StepFailed(f"{ns} strains, {kind}, round {rnd}, {flag}: the tables differ from the first run's")
                            res[flag].append(r)
                    say(f"{ns} strains, {kind}: the {ns} tables are the same bytes in all {2 * args.rounds} runs (MD5 {md5})")
                    for flag, rs in res.items():
                        say(f"    {flag:16s} pass {row(rs, 'passed', '.2f')} s; wall {row(rs, 'wall', '.2f')} s; CPU-seconds {row(rs, 'cpu', '.1f')}; "
                            f"results copied from the device {rs[0]['d2h']} bytes; runs on the device {rs[0]['dev']}, replayed {rs[0]['replayed']}")
                    med = {f: {k: statistics.median(r[k] for r in rs) for k in ("passed", "wall", "cpu")} for f, rs in res.items()}
                    say("    --coverage-only / --coverage-depth at the medians: pass %.2f, wall %.2f, CPU-seconds %.2f, bytes from the device %.4f" %
                        tuple([med["--coverage-only"][k] / med["--coverage-depth"][k] for k in ("passed", "wall", "cpu")] +
                              [res["--coverage-only"][0]["d2h"] / max(res["--coverage-depth"][0]["d2h"], 1)]))
                    if args.parent_exe:
                        rs = [step(args.parent_exe, argv + ["--coverage-depth"], dict(env), args.limit, tmp, ns, True) for _ in range(3)]
                        if any(r["md5"] != md5 for r in rs):
                            raise StepFailed(f"{ns} strains, {kind}: the parent build writes other tables")
                        say(f"    parent build, --coverage-depth x3: pass {row(rs, 'passed', '.2f')} s; wall {row(rs, 'wall', '.2f')} s; "
                            f"CPU-seconds {row(rs, 'cpu', '.1f')} (same tables)")
            if args.scrub_sweep:
                sweep_steps(say, args, env, tmp, lists["plain FASTQ"], nfiles)
        except StepFailed as x:
            ok = False
            say(f"STOPPED: {x}")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
