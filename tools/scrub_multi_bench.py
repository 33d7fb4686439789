#!/usr/bin/env python3
"""kmer_scrub_count -S on one MI355X: what one pass over the lists costs when many strains share a union table.

  (a) the union COUNT kernel: ms per resident batch of READS x 150 bp reads (1.5 Gbase by default) at 1, 8 and 32 cfg5-style
      strains (strainer2_amd/cfg5.py: i.i.d. 5 Mbp genomes; 2 % of the reads cut from them), from the HIP events around the
      scan launches (sk_union_scan_timing), and that time as a fraction of the HBM roofline on the compulsory bytes (the
      batch read once);
  (b) sk_union_counts_fold: wall ms of one fold into every member (synchronous call);
  (c) end to end: `kmer_scrub_count -S` with E2E_STRAINS strains over a plain FASTQ -B list of the same reads, against the
      sum of the E2E_STRAINS single-strain runs, outputs compared byte for byte (md5).

  (d) with --workflow, instead of (a)-(c): steps 1 to 3 for WORKFLOW_STRAINS cfg5 strains (8; "8,32" for both sizes) over a
      plain FASTQ -B list, fused -- `kmer_scrub_count -S .. --scrub 0.01 --detect -B <targets>` -- against the chain of
      three programs: `kmer_scrub_count -S` (gz count tables), `kmer_scrub_filter -l` once per strain, `strain_detect -S`.
      Every informative list and hit list (decompressed) is compared by md5 in the same run.  Each program runs under its own
      `timeout -k 10`; the first failure ends the run.

  (e) with --onepass, instead: `kmer_scrub_count -S` for G x 32 cfg5 strains (ONEPASS_G, "2,8": 64 and 256 strains) over a -B
      list of one plain FASTQ of ONEPASS_READS reads, then over its .gz copy, with the default (every union that fits fed by
      one decode of the lists) and with SK_SCRUB_UNIONS=1 (one decode per union, as before).  Every outfile is compared by md5
      in the same run; reported: wall time, the list phase from SK_TIMING, decodes, unions per decode.  Each run under its
      own `timeout -k 10`; the first failure ends the tool.

Prints one JSON line.  Environment: READS (10,000,000), E2E_STRAINS (8), WORK (/tmp/sk_scrub_multi_bench), for (d)
WORKFLOW_STRAINS (8), TARGET_READS (2,000,000: the -B list of strain_detect, one plain FASTQ), for (e) ONEPASS_G ("2,8"),
ONEPASS_READS (4,000,000)."""
import hashlib
import json
import os
import re
import shutil
import subprocess
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import strainer2_amd as sk  # noqa: E402
from strainer2_amd import cfg5, synth  # noqa: E402
from strainer2_amd.native import lib  # noqa: E402

READS = int(os.environ.get("READS", "10000000"))
E2E = int(os.environ.get("E2E_STRAINS", "8"))
WORK = os.environ.get("WORK", "/tmp/sk_scrub_multi_bench")
HBM_TBS = 8.0                                  # MI355X peak HBM3E bandwidth, TB/s
REPS = 3


def md5(path):
    h = hashlib.md5()
    with open(path, "rb") as f:
        for blk in iter(lambda: f.read(1 << 24), b""):
            h.update(blk)
    return h.hexdigest()


def write_fastq(path, reads):
    """a record stream of 150 bp reads (151 bytes per record) as a plain FASTQ file"""
    r2 = reads.reshape(-1, 151)[:, :150]
    with open(path, "wb") as f:
        for a in range(0, r2.shape[0], 500_000):
            blk = r2[a:a + 500_000]
            rec = np.empty((blk.shape[0], 4 + 151 + 2 + 151), dtype=np.uint8)
            rec[:, 0:4] = np.frombuffer(b"@rd\n", dtype=np.uint8)
            rec[:, 4:154] = blk
            rec[:, 154] = 10
            rec[:, 155:157] = np.frombuffer(b"+\n", dtype=np.uint8)
            rec[:, 157:307] = ord("I")
            rec[:, 307] = 10
            f.write(rec.tobytes())


def md5_any(path):
    """md5 of the decompressed bytes (gzip by its magic)"""
    import gzip
    with open(path, "rb") as f:
        gz = f.read(2) == b"\x1f\x8b"
    h = hashlib.md5()
    with (gzip.open if gz else open)(path, "rb") as f:
        for blk in iter(lambda: f.read(1 << 24), b""):
            h.update(blk)
    return h.hexdigest()


def timed(argv, limit_s, what, **kw):
    """one program under its own time limit; a failure ends the bench (nothing more is started)"""
    t = time.time()
    kw.setdefault("stdout", subprocess.PIPE)
    p = subprocess.run(["timeout", "-k", "10", str(limit_s)] + argv, stderr=subprocess.PIPE, text=True, **kw)
    if p.returncode != 0:
        sys.stderr.write(f"{what} failed with status {p.returncode}:\n{p.stderr[-3000:]}\n")
        sys.exit(1)
    return time.time() - t, p


def workflow():
    """(d): the fused job against the chain of three programs, outputs compared"""
    os.makedirs(WORK, exist_ok=True)
    sizes = [int(x) for x in os.environ.get("WORKFLOW_STRAINS", "8").split(",")]
    target_reads = int(os.environ.get("TARGET_READS", "2000000"))
    res = {"reads": READS, "target_reads": target_reads, "read_len": 150, "min_fraction": "0.01", "runs": []}
    t0 = time.time()
    genomes = [cfg5.strain(s) for s in range(max(sizes))]
    reads, bases = synth.make_reads(genomes, READS)
    fq = os.path.join(WORK, "reads.fq")
    write_fastq(fq, reads)
    del reads
    treads, tbases = synth.make_reads(genomes, target_reads, seed=synth.SEED + 7)
    tq = os.path.join(WORK, "targets.fq")
    write_fastq(tq, treads)
    del treads
    paths = []
    for s in range(max(sizes)):
        p = os.path.join(WORK, f"s{s}.fa")
        with open(p, "wb") as f:
            f.write(b">s%d\n" % s + genomes[s].tobytes() + b"\n")
        paths.append(p)
    res["setup_s"] = round(time.time() - t0, 1)
    res["list_gbase"] = round(bases / 1e9, 3)
    res["target_gbase"] = round(tbases / 1e9, 3)
    with open(os.path.join(WORK, "A.txt"), "w") as f:
        f.write(paths[-1] + "\n")
    with open(os.path.join(WORK, "B.txt"), "w") as f:
        f.write(fq + "\n")
    with open(os.path.join(WORK, "T.txt"), "w") as f:
        f.write(f"SE\t{tq}\n")
    exe, flt, sd = sk.cli_path(), sk.cli_path("kmer_scrub_filter"), sk.cli_path("strain_detect")
    lists = ["-A", os.path.join(WORK, "A.txt"), "-B", os.path.join(WORK, "B.txt")]
    env = dict(os.environ, SK_TIMING="1")
    for n in sizes:
        w = os.path.join(WORK, f"n{n}")
        os.makedirs(w, exist_ok=True)
        fused_s, chain_s = os.path.join(w, "fused.txt"), os.path.join(w, "chain.txt")
        with open(fused_s, "w") as f:
            for s in range(n):
                f.write(f"{paths[s]}\t{w}/fused{s}.inf\t{w}/fused{s}.kmer_hits.gz\n")
        with open(chain_s, "w") as f:
            for s in range(n):
                f.write(f"{paths[s]}\t{w}/counts{s}.tsv.gz\n")
        run = {"strains": n}
        # the fused job: steps 1-3 in one process, the tables of step 1 resident to the end
        run["fused_s"], p = timed([exe, "-S", fused_s] + lists + ["--scrub", "0.01", "--detect", "-B", os.path.join(WORK, "T.txt")],
                                  900, "fused -S", env=env)
        run["fused_timing"] = [l for l in p.stderr.splitlines() if "timing" in l]
        # the chain: -S count tables (gz), the filter per strain, strain_detect -S
        run["chain_count_s"], p = timed([exe, "-S", chain_s] + lists, 900, "-S count tables", env=env)
        run["count_tables_gz_bytes"] = sum(os.path.getsize(f"{w}/counts{s}.tsv.gz") for s in range(n))
        run["chain_filter_s"] = 0.0
        for s in range(n):
            with open(f"{w}/list{s}.txt", "w") as f:
                f.write(f"{w}/counts{s}.tsv.gz\n")
            with open(f"{w}/chain{s}.inf", "w") as out:
                dt, _ = timed([flt, "-l", f"{w}/list{s}.txt", "-m", "0.01"], 600, f"kmer_scrub_filter strain {s}", stdout=out)
            run["chain_filter_s"] += dt
        with open(os.path.join(w, "sd.txt"), "w") as f:
            for s in range(n):
                f.write(f"{paths[s]}\t{w}/chain{s}.inf\t{w}/chain{s}.kmer_hits.gz\n")
        run["chain_detect_s"], _ = timed([sd, "-S", os.path.join(w, "sd.txt"), "-B", os.path.join(WORK, "T.txt")], 900, "strain_detect -S")
        run["chain_s"] = round(run["chain_count_s"] + run["chain_filter_s"] + run["chain_detect_s"], 2)
        for k in ("fused_s", "chain_count_s", "chain_filter_s", "chain_detect_s"):
            run[k] = round(run[k], 2)
        run["speedup"] = round(run["chain_s"] / run["fused_s"], 2)
        same_inf = all(md5_any(f"{w}/fused{s}.inf") == md5_any(f"{w}/chain{s}.inf") for s in range(n))
        same_hits = all(md5_any(f"{w}/fused{s}.kmer_hits.gz") == md5_any(f"{w}/chain{s}.kmer_hits.gz") for s in range(n))
        run["informative_identical"], run["hits_identical"] = same_inf, same_hits
        run["informative_kmers"] = sum(sum(1 for _ in open(f"{w}/fused{s}.inf")) for s in range(n))
        res["runs"].append(run)
        shutil.rmtree(w)
    os.unlink(fq)
    os.unlink(tq)
    print(json.dumps(res))


def onepass():
    """(e): G unions fed by one decode against one decode per union, plain and .gz -B list, outputs compared"""
    os.makedirs(WORK, exist_ok=True)
    gs = [int(x) for x in os.environ.get("ONEPASS_G", "2,8").split(",")]
    nreads = int(os.environ.get("ONEPASS_READS", "4000000"))
    res = {"reads": nreads, "read_len": 150, "runs": []}
    t0 = time.time()
    genomes = [cfg5.strain(s) for s in range(32 * max(gs))]
    reads, bases = synth.make_reads(genomes[:32], nreads)
    fq = os.path.join(WORK, "reads.fq")
    write_fastq(fq, reads)
    del reads
    timed(["sh", "-c", f"gzip -1 -c {fq} > {fq}.gz"], 600, "gzip of the -B file")
    paths = []
    for s in range(len(genomes)):
        p = os.path.join(WORK, f"s{s}.fa")
        with open(p, "wb") as f:
            f.write(b">s%d\n" % s + genomes[s].tobytes() + b"\n")
        paths.append(p)
    del genomes
    res["setup_s"] = round(time.time() - t0, 1)
    res["list_gbase"] = round(bases / 1e9, 3)
    res["fastq_bytes"], res["fastq_gz_bytes"] = os.path.getsize(fq), os.path.getsize(fq + ".gz")
    with open(os.path.join(WORK, "A.txt"), "w") as f:
        f.write(paths[-1] + "\n")
    exe = sk.cli_path()
    pat = re.compile(r"(\d+) union pass\(es\) \+ (\d+) single pass\(es\) ([0-9.]+) s .*lists decoded (\d+) time\(s\) \((\d+) bases\)")
    for g in gs:
        n = 32 * g
        w = os.path.join(WORK, f"g{g}")
        os.makedirs(w, exist_ok=True)
        with open(os.path.join(w, "S.txt"), "w") as f:
            for s in range(n):
                f.write(f"{paths[s]}\t{w}/o{s}.tsv\n")
        for form, path in (("plain", fq), ("gz", fq + ".gz")):
            with open(os.path.join(w, "B.txt"), "w") as f:
                f.write(path + "\n")
            run = {"strains": n, "list": form}
            sums = {}
            for mode, extra in (("onepass", {}), ("per_union", {"SK_SCRUB_UNIONS": "1"})):
                env = dict(os.environ, SK_TIMING="1", **extra)
                wall, p = timed([exe, "-S", os.path.join(w, "S.txt"), "-A", os.path.join(WORK, "A.txt"), "-B", os.path.join(w, "B.txt")],
                                1800, f"-S {n} strains ({form}, {mode})", env=env)
                m = pat.search(p.stderr)
                if not m:
                    sys.stderr.write(f"no SK_TIMING line in:\n{p.stderr[-3000:]}\n")
                    sys.exit(1)
                unions, singles, list_s, decodes, dbases = int(m[1]), int(m[2]), float(m[3]), int(m[4]), int(m[5])
                run[mode] = {"wall_s": round(wall, 2), "list_phase_s": list_s, "unions": unions, "single_passes": singles,
                             "decodes": decodes, "unions_per_decode": round(unions / max(decodes - singles, 1), 2),
                             "bases_decoded": dbases}
                with ThreadPoolExecutor(16) as ex:
                    sums[mode] = list(ex.map(md5, [f"{w}/o{s}.tsv" for s in range(n)]))
                for s in range(n):
                    os.unlink(f"{w}/o{s}.tsv")
            run["outputs_identical"] = sums["onepass"] == sums["per_union"]
            run["list_phase_speedup"] = round(run["per_union"]["list_phase_s"] / max(run["onepass"]["list_phase_s"], 1e-9), 2)
            run["wall_speedup"] = round(run["per_union"]["wall_s"] / run["onepass"]["wall_s"], 2)
            res["runs"].append(run)
            if not run["outputs_identical"]:
                print(json.dumps(res))
                sys.stderr.write("outfiles differ between the two modes\n")
                sys.exit(1)
        shutil.rmtree(w)
    for p in paths:
        os.unlink(p)
    os.unlink(fq)
    os.unlink(fq + ".gz")
    print(json.dumps(res))


def main():
    os.makedirs(WORK, exist_ok=True)
    res = {"reads": READS, "read_len": 150}
    t0 = time.time()
    genomes = [cfg5.strain(s) for s in range(32)]
    with ThreadPoolExecutor(16) as ex:
        sets = list(ex.map(lambda g: sk.Keyset.from_stream(g.tobytes() + b"\n"), genomes))
    reads, bases = synth.make_reads([g for g in genomes], READS)
    res["setup_s"] = round(time.time() - t0, 1)
    res["batch_gbase"] = round(bases / 1e9, 3)

    # (a) + (b): resident batch, union COUNT scan, fold
    holder = sk.KmerContext(0)
    dptr = holder.dev_alloc(reads.size)
    holder.dev_upload(dptr, reads)
    res["union"] = []
    for n in (1, 8, 32):
        ctxs = [sk.KmerContext(0) for _ in range(n)]
        try:
            for c, ks in zip(ctxs, sets[:n]):
                c.load_keyset(ks, 4)
            with sk.KmerUnion(ctxs) as u:
                u.count_enable(1)
                uc = lib.sk_union_context(u._h)
                rc = lib.sk_scan_device(uc, dptr, reads.size, 0)          # warm-up (and the filters' first touch)
                assert rc == 0, rc
                u.fold_counts(0, 1)
                u.scan_timing(reset=True)
                for _ in range(REPS):
                    assert lib.sk_scan_device(uc, dptr, reads.size, 0) == 0
                ms, launches = u.scan_timing(reset=True)
                t = time.perf_counter()
                u.fold_counts(0, 1)
                fold_ms = 1e3 * (time.perf_counter() - t)
                per = ms / REPS
                hits = int(sum(int(c.counts(1).sum()) for c in ctxs))
                res["union"].append({"strains": n, "rows": u.rows, "scan_ms_per_batch": round(per, 3), "launches": launches,
                                     "gbase_per_s": round(bases / per / 1e6, 1),
                                     "hbm_roofline_frac": round(reads.size / (per * 1e-3) / (HBM_TBS * 1e12), 4),
                                     "fold_ms": round(fold_ms, 2), "member_hits": hits})
        finally:
            for c in ctxs:
                c.close()
    holder.dev_free(dptr)
    holder.close()
    for ks in sets:
        ks.close()

    # (c) end to end: -S over a plain FASTQ -B list against the single runs
    paths = []
    for s in range(E2E):
        p = os.path.join(WORK, f"s{s}.fa")
        with open(p, "wb") as f:
            f.write(b">s%d\n" % s + genomes[s].tobytes() + b"\n")
        paths.append(p)
    fq = os.path.join(WORK, "reads.fq")
    r2 = reads.reshape(-1, 151)[:, :150]
    with open(fq, "wb") as f:
        for a in range(0, r2.shape[0], 500_000):
            blk = r2[a:a + 500_000]
            rec = np.empty((blk.shape[0], 4 + 151 + 2 + 151), dtype=np.uint8)
            rec[:, 0:4] = np.frombuffer(b"@rd\n", dtype=np.uint8)
            rec[:, 4:154] = blk
            rec[:, 154] = 10
            rec[:, 155:157] = np.frombuffer(b"+\n", dtype=np.uint8)
            rec[:, 157:307] = ord("I")
            rec[:, 307] = 10
            f.write(rec.tobytes())
    with open(os.path.join(WORK, "A.txt"), "w") as f:
        f.write(os.path.join(WORK, f"s{E2E - 1}.fa") + "\n")
    with open(os.path.join(WORK, "B.txt"), "w") as f:
        f.write(fq + "\n")
    with open(os.path.join(WORK, "S.txt"), "w") as f:
        for s in range(E2E):
            f.write(f"{paths[s]}\t{WORK}/multi{s}.tsv\n")
    exe = sk.cli_path()
    lists = ["-A", os.path.join(WORK, "A.txt"), "-B", os.path.join(WORK, "B.txt")]
    env = dict(os.environ, SK_TIMING="1")
    t = time.time()
    p = subprocess.run([exe, "-S", os.path.join(WORK, "S.txt")] + lists, env=env, capture_output=True, text=True)
    multi_s = time.time() - t
    assert p.returncode == 0, p.stderr
    res["multi_timing"] = p.stderr.strip().splitlines()[-1] if p.stderr.strip() else ""
    single_s, same = 0.0, True
    for s in range(E2E):
        out = os.path.join(WORK, f"single{s}.tsv")
        t = time.time()
        with open(out, "wb") as f:
            q = subprocess.run([exe, "-r", paths[s]] + lists, stdout=f, stderr=subprocess.PIPE)
        single_s += time.time() - t
        assert q.returncode == 0, q.stderr
        same = same and md5(out) == md5(os.path.join(WORK, f"multi{s}.tsv"))
        os.unlink(out)
    res["e2e"] = {"strains": E2E, "fastq_bytes": os.path.getsize(fq), "multi_s": round(multi_s, 2),
                  "sum_single_s": round(single_s, 2), "speedup": round(single_s / multi_s, 2), "outputs_identical": same}
    for s in range(E2E):
        os.unlink(os.path.join(WORK, f"multi{s}.tsv"))
    os.unlink(fq)
    print(json.dumps(res))


if __name__ == "__main__":
    if "--workflow" in sys.argv[1:]:
        workflow()
    elif "--onepass" in sys.argv[1:]:
        onepass()
    else:
        main()
