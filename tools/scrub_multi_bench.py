#!/usr/bin/env python3
"""kmer_scrub_count -S on one MI355X: what one pass over the lists costs when many strains share a union table.

  (a) the union COUNT kernel: ms per resident batch of READS x 150 bp reads (1.5 Gbase by default) at 1, 8 and 32 cfg5-style
      strains (strainer2_amd/cfg5.py: i.i.d. 5 Mbp genomes; 2 % of the reads cut from them), from the HIP events around the
      scan launches (sk_union_scan_timing), and that time as a fraction of the HBM roofline on the compulsory bytes (the
      batch read once);
  (b) sk_union_counts_fold: wall ms of one fold into every member (synchronous call);
  (c) end to end: `kmer_scrub_count -S` with E2E_STRAINS strains over a plain FASTQ -B list of the same reads, against the
      sum of the E2E_STRAINS single-strain runs, outputs compared byte for byte (md5).

Prints one JSON line.  Environment: READS (10,000,000), E2E_STRAINS (8), WORK (/tmp/sk_scrub_multi_bench)."""
import hashlib
import json
import os
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
    main()
