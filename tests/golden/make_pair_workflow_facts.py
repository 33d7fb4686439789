#!/usr/bin/env python3
"""tests/golden/make_pair_workflow_facts.py -- pin what the UNMODIFIED reference's workflow (steps 1-4) gives the two bundled
strains.

`kmer_scrub_count -S <strains> ... --scrub 0.01 [--independent] --detect -B target_metagenomes.txt` runs steps 1 to 4 for many
strains in one job; every strain's informative list, hit list and coverage table must be the ones the reference's chain of
programs and scripts makes for that strain alone (test/example.sh):

  1. oracle/_ref/kmer_scrub_count -r <strain> -A genomes_to_scrub.txt -B metagenomes_to_scrub.txt [-C drug_pair.txt]
  2. scripts/kmer_scrub_filter.py -s <table.gz> -m 0.01 [-i]
  3. oracle/_ref/strain_detect -r <strain> -a <informative.gz> -B target_metagenomes.txt -o <hits.gz>
  4. scripts/coverage_depth.py -k <hits.gz>

run in tests/golden/bundled for B8 and D4, without and with the -C list of make_step1_pair_facts.py (both strains, B8 twice),
and once more with -i (B8, D4, no -C).  Recorded per strain and case: the md5 of the informative list, of the hit list
(decompressed) and of the coverage table.  Only data is committed (tests/golden/pair_workflow_facts.json); build container
only (it needs the reference's scripts and `make -C oracle`).

  make -C oracle && python3 tests/golden/make_pair_workflow_facts.py
"""
import gzip
import hashlib
import json
import os
import shutil
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
KSC = os.path.join(REPO, "oracle", "_ref", "kmer_scrub_count")
SD = os.path.join(REPO, "oracle", "_ref", "strain_detect")
FILTER_REF = "/root/reference/scripts/kmer_scrub_filter.py"
COV_REF = "/root/reference/scripts/coverage_depth.py"
BUNDLED = os.path.join(REPO, "tests", "golden", "bundled")
STRAINS = {
    "B8": "strains/Bacteroides_ovatus_1001283st1_B8_1001283B150210_160208.fna.gz",
    "D4": "strains/Bacteroides_ovatus_1001302st1_D4_1001302B_160321.fna.gz",
}
C_LINES = [STRAINS["B8"], STRAINS["D4"], STRAINS["B8"]]
C_NAME = "drug_pair.txt"          # written next to the bundled lists by the tests too (relative paths, cwd = bundled)
FRACTION = "0.01"
CASES = {"plain": ([], []), "drug": (["-C", C_NAME], []), "independent": ([], ["-i"])}


def md5(data):
    return hashlib.md5(data).hexdigest()


def check(p, what):
    if p.returncode != 0:
        sys.exit(f"{what} failed ({p.returncode}): {p.stderr.decode()[-2000:]}")


def chain(d, genome, list_args, filter_args):
    """one strain's chain in its case's directory d; the files are named after the genome, as test/example.sh names them
    (the coverage table's strain_name column is the hit list's name)"""
    name = os.path.basename(genome)[: -len(".fna.gz")]
    table = os.path.join(d, name + ".scrub_kmer_counts.gz")
    inform = os.path.join(d, name + ".scrubbed_kmers.gz")
    hits = os.path.join(d, name + ".kmer_hits.gz")
    p = subprocess.run([KSC, "-r", genome, "-A", "genomes_to_scrub.txt", "-B", "metagenomes_to_scrub.txt"] + list_args,
                       cwd=BUNDLED, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    check(p, "step 1 " + name)
    with gzip.open(table, "wb", compresslevel=1) as f:
        f.write(p.stdout)
    p = subprocess.run([sys.executable, FILTER_REF, "-s", table, "-m", FRACTION] + filter_args, cwd=BUNDLED, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE)
    check(p, "step 2 " + name)
    informative = p.stdout
    with gzip.open(inform, "wb") as f:
        f.write(informative)
    p = subprocess.run([SD, "-r", genome, "-a", inform, "-B", "target_metagenomes.txt", "-o", hits], cwd=BUNDLED, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE)
    check(p, "step 3 " + name)
    sd_out = p.stdout.decode() + p.stderr.decode()
    with gzip.open(hits, "rb") as f:
        hit_bytes = f.read()
    p = subprocess.run([sys.executable, COV_REF, "-k", hits], cwd=BUNDLED, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    check(p, "step 4 " + name)
    return {"informative_md5": md5(informative), "informative_lines": informative.count(b"\n"),
            "hits_md5": md5(hit_bytes), "hits_lines": hit_bytes.count(b"\n"),
            "coverage_md5": md5(p.stdout), "coverage_lines": p.stdout.count(b"\n"), "strain_detect_said": sd_out}


def main():
    facts = {"c_list": C_LINES, "c_name": C_NAME, "strains": STRAINS, "min_fraction": FRACTION,
             "detect_args": ["-B", "target_metagenomes.txt"], "cases": {}}
    cpath = os.path.join(BUNDLED, C_NAME)
    with open(cpath, "w") as f:
        f.write("".join(l + "\n" for l in C_LINES))
    d = tempfile.mkdtemp()
    try:
        for case, (list_args, filter_args) in CASES.items():
            facts["cases"][case] = {"kmer_scrub_count": list_args, "kmer_scrub_filter": filter_args, "strains": {}}
            os.mkdir(os.path.join(d, case))
            for name, genome in STRAINS.items():
                facts["cases"][case]["strains"][name] = chain(os.path.join(d, case), genome, list_args, filter_args)
    finally:
        os.unlink(cpath)
        shutil.rmtree(d)
    with open(os.path.join(REPO, "tests", "golden", "pair_workflow_facts.json"), "w") as f:
        json.dump(facts, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
