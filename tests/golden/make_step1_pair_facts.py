#!/usr/bin/env python3
"""tests/golden/make_step1_pair_facts.py -- pin what the UNMODIFIED reference's step 1 prints for the two bundled strains.

kmer_scrub_count -S (several strains over one pass of the lists) must give every strain exactly the table a run of its own would
print.  This runs the reference program (oracle/_ref/kmer_scrub_count, built by `make -C oracle`) in tests/golden/bundled once per
strain (B8, D4) with the bundled -A/-B lists, and once more per strain with a -C list that names both strains' genomes (B8's
twice): each run skips its own genome (src/genome_compare.c:115-146).  Recorded per run: argv, exit status, stdout size and md5,
stderr.  Only data is committed (tests/golden/step1_pair_facts.json); build container only.

  make -C oracle && python3 tests/golden/make_step1_pair_facts.py
"""
import hashlib
import json
import os
import subprocess
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
EXE = os.path.join(REPO, "oracle", "_ref", "kmer_scrub_count")
BUNDLED = os.path.join(REPO, "tests", "golden", "bundled")
STRAINS = {
    "B8": "strains/Bacteroides_ovatus_1001283st1_B8_1001283B150210_160208.fna.gz",
    "D4": "strains/Bacteroides_ovatus_1001302st1_D4_1001302B_160321.fna.gz",
}
# the -C list of the runs with a drug column: both strains, B8 a second time (a line may come more than once)
C_LINES = [STRAINS["B8"], STRAINS["D4"], STRAINS["B8"]]
C_NAME = "drug_pair.txt"          # written next to the bundled lists by the tests too (relative paths, cwd = bundled)


def run(argv):
    with tempfile.TemporaryFile() as out:
        p = subprocess.run([EXE] + argv, cwd=BUNDLED, stdout=out, stderr=subprocess.PIPE)
        out.seek(0)
        h, n = hashlib.md5(), 0
        for blk in iter(lambda: out.read(1 << 24), b""):
            h.update(blk)
            n += len(blk)
    return {"argv": argv, "returncode": p.returncode, "stdout_bytes": n, "stdout_md5": h.hexdigest(), "stderr": p.stderr.decode()}


def main():
    facts = {"c_list": C_LINES, "c_name": C_NAME, "strains": STRAINS, "runs": {}}
    cpath = os.path.join(BUNDLED, C_NAME)
    with open(cpath, "w") as f:
        f.write("".join(l + "\n" for l in C_LINES))
    try:
        for name, path in STRAINS.items():
            base = ["-r", path, "-A", "genomes_to_scrub.txt", "-B", "metagenomes_to_scrub.txt"]
            facts["runs"][name] = run(base)
            facts["runs"][name + "+C"] = run(base + ["-C", C_NAME])
    finally:
        os.unlink(cpath)
    with open(os.path.join(REPO, "tests", "golden", "step1_pair_facts.json"), "w") as f:
        json.dump(facts, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
