#!/usr/bin/env python3
"""tests/golden/make_fuzz_facts.py -- pin what the reference prints for the random inputs of two oracle tests.

  oracle_fuzz   tests/test_oracle_golden.py::test_oracle_equals_live_reference_on_fuzz: a kmer_scrub_count job over random
                FASTA/FASTQ soup (_synth.oracle_fuzz_world, seeds 1-3) -- status, md5 and length of stdout, the whole stderr
  reader_soup   tests/test_host_layer.py::test_reader_grammar_soup_vs_oracle: a job whose -A and -B lists name one reader soup
                (_synth.reader_soup + _synth.soup_job, seeds 0-59) -- status, md5 and line count of stdout

The inputs are written by the tests' own generators; the UNMODIFIED reference program (oracle/_ref/kmer_scrub_count, built by
oracle/Makefile where the reference sources exist) is run on them.  Only data is committed (tests/golden/fuzz_facts.json), so the
tests hold the oracle to the reference where the reference cannot be built.

  python3 tests/golden/make_fuzz_facts.py
"""
import hashlib
import json
import os
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(REPO, "tests"))
import _synth  # noqa: E402

EXE = os.path.join(REPO, "oracle", "_ref", "kmer_scrub_count")
OUT = os.path.join(REPO, "tests", "golden", "fuzz_facts.json")


def main():
    if not os.access(EXE, os.X_OK):
        sys.exit("build the reference first: make -C oracle ref")
    facts = {"producer": "oracle/_ref/kmer_scrub_count (the unmodified reference), tests/golden/make_fuzz_facts.py",
             "oracle_fuzz": {}, "reader_soup": {}}
    for seed in (1, 2, 3):
        with tempfile.TemporaryDirectory() as d:
            argv = _synth.oracle_fuzz_world(seed, d)
            p = subprocess.run([EXE] + argv, cwd=d, capture_output=True, timeout=60)
        facts["oracle_fuzz"][str(seed)] = {"argv": argv, "returncode": p.returncode, "stdout_md5": hashlib.md5(p.stdout).hexdigest(),
                                           "stdout_bytes": len(p.stdout), "stderr": p.stderr.decode("latin-1")}
    for seed in range(60):
        with tempfile.TemporaryDirectory() as d:
            strain, soup = _synth.reader_soup(seed, d)
            p = subprocess.run([EXE] + _synth.soup_job(strain, soup, d), capture_output=True, timeout=60)
        facts["reader_soup"][str(seed)] = {"returncode": p.returncode, "stdout_md5": hashlib.md5(p.stdout).hexdigest(),
                                           "stdout_lines": len(p.stdout.splitlines())}
    with open(OUT, "w") as f:
        json.dump(facts, f, indent=1)
        f.write("\n")
    print(f"wrote {OUT}")


if __name__ == "__main__":
    main()
