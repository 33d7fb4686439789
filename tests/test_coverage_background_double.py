"""strain_detect --coverage-background on the CPU: the host layer (sk_host_sd.c, sk_host.c, sk_host_cov.c, sk_host_background.c) over
tests/native/background_double.c -- the device double plus plain-C stand-ins for the background's entry points -- as a stand-alone
program under AddressSanitizer + UBSan.  What only this build can show: every table is loaded or built with SIX columns without the
flag and SEVEN with it (the double reports each table's ncols), in a union and member by member; and the host's part of the rule --
one count scan per chunk, PE2's unpaired tail, the sweep per target, the tables -- gives the model's numbers without a GPU."""
import os
import random
import subprocess

import pytest

import _background_model as model
import _synth

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(REPO, "tests", "native")
CSRC = os.path.join(REPO, "strainer2_amd", "csrc")
HOST = [os.path.join(CSRC, f) for f in ("sk_host.c", "sk_host_sd.c", "sk_host_cov.c")]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
NAME = "Genus_species_st%d.kmer_hits.gz"


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("bgdouble") / "background_double")
    subprocess.run(["gcc", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", os.path.join(NATIVE, "background_double.c")] + HOST +
                   ["-lz", "-lpthread", "-o", out], check=True)
    return out


class Job:
    pass


@pytest.fixture(scope="module")
def job(tmp_path_factory):
    """three strains (1 and 2 related) and two targets: SE FASTA with reads shorter than k, and PE FASTQ whose PE2 holds 40 reads
    beyond PE1's last"""
    d = tmp_path_factory.mktemp("bgjob")
    rng = random.Random(606)
    j = Job()
    j.d = d
    g = _synth.rand_dna(rng, 2500)
    j.strains = [_synth.rand_dna(rng, 600), g, _synth.mutate(rng, g, 0.01)]
    j.inf = []
    for s, t in enumerate(j.strains):
        (d / f"s{s}.fa").write_bytes(b">s%d\n%s\n" % (s, t))
        kms = sorted({model.key_of(t[i:i + 31]) for i in range(s, len(t) - 31, 29)})
        j.inf.append(set(kms))
        (d / f"s{s}.inf").write_bytes(b"\n".join(kms) + b"\n")

    def reads(n, seed):
        r = random.Random(seed)
        out = []
        for i in range(n):
            t = j.strains[r.randrange(3)]
            ln = r.choice([31, 60, 100])
            a = r.randrange(len(t) - ln)
            rd = t[a:a + ln] if r.random() < 0.7 else _synth.rand_dna(r, ln)
            out.append(_synth.revcomp(rd) if i % 2 else rd)
            if i % 17 == 0:
                out.append(rd[:20])
        return out

    j.files = {"se.fa": reads(150, 1), "pe_1.fq": reads(100, 2), "pe_2.fq": reads(100, 3) + reads(40, 4)}
    for name, recs in j.files.items():
        raw = b"".join((b"@r%d\n%s\n+\n%s\n" % (i, x, b"I" * len(x))) if name.endswith(".fq") else (b">r%d\n%s\n" % (i, x)) for i, x in enumerate(recs))
        (d / name).write_bytes(raw)
    (d / "T.txt").write_text(f"SE\t{d}/se.fa\nPE\t{d}/pe_1.fq\t{d}/pe_2.fq\n")
    j.targets = [("se.fa", ["se.fa"]), ("pe_1.fq", ["pe_1.fq", "pe_2.fq"])]
    return j


def _want(job, s, D=63):
    keys = model.strain_keys([job.strains[s]])
    inf = [k in job.inf[s] for k in keys]
    return [(first, model.block(model.row_counts(keys, [r for f in files for r in job.files[f]]), inf, D)) for first, files in job.targets]


def _run(exe, job, tag, flags, strains=(0, 1, 2), **env):
    d = job.d / tag
    d.mkdir()
    if len(strains) > 1:
        (d / "S.txt").write_text("".join(f"{job.d}/s{s}.fa\t{job.d}/s{s}.inf\t{d}/{NAME % s}\n" for s in strains))
        argv = ["-S", str(d / "S.txt")]
    else:
        s = strains[0]
        argv = ["-r", str(job.d / f"s{s}.fa"), "-a", str(job.d / f"s{s}.inf"), "-o", str(d / (NAME % s))]
    p = subprocess.run([exe] + argv + ["-B", str(job.d / "T.txt")] + flags, env=dict(ENV, DOUBLE_NCOLS_LOG=str(d / "ncols"), SK_SD_CHUNK_BYTES="3000", **env),
                       capture_output=True, timeout=300)
    assert b"runtime error" not in p.stderr and b"AddressSanitizer" not in p.stderr, p.stderr.decode()[-2000:]
    assert p.returncode == 0, p.stderr.decode()[-1000:]
    ncols = [int(x) for x in (d / "ncols").read_text().split()]
    files = {}
    for s in strains:
        b = str(d / (NAME % s))[: -len(".kmer_hits.gz")]
        files[s] = {x: (open(b + "." + x, "rb").read() if os.path.exists(b + "." + x) else None)
                    for x in ("coverage_background", "coverage_background_spectrum", "coverage_depth", "kmer_hits.gz")}
    return ncols, files, p.stdout, p.stderr


@pytest.mark.parametrize("tag,strains,env", [("union", (0, 1, 2), {}), ("members", (0, 1, 2), {"DOUBLE_NO_UNION": "1"}),
                                             ("no_union", (0, 1, 2), {"SK_SD_NO_UNION": "1"}), ("single", (1,), {})])
def test_six_columns_without_the_flag_seven_with_it(exe, job, tag, strains, env):
    n0, off, out0, err0 = _run(exe, job, tag + "_off", ["--coverage-depth"], strains, **env)
    n1, on, out1, err1 = _run(exe, job, tag + "_on", ["--coverage-depth", "--coverage-background", "--background-spectrum"], strains, **env)
    assert n0 == [6] * len(strains), "without the flag every table has six columns"
    assert n1 == [7] * len(strains), "with the flag every table has one more"
    here0, here1 = str(job.d / (tag + "_off")).encode(), str(job.d / (tag + "_on")).encode()
    assert out0.replace(here0, b"") == out1.replace(here1, b"") and err0.replace(here0, b"") == err1.replace(here1, b"")
    for s in strains:
        assert off[s]["coverage_background"] is None and off[s]["coverage_background_spectrum"] is None
        assert on[s]["coverage_depth"] == off[s]["coverage_depth"] and on[s]["kmer_hits.gz"] == off[s]["kmer_hits.gz"]
        want, name = _want(job, s), model.strain_name(NAME % s)
        assert on[s]["coverage_background"] == model.table(name, want), s
        assert on[s]["coverage_background_spectrum"] == model.spectrum(name, want), s
        model.blocks_of_tables(on[s]["coverage_background"], on[s]["coverage_background_spectrum"])
    t, _ = model.parse_table(on[strains[-1]]["coverage_background"])
    assert t[(model.strain_name(NAME % strains[-1]), "pe_1.fq", "background")][2] > 0


def test_pe2s_unpaired_tail_is_counted(job):
    """the world tests it: strain 1's counts over the PE target differ with and without the 40 reads beyond PE1's last"""
    keys = model.strain_keys([job.strains[1]])
    whole = model.row_counts(keys, job.files["pe_1.fq"] + job.files["pe_2.fq"])
    paired = model.row_counts(keys, job.files["pe_1.fq"] + job.files["pe_2.fq"][: len(job.files["pe_1.fq"])])
    assert int(whole.sum()) > int(paired.sum()) and len(job.files["pe_2.fq"]) > len(job.files["pe_1.fq"]) + 40
