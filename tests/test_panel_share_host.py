"""strain_detect -S --panel-share=FILE, the parts that need no device: the new ABI entry (header, export list, library symbol, the
Python method), the model's arithmetic (tests/_panel_model.py) on a hand-written example, the command lines the flag refuses before
anything is opened -- each with one line on stderr, a non-zero status and nothing written -- the word behind kmer_scrub_count's
--detect, and a build of the host layer without the device's entry point."""
import os
import re
import subprocess

import numpy as np
import pytest

import _panel_model as model
import _synth
import strainer2_amd as sk
from strainer2_amd import native
from test_coverage_regions_host import ONE, _job, _refused, _run

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MANY = ["-S", "S.txt", "-B", "T.txt"]


def test_the_new_entry_point_is_declared_listed_and_exported(repo):
    hdr = open(os.path.join(repo, "include", "strainer_kmer.h")).read()
    syms = subprocess.run(["nm", "-D", "--defined-only", sk.library_path()], capture_output=True, text=True).stdout
    assert re.search(r"\bsk_union_share\(", hdr)
    assert "sk_union_share" in native.ABI_SYMBOLS
    assert re.search(r"\bT sk_union_share$", syms, re.M)
    assert model.HEADER.decode().rstrip("\n").replace("\t", "<TAB>") in hdr
    assert callable(getattr(sk.KmerUnion, "share", None))


def test_the_models_arithmetic_on_three_strains_by_hand():
    """strain 0 holds a b c d (informative a b), strain 1 holds b c e (informative b e), strain 2 holds f (informative nothing)"""
    keys = [{"a", "b", "c", "d"}, {"b", "c", "e"}, {"f"}]
    inf = [{"a", "b"}, {"b", "e"}, set()]
    m0, m1, m2 = model.share(keys, inf)
    assert m0.tolist() == [[4, 2, 0], [2, 3, 0], [0, 0, 1]]
    assert m1.tolist() == [[2, 1, 0], [1, 2, 0], [0, 0, 0]]      # a's informative keys that b holds: of {a, b} strain 1 holds b; of {b, e} strain 0 holds b
    assert m2.tolist() == [[2, 1, 0], [1, 2, 0], [0, 0, 0]]
    # a foreign side: the columns are the other list's members
    n0, n1, n2 = model.share(keys[:2], inf[:2], [{"a", "e", "f"}], [{"e"}])
    assert n0.tolist() == [[1], [1]] and n1.tolist() == [[1], [1]] and n2.tolist() == [[0], [1]]
    want = (b"strain_a\tstrain_b\tkmers_a\tinformative_a\tshared_kmers\tinformative_a_in_b\tinformative_both\n"
            b"x\tx\t4\t2\t4\t2\t2\nx\ty\t4\t2\t2\t1\t1\nx\tz\t4\t2\t0\t0\t0\n"
            b"y\tx\t3\t2\t2\t1\t1\ny\ty\t3\t2\t3\t2\t2\ny\tz\t3\t2\t0\t0\t0\n"
            b"z\tx\t1\t0\t0\t0\t0\nz\ty\t1\t0\t0\t0\t0\nz\tz\t1\t0\t1\t0\t0\n")
    assert model.table(["x", "y", "z"], m0, m1, m2) == want
    assert model.strain_name("d/Genus_species_a.kmer_hits.gz") == "Genus_species_a" and model.strain_name("d/plain.gz") == "plain.gz"
    with pytest.raises(AssertionError):
        model.share([{"a"}], [{"b"}])


def test_the_models_keys_are_the_librarys(tmp_path):
    """the informative lists name k-mers as text on either strand; a key is the larger of a word and its reverse complement"""
    import random
    g = _synth.rand_dna(random.Random(11), 300)
    (tmp_path / "g.fa").write_bytes(b">g\n" + g + b"\n")
    keys = model.keys_of_genome(tmp_path / "g.fa")
    words = {g[i:i + 31] for i in range(len(g) - 30)}
    assert keys == {model.canonical(w) for w in words} == {model.canonical(_synth.revcomp(w)) for w in words}
    (tmp_path / "a.txt").write_bytes(b"#c\n" + g[5:36] + b"\n" + _synth.revcomp(g[40:71]) + b"\n" + g[80:110] + b"\n" + g[120:151].lower() + b"\n")
    assert model.keys_of_list(tmp_path / "a.txt") == {model.canonical(g[5:36]), model.canonical(g[40:71])}


@pytest.mark.parametrize("flag", ["--panel-share", "--panel-share="])
def test_the_flag_without_a_file_name_is_refused(tmp_path, flag):
    before = _job(tmp_path)
    p = _run(MANY + [flag], str(tmp_path))
    _refused(p, before, tmp_path)
    assert b"--panel-share=FILE needs a file name" in p.stderr


@pytest.mark.parametrize("argv", [ONE, ONE + ["-S", "S.txt"], ONE + ["--coverage-only"]])
def test_the_flag_without_several_strains_is_refused(tmp_path, argv):
    before = _job(tmp_path)
    p = _run(argv + ["--panel-share=x.tsv"], str(tmp_path))
    _refused(p, before, tmp_path)
    assert p.stderr == b"strain_detect: --panel-share goes with -S: it compares the strains of a panel\n"


def _run_env(argv, cwd, **env):
    return subprocess.run([sk.cli_path("strain_detect")] + argv, cwd=cwd, env=dict(os.environ, **env), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                          timeout=120)


@pytest.mark.parametrize("var", ["WORLD_SIZE", "SK_WORLD_SIZE"])
def test_more_than_one_rank_is_refused(tmp_path, var):
    before = _job(tmp_path)
    p = _run_env(MANY + ["--panel-share=x.tsv"], str(tmp_path), **{var: "2", "RANK": "0"})
    _refused(p, before, tmp_path)
    assert b"--panel-share" in p.stderr and b"each rank holds only its own strains" in p.stderr


@pytest.mark.parametrize("devices", ["2", "0,1", "0,0,1"])
def test_more_than_one_physical_device_is_refused(tmp_path, devices):
    before = _job(tmp_path)
    p = _run_env(MANY + ["--panel-share=x.tsv"], str(tmp_path), SK_DEVICES=devices)
    _refused(p, before, tmp_path)
    assert b"--panel-share" in p.stderr and b"one-device run" in p.stderr


def test_the_word_behind_detect(tmp_path):
    """kmer_scrub_count -S ... --detect ... --panel-share=x passes sm_check_detect (the run then stops at the next check, which
    SK_DEVICES trips on purpose: no device is needed); without =FILE the word is refused there"""
    before = _job(tmp_path)
    exe = sk.cli_path("kmer_scrub_count")
    argv = ["-S", "S.txt", "-A", "T.txt", "-B", "T.txt", "--scrub", "0.5", "--detect", "-B", "T.txt"]
    env = dict(os.environ, SK_DEVICES="1")
    p = subprocess.run([exe] + argv + ["--panel-share=x.tsv"], cwd=str(tmp_path), env=env, capture_output=True, timeout=120)
    _refused(p, before, tmp_path)
    assert b"panel-share" not in p.stderr and b"SK_DEVICES is not for this run" in p.stderr
    for flag in ("--panel-share", "--panel-share="):
        p = subprocess.run([exe] + argv + [flag], cwd=str(tmp_path), env=env, capture_output=True, timeout=120)
        _refused(p, before, tmp_path)
        assert b"--panel-share=FILE needs a file name" in p.stderr


def test_a_library_without_the_entry_point_says_so(tmp_path):
    """sk_host_sd.c reaches sk_union_share through a weak reference: the host layer links against the CPU double, which has no such
    symbol, runs -S as ever without the flag, and with it refuses before anything is opened"""
    srcs = [os.path.join(REPO, "tests", "native", "device_double.c")] + \
           [os.path.join(REPO, "strainer2_amd", "csrc", f) for f in ("sk_host.c", "sk_host_sd.c", "sk_host_cov.c")]
    exe = str(tmp_path / "sd_double")
    subprocess.run(["gcc", "-O1", "-g"] + srcs + ["-lz", "-lpthread", "-o", exe], check=True)
    d = tmp_path / "job"
    d.mkdir()
    before = _job(d)
    p = _run(MANY + ["--panel-share=x.tsv"], str(d), exe=exe)
    _refused(p, before, d)
    assert p.stderr == b"strain_detect: --panel-share: this build has no sk_union_share\n"
    p = _run(MANY, str(d), exe=exe)
    assert p.returncode == 0, p.stderr
    assert os.path.exists(d / "Genus_species_a.kmer_hits.gz") and not os.path.exists(d / "x.tsv")
