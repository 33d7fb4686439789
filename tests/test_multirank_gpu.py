"""N > 1 on the one card of a gpurun box (gloo: RCCL wants a device per rank; the in-library RCCL sequence is covered on the CPU by
tests/test_multirank_protocol.py).  VERDICT r03 item 1: (a) the PLAIN command `python bench.py --gpus 2` must start its own ranks
and print one parity-checked line; (b) a cut that does not hold must not fail a multi-rank scan -- dist.scan_list_sharded makes
every rank put its column back and scan the whole-file plan (src/genome_compare.c:203 accepts such files with exit 0)."""
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch.multiprocessing as tmp

import _synth

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)


def test_plain_bench_command_at_two_ranks_is_parity_checked():
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "2", "--steps", "5", "--warmup", "2", "--backend", "gloo",
                        "--full", "--no-cpu", "--no-sd"], env=env, capture_output=True, timeout=840)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    lines = p.stdout.decode().splitlines()
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["n_gpus"] == 2 and line["steps"] == 5 and line["scaling"] == "weak"
    assert line["parity"]["checked"] is True                  # each rank's stream == the reference's vector for that rank (cfg2_facts.json)
    assert line["value"] > 1e11
    ff = line["config"]["file_fed_rank_sharded"]
    assert ff and "bases_per_s" in ff, ff


def _worker(rank, world, port, d, split):
    sys.path.insert(0, REPO)
    import torch.distributed as dist
    import strainer2_amd as sk
    from strainer2_amd.dist import allreduce_count_array, scan_list_sharded
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ["SK_THREADS"] = "3"
    if split:
        os.environ["SK_SPLIT_BYTES"] = split
    dist.init_process_group("gloo", rank=rank, world_size=world)
    ks = sk.Keyset.from_file(os.path.join(d, "strain.fa"))
    with sk.KmerContext(0) as ctx:
        ctx.load_keyset(ks, 4)
        before = np.arange(ks.nrows, dtype=np.uint32) % 7            # what is in the column must survive the round trip
        ctx.set_counts(2, before)
        bases = scan_list_sharded(ctx, os.path.join(d, "list.txt"), 2, rank, world)
        col = ctx.counts(2) - before
    total = allreduce_count_array(np.ascontiguousarray(col))
    np.save(os.path.join(d, f"rank{rank}.npy"), total)
    np.save(os.path.join(d, f"bases{rank}.npy"), np.array([bases], dtype=np.uint64))
    dist.destroy_process_group()


def test_sharded_scan_goes_round_again_uncut_when_a_cut_does_not_hold(tmp_path):
    import strainer2_amd as sk
    rng = random.Random(23)
    strain = _synth.rand_dna(rng, 30000)
    (tmp_path / "strain.fa").write_bytes(b">s\n" + strain + b"\n")

    def fastq(n):
        out = []
        for i in range(n):
            a = rng.randrange(0, len(strain) - 150)
            out.append(b"@r%d\n%s\n+\n%s\n" % (i, strain[a:a + 150] if rng.random() < 0.6 else _synth.rand_dna(rng, 150), b"I" * 150))
        return b"".join(out)
    recs = []
    for i in range(400):
        a = rng.randrange(0, len(strain) - 150)
        s = strain[a:a + 150]
        q = b"@" + b"I" * 49 + b"\n" + b"I" * 50 + b"\n" + b"+" + b"I" * 49
        recs.append(b"@r%d\n%s\n%s\n%s\n+\n%s\n" % (i, s[:50], s[50:100], s[100:], q))
    (tmp_path / "wrapped.fq").write_bytes(b"".join(recs))
    bad = b"@bad\n" + strain[100:250] + b"\n+\n" + b"I" * 170 + b"\n"
    (tmp_path / "whole.fq").write_bytes(fastq(300) + bad + fastq(300))
    (tmp_path / "ok.fq").write_bytes(fastq(500))
    (tmp_path / "list.txt").write_text("".join(str(tmp_path / n) + "\n" for n in ("ok.fq", "wrapped.fq", "whole.fq", "ok.fq")))
    ks = sk.Keyset.from_file(str(tmp_path / "strain.fa"))
    os.environ["SK_NO_SPLIT"] = "1"
    try:
        with sk.KmerContext(0) as ctx:
            ctx.load_keyset(ks, 4)
            want_bases = ctx.scan_list(str(tmp_path / "list.txt"), 2)
            want = ctx.counts(2)
    finally:
        del os.environ["SK_NO_SPLIT"]
    assert want.sum() > 10000
    port = 29500 + os.getpid() % 2000
    tmp.spawn(_worker, args=(2, port, str(tmp_path), "5000"), nprocs=2, join=True)
    r0, r1 = np.load(tmp_path / "rank0.npy"), np.load(tmp_path / "rank1.npy")
    assert np.array_equal(r0, r1) and np.array_equal(r0, want)
    assert int(np.load(tmp_path / "bases0.npy")[0]) + int(np.load(tmp_path / "bases1.npy")[0]) == want_bases
