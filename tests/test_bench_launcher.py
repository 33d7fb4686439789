"""`python bench.py --gpus N` with no launcher around it must start its own N ranks (the driver's command is
the plain one, and round 3's bench.py answered it with "launch with torch.distributed.run").  The parent picks a free port,
runs `python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 ...` as a CHILD, passes exactly
one JSON line on and returns the child's status -- and never imports torch or the library itself (a process that has
initialised the GPU must not start others by exec; this one starts them without ever touching it).  The ranks here are a
stub (tests/native/bench_rank_stub.py, gloo): the real ranks need a GPU; tests/test_scale_checks_gpu.py runs those."""
import json
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUB = os.path.join(REPO, "tests", "native", "bench_rank_stub.py")


def _run(argv, **env):
    e = dict(os.environ, SK_BENCH_RANK_SCRIPT=STUB, **env)
    e.pop("WORLD_SIZE", None)
    e.pop("RANK", None)
    return subprocess.run([sys.executable, os.path.join(REPO, "bench.py")] + argv, env=e, capture_output=True, timeout=300)


def test_plain_command_starts_the_ranks_and_relays_one_line():
    p = _run(["--gpus", "2", "--steps", "7", "--warmup", "2", "--backend", "gloo"])
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    lines = p.stdout.decode().splitlines()
    assert len(lines) == 1                                                  # the noise of both ranks went to stderr
    line = json.loads(lines[0])
    assert line["n_gpus"] == 2 and line["value"] == 3 and line["steps"] == 7 and line["warmup"] == 2 and int(line["port"]) > 0
    err = p.stderr.decode()
    assert "noise on stdout from rank 0" in err and "noise on stdout from rank 1" in err
    assert "--nproc-per-node=2 --master-addr 127.0.0.1 --master-port %s" % line["port"] in err


def test_a_failing_rank_fails_the_plain_command():
    p = _run(["--gpus", "2", "--steps", "99", "--backend", "gloo"])
    assert p.returncode != 0 and p.stdout == b""


def test_the_parent_touches_neither_torch_nor_the_library():
    code = ("import runpy, sys\n"
            "sys.argv = ['bench.py', '--gpus', '2', '--steps', '1', '--backend', 'gloo']\n"
            "try:\n    runpy.run_path(%r, run_name='__main__')\nexcept SystemExit as e:\n    assert e.code == 0, e.code\n"
            "bad = [m for m in sys.modules if m == 'torch' or m.startswith('torch.') or m.startswith('strainer2_amd')]\n"
            "assert not bad, bad\nprint('parent clean', file=sys.stderr)\n" % os.path.join(REPO, "bench.py"))
    e = dict(os.environ, SK_BENCH_RANK_SCRIPT=STUB)
    e.pop("WORLD_SIZE", None)
    p = subprocess.run([sys.executable, "-c", code], env=e, capture_output=True, timeout=300)
    assert p.returncode == 0 and b"parent clean" in p.stderr, p.stderr.decode()[-2000:]


def test_under_a_launcher_the_world_must_match():
    e = dict(os.environ, WORLD_SIZE="3", RANK="0", SK_BENCH_RANK_SCRIPT=STUB)
    p = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "2", "--no-cpu"], env=e, capture_output=True, timeout=120)
    assert p.returncode != 0 and b"must be the same" in p.stderr


def _bench_module():
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(REPO, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_dump_outputs_writes_exact_float64_and_samples_over_budget(tmp_path, monkeypatch):
    """--dump-outputs DIR: each array as DIR/<name>.npy in float64 (u32 counts exactly); over the byte budget every array is cut
    to the same seeded sample of rows, the row indices beside it, and two dumps of the same arrays are the same files"""
    import numpy as np
    bench = _bench_module()
    counts = np.random.default_rng(1).integers(0, 2**32, size=1000, dtype=np.uint64).astype(np.uint32)
    assert bench.dump_outputs(str(tmp_path / "a"), {"counts_per_step": counts}) == {"counts_per_step": 1000}
    got = np.load(tmp_path / "a" / "counts_per_step.npy")
    assert got.dtype == np.float64 and np.array_equal(got.astype(np.uint32), counts)
    assert sorted(os.listdir(tmp_path / "a")) == ["counts_per_step.npy"]
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 4000)
    for d in ("b", "c"):
        written = bench.dump_outputs(str(tmp_path / d), {"counts_per_step": counts})
        assert 8 * sum(written.values()) <= 4000 and written["counts_per_step"] == written["counts_per_step_rows"] > 0
    rows = np.load(tmp_path / "b" / "counts_per_step_rows.npy").astype(np.int64)
    assert np.all(np.diff(rows) > 0)
    assert np.array_equal(np.load(tmp_path / "b" / "counts_per_step.npy").astype(np.uint32), counts[rows])
    for name in ("counts_per_step.npy", "counts_per_step_rows.npy"):
        assert (tmp_path / "b" / name).read_bytes() == (tmp_path / "c" / name).read_bytes()


def test_steps_below_one_is_refused_before_anything_starts():
    p = _run(["--gpus", "2", "--steps", "0", "--backend", "gloo"])
    assert p.returncode != 0 and p.stdout == b"" and b"--steps must be at least 1" in p.stderr


@pytest.mark.gpu
def test_a_plain_run_does_only_the_headline_and_full_adds_the_side_legs(tmp_path):
    """a plain `bench.py --gpus 1` sets up, times its steps, dumps and prints the line with no side leg in it; --full brings the
    CPU baseline, the PCIe-inclusive, packed-input and file-fed rates back (the strain_detect leg is left out here for time)"""
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR", "SK_BENCH_RANK_SCRIPT"):
        env.pop(k, None)
    argv = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--reads", "200000"]
    p = subprocess.run(argv + ["--dump-outputs", str(tmp_path)], env=env, capture_output=True, timeout=300)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    plain = json.loads(p.stdout.decode())
    assert plain["full"] is False and plain["steps"] == 3 and plain["value"] > 0 and plain["ms_per_step"] > 0
    assert plain["cpu_baseline"] is None and plain["strain_detect"] is None and plain["parity"]["checked"] is False
    cfg = plain["config"]
    assert cfg["pcie_inclusive_bases_per_s_host_buffers"] is None and cfg["packed_input_resident"] is None and cfg["file_fed_rank_sharded"] is None
    assert sorted(os.listdir(tmp_path)) == ["counts_per_step.npy"]
    p = subprocess.run(argv + ["--full", "--no-sd"], env=env, capture_output=True, timeout=600)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    full = json.loads(p.stdout.decode())
    assert full["full"] is True and full["cpu_baseline"]["value"] > 0 and full["strain_detect"] is None
    cfg = full["config"]
    assert cfg["pcie_inclusive_bases_per_s_host_buffers"] > 0 and cfg["packed_input_resident"]["bases_per_s"] > 0
    assert cfg["file_fed_rank_sharded"]["bases_per_s"] > 0
    assert full["config"]["hits_per_pass_rank0_or_sum"] == plain["config"]["hits_per_pass_rank0_or_sum"] > 0
