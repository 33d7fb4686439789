#!/usr/bin/env python3
"""tools/half_launch_probe.py -- what one extra launch boundary costs: the resident cfg-2 batch scanned as ONE launch and as TWO
launches of half the tiles each (cut at a tile edge; the counts of the windows across the cut differ, the work does not), wall
time per pass over STEPS passes.  The difference between the two is one more drain + ramp + inter-kernel gap per pass.
SCAN_LANES=1|2 sets the context's "scan_lanes" option where the library has it."""
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import strainer2_amd as sk  # noqa: E402
from strainer2_amd import synth  # noqa: E402

READS = int(os.environ.get("READS", "10000000"))
STEPS = int(os.environ.get("STEPS", "300"))
TILE = 32768
contigs = synth.make_strain()
ks = sk.Keyset.from_stream(synth.strain_stream(contigs))
reads, nb = synth.make_reads(contigs, READS, 150, seed=synth.SEED + 1)
n = int(reads.size)
half = (n // TILE // 2) * TILE
with sk.KmerContext(0) as ctx:
    if os.environ.get("SCAN_LANES"):
        ctx.set_option("scan_lanes", int(os.environ["SCAN_LANES"]))
    ctx.load_keyset(ks, 4)
    dev = ctx.dev_alloc(n)
    ctx.dev_upload(dev, reads)
    pieces = {"one launch": [(dev, n)], "two half launches": [(dev, half), (dev + half, n - half)]}
    for _ in range(600):                                  # the card's running clocks
        ctx.scan_device(dev, n, 2)
    ctx.sync()
    res = {}
    for rep in range(3):
        for label, parts in pieces.items():
            ctx.sync()
            ctx.scan_timing(reset=True)
            t0 = time.perf_counter()
            for _ in range(STEPS):
                for p, m in parts:
                    ctx.scan_device(p, m, 2)
            ctx.sync()
            wall = (time.perf_counter() - t0) * 1e3 / STEPS
            ms, nl = ctx.scan_timing(reset=True)
            res.setdefault(label, []).append(wall)
            print(f"{label:18s} rep {rep}: wall {wall * 1e3:8.2f} us per pass, scan kernels {ms / STEPS * 1e3:8.2f} us per pass ({nl} launches)", flush=True)
    a, b = min(res["one launch"]), min(res["two half launches"])
    print(f"one extra boundary: {(b - a) * 1e3:.2f} us per pass ({(b - a) / a * 100:.2f} % of {a * 1e3:.2f} us)")
