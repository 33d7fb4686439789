#!/usr/bin/env python3
"""sk_recur_finish measured from the library (one MI355X): 32 members of 50 000 bits, T = 20, 256 and 4096 samples, each plane with
1 % of its bits set at random plus one bit per member set in every plane.  Per T: the wall time of finish() -- the sweep(s), the copy
home and the host's mirror of the triangle -- histogram alone and, up to SK_RECUR_PAIRS_MAX samples, with the pair table; seven calls
each, all printed.  The tables are checked against their invariants, not against a model (tests/test_coverage_recurrence_gpu.py
does that).

    python tools/recurrence_finish_bench.py [--out FILE]
"""
import argparse
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import strainer2_amd as sk  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", type=int, default=32)
    ap.add_argument("--bits", type=int, default=50000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    rng = np.random.default_rng(3)
    nbits = [args.bits] * args.members
    with sk.KmerContext(0) as ctx:
        for T in (20, 256, 4096):
            with sk.Recurrence(ctx, nbits, T) as r:
                t0 = time.perf_counter()
                for s in range(T):
                    for m in range(args.members):
                        r.mark_bits(m, s, np.concatenate([[m], rng.integers(0, args.bits, args.bits // 100)]))
                t_mark = time.perf_counter() - t0
                res = {}
                for pairs in ([False, True] if T <= sk.SK_RECUR_PAIRS_MAX else [False]):
                    ts = []
                    for _ in range(7):
                        t0 = time.perf_counter()
                        got = r.finish(pairs=pairs)
                        ts.append((time.perf_counter() - t0) * 1e3)
                    res[pairs] = ts
                    hist = got[0] if pairs else got
                    assert (hist.sum(axis=1) == args.bits).all() and (hist[:, T] >= 1).all()
                    if pairs:
                        sh = got[1]
                        assert (sh == sh.transpose(0, 2, 1)).all()
                        assert ((np.arange(T + 1) * hist).sum(axis=1) == np.trace(sh, axis1=1, axis2=2)).all()
                say(f"T = {T}: {args.members} members x {args.bits} bits, {T * args.members} mark calls in {t_mark:.2f} s; finish, histogram alone: "
                    + " ".join(f"{t:.3f}" for t in res[False]) + " ms"
                    + ("; with the pair table: " + " ".join(f"{t:.3f}" for t in res[True]) + " ms" if True in res else ""))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
