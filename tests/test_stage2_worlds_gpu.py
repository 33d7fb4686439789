"""Stage 2 of the scan kernel (sk_scan_grid: seed, verify on the diagonal, ranks, runs of rows, the rest one by one) on the GPU, in
worlds built around the places where random reads with substitutions cannot show a mistake (tests/_stage2_worlds.py; their
premises: tests/test_stage2_worlds_host.py), in every form of the kernel, against the oracle.  Every comparison is exact.

  shift   breakpoints (deletions, insertions, jumps, the other strand) at every place of a chunk: the three-question filter's
          window ranges, where one window rejected too many is a k-mer of the strain
  ends    strains of 31..129 and 4000 bases read whole and by their ends at every phase, both strands: the guard of the 48-base
          compare at position 0 and at the text's end, the loads behind it; and the same across the members of a union
  seams   reads that equal the text across a record junction or an N: verified windows that are no k-mer there (no rank bit), and
          in four variants are one elsewhere
  runs    (COUNT) runs of rows split by repeats, merged across chunks, waves and tiles, through the tile's table of indices
  diff    the difference array and its three flush kernels at nrows + 1 around multiples of 4096

Forms: COUNT with text_stage 1 and 0 (0: the control, none of stage 2's text), pipeline 2, resident on the device twice (both lanes),
the host-packed form on the device, one TALLY launch, the TALLY launch of a union.  And one form more, for shift, ends and seams: every
table built on the device from the strain's records (COUNT, packed, resident twice, TALLY, a union of members all built there)."""
import numpy as np
import pytest

import _oracle
import _stage2_worlds as w2
import _synth
import strainer2_amd as sk

pytestmark = pytest.mark.gpu


def test_shift_in_every_form():
    w2.run_every_form(w2.shift_world())


@pytest.mark.parametrize("L", w2.ENDS_LENGTHS)
def test_ends_in_every_form(L):
    w2.run_every_form(w2.ends_world(L), union=False)


@pytest.mark.parametrize("pair", w2.ENDS_UNIONS, ids=lambda p: "%d+%d" % p)
def test_ends_of_union_members_in_every_form(pair):
    w2.run_every_form(w2.ends_union_world(pair))


@pytest.mark.parametrize("main", range(5), ids=["records", "N-A", "N-C", "N-G", "N-T"])
def test_seams_in_every_form(main):
    w2.run_every_form(w2.seams_world(), main=main, union=main == 0)


def test_runs_in_every_count_form():
    w2.run_every_form(w2.runs_world(), tally=False, union=False)


# ---- the same worlds on tables the device built itself (sk_table_build_from_text) ----------------------------------------------------------
def _device_form(w):
    """the id of a case of the form "built on the device": a world whose strains hold a letter build_from_text cannot take (U, an
    IUPAC letter) says so and runs nothing"""
    return "device" if w2.device_buildable(w) else "device-not-run-strain-has-U-or-IUPAC"


def _built_on_the_device(w, **kw):
    if w2.device_buildable(w):
        w2.run_every_form(w, built="device", **kw)


_ENDS = [pytest.param(L, id="%d-%s" % (L, _device_form(w2.ends_world(L)))) for L in w2.ENDS_LENGTHS]
_UNIONS = [pytest.param(p, id="%d+%d-%s" % (p + (_device_form(w2.ends_union_world(p)),))) for p in w2.ENDS_UNIONS]
_SEAMS = [pytest.param(m, id="%s-%s" % (n, _device_form(w2.seams_world()))) for m, n in enumerate(["records", "N-A", "N-C", "N-G", "N-T"])]


def test_shift_built_on_the_device():
    assert _device_form(w2.shift_world()) == "device"
    _built_on_the_device(w2.shift_world())


@pytest.mark.parametrize("L", _ENDS)
def test_ends_built_on_the_device(L):
    _built_on_the_device(w2.ends_world(L), union=False)


@pytest.mark.parametrize("pair", _UNIONS)
def test_ends_of_union_members_built_on_the_device(pair):
    _built_on_the_device(w2.ends_union_world(pair))


@pytest.mark.parametrize("main", _SEAMS)
def test_seams_built_on_the_device(main):
    _built_on_the_device(w2.seams_world(), main=main, union=main == 0)


@pytest.mark.parametrize("resident", [False, True], ids=["scan_stream", "scan_device"])
@pytest.mark.parametrize("nrows", w2.DIFF_NROWS)
def test_difference_array_geometry(nrows, resident):
    """a strain of exactly nrows keys: itself and its reverse complement into column 1 (every row twice: one run over all rows, its
    closing entry behind the last row), then three reads of its last 80 bases into column 2 -- the change of column flushes column 1,
    whose last block is the partial one.  Both columns are the oracle's, and the same when fetched again: the array was left zero."""
    _, g = w2.diff_strain(nrows)
    whole, tail = g + b"\n" + _synth.revcomp(g) + b"\n", (g[-80:] + b"\n") * 3
    t = _oracle.OracleTable(capacity=w2.SLOTS)
    assert t.build_stream(g + b"\n", default=1, incr=0, short_policy=1) == 0
    t.scan_stream(whole, 1)
    t.scan_stream(tail, 2)
    okeys, ocounts = t.rows()
    t.close()
    ks = sk.Keyset.from_stream(g + b"\n", initial_slots=w2.SLOTS, default_val=1, incr=0)
    try:
        assert ks.nrows == nrows and ks.keys() == okeys
        assert (ocounts[:, 1] == 2).all() and int(ocounts[:, 2].sum()) == 3 * min(50, nrows)
        with sk.KmerContext(0) as c:
            c.load_keyset(ks, 4)
            bufs = []
            for data, col in ((whole, 1), (tail, 2)):
                if resident:
                    bufs.append(c.dev_alloc(len(data)))
                    c.dev_upload(bufs[-1], np.frombuffer(data, dtype=np.uint8))
                    c.scan_device(bufs[-1], len(data), col)
                else:
                    c.scan_stream(data, col)
            for again in range(2):
                for col in (1, 2):
                    got = c.counts(col)
                    assert np.array_equal(got, ocounts[:, col]), (nrows, col, again, np.nonzero(got != ocounts[:, col])[0][:10])
            for b in bufs:
                c.dev_free(b)
    finally:
        ks.close()
