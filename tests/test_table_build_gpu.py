"""The table built on the device (sk_table_build_from_text: sk_build_insert, sk_build_first, sk_build_rank_scan, sk_build_index,
sk_grid_insert_text) and what reads it (sk_first_pos_from_rank, the scans) at the builder's structural edges, against a plain model
of what it must leave behind (tests/_build_model.py; the model and every world's premise are checked on the CPU in
tests/test_table_build_host.py) and against the oracle's counts.  Every comparison is equality of integers.

  one<L>       one record of L = 31..129 bases: the text's words and the rank map's blocks at their boundaries, the last window, the
               last places of the text in sk_grid_insert_text
  thirty_ones  2,000 records of 31 bases: one window each, a start at every place of a 64-position block
  n_runs       N runs and lower case: blocks without a start bit, code 0 under N
  poly_a, tandem<p>  thousands of windows on one to 64 slots: atomicMin keeps the lowest position and its orientation bit
  strands      keys first seen on the other strand; duplicates, which get no rank bit
  rank<nblk>_r<r>    sk_build_rank_scan with per = 1, 2, 3, idle threads, a partial last slice, *total
  big          1.05 Mbase: the grid-stride loops of sk_first_pos_from_rank and sk_fill64, per = 17
  step<pct>_<slots>_<tag>  nstarts on, over and under the step of the slot count, all keys distinct, and as a tandem repeat
  no window    nstarts == 0: an empty table

Each world is scanned in both forms, scan_stream and scan_device."""
import numpy as np
import pytest

import _build_model as bm
import strainer2_amd as sk
from test_hash_worlds_gpu import _context

pytestmark = pytest.mark.gpu

NO_POS = 0xFFFFFFFF
COL0 = 3


def _scan_both(c, stream):
    """the stream into column 1 by scan_stream and into column 2 by scan_device"""
    c.scan_stream(stream, 1)
    buf = c.dev_alloc(len(stream) + 16)
    c.dev_upload(buf, np.frombuffer(stream, dtype=np.uint8))
    c.scan_device(buf, len(stream), 2)
    c.sync()
    c.dev_free(buf)


def _check_built(c, name, nrows):
    """context c holds the table built from world `name`: structure against the model, a scan against the oracle"""
    m = bm.model(name)
    assert nrows == c.nrows == m.nrows, (name, nrows, m.nrows)
    keys = bm.exported_keys(c)
    assert np.array_equal(keys, m.keys), (name, "keys in row order", np.nonzero(keys != m.keys)[0][:10])
    pos = c.first_pos().astype(np.int64)
    assert np.array_equal(pos, m.pos), (name, "first positions", np.nonzero(pos != m.pos)[0][:10])
    assert (np.diff(pos) > 0).all()
    assert np.array_equal(c.counts(0), np.full(nrows, COL0, dtype=np.uint32)), (name, "column 0")
    some = np.array([nrows - 1, 0, min(17, nrows - 1), min(17, nrows - 1), nrows // 2], dtype=np.uint32)
    assert np.array_equal(bm.exported_keys(c, some), keys[some]), (name, "sk_table_export_keys_of")
    stream = bm.scan_stream_of(name)
    okeys, ocounts = bm.oracle_rows(bm.records(name), stream)
    want = ocounts[bm.rows_of(keys, okeys)]
    assert len(okeys) == nrows and want.sum() > 0
    _scan_both(c, stream)
    for col, form in ((1, "scan_stream"), (2, "scan_device")):
        got = c.counts(col)
        assert np.array_equal(got, want), (name, form, np.nonzero(got != want)[0][:10], int(got.sum()), int(want.sum()))
    assert np.array_equal(c.counts(0), np.full(nrows, COL0, dtype=np.uint32)) and not c.counts(3).any()


@pytest.mark.parametrize("name", list(bm.WORLDS))
def test_table_built_on_the_device_at_its_edges(name):
    with sk.KmerContext(0) as c:
        _check_built(c, name, c.build_from_text(bm.records(name), 4, COL0))


@pytest.mark.parametrize("name", list(bm.STEP_WORLDS))
def test_slot_count_step(name):
    """nstarts the largest that keeps 1,024 or 2,048 slots at 50 and 90 % load, one more (the table doubles), one fewer; and the same
    nstarts as one tandem repeat: slots sized for windows that are five keys"""
    with _context(bm.load_pct(name)) as c:
        _check_built(c, name, c.build_from_text(bm.records(name), 4, COL0))


def test_text_without_a_window():
    """nstarts == 0 through sk_table_build_from_text itself (skh_keyset_build_on_device never hands such a text over): SK_OK and no
    row; nothing to export, no first position; scans of any stream return and count nothing; the context builds its next table as
    if nothing had been"""
    recs = bm.EMPTY_WORLD()
    stream = bm.scan_stream_of("one129") + b"\n".join(recs) + b"\n"
    with sk.KmerContext(0) as c:
        assert c.build_from_text(recs, 4, COL0) == 0 and c.nrows == 0 and c.ncols == 4
        assert len(c.first_pos()) == 0 and len(bm.exported_keys(c)) == 0
        _scan_both(c, stream)
        assert len(c.counts(1)) == 0 and len(c.counts(2)) == 0
        _check_built(c, "one129", c.build_from_text(bm.records("one129"), 4, COL0))
        assert c.build_from_text(recs, 4, COL0) == 0 and c.nrows == 0      # and an empty table after a full one
        _scan_both(c, stream)
        assert len(c.first_pos()) == 0
