"""The scrub sweep (include/strainer_kmer.h has the rule) in Python: the model every sweep test compares against.

The sets come from running the EXISTING single-fraction step 2 once per fraction -- the filter oracle (oracle/ksf_oracle) or
kmer_scrub_filter -m f, both pinned to the reference script by tests/golden/filter_cases -- never from the code under test:

sets_by_runs(run, fractions)      run(f) -> the stdout of step 2 at fraction f (None: the run failed)  ->  [informative list per f]
assert_nested / classes           the premise itself (set q + 1 is a subsequence of set q), and every k-mer's class from the sets
class_file(fractions, sets)       the class file's bytes
sweep_table(...)                  the sweep table's bytes from the separate runs' main coverage tables
parse_sweep                       the table as {sample: [(fraction text, set size, unique, total)]}
numbers_by_class(...)             (depth, class) per row -> (unique[F], total[F], stray): the device pass in numpy"""
import numpy as np

HEADER = (b"strain_name\tmetagenome\tmin_fraction\tgenome_num_informative_kmers\tunique_observed_informative_kmers\t"
          b"total_observed_informative_kmers")
LISTS = ("0.9,0.5,0.04,0.01,0", "1,0")


def informative(stdout):
    """step 2's stdout -> its informative list, in order"""
    return [ln for ln in stdout.split(b"\n") if ln and not ln.startswith(b"#")]


def sets_by_runs(run, fractions):
    out = []
    for f in fractions:
        got = run(f)
        if got is None:
            return None
        out.append(informative(got))
    return out


def assert_nested(sets):
    """set q + 1 keeps the order of set q and drops some of its k-mers; no k-mer twice"""
    for big, small in zip(sets, sets[1:]):
        it = iter(big)
        assert all(any(k == x for x in it) for k in small), "not a subsequence"
    for s in sets:
        assert len(set(s)) == len(s)


def classes(sets):
    """{k-mer: class}: the number of sets that hold it (nested: the first `class` of them)"""
    assert_nested(sets)
    cl = {}
    for s in sets:
        for k in s:
            cl[k] = cl.get(k, 0) + 1
    for q, s in enumerate(sets):
        assert all(cl[k] >= q + 1 for k in s) and sum(c >= q + 1 for c in cl.values()) == len(s)
    return cl


def class_file(fractions, sets):
    cl = classes(sets)
    head = b"#min_fractions\t" + ",".join(fractions).encode() + b"\n#post_scrub_kmers\t" + ",".join(str(len(s)) for s in sets).encode() + b"\n"
    return head + b"".join(b"%s\t%d\n" % (k, cl[k]) for k in sets[0])


def main_rows(table):
    """a main coverage table -> (strain name, {sample: (informative, unique, total)} in its order)"""
    out, name = {}, None
    for ln in table.split(b"\n")[1:]:
        if ln:
            f = ln.split(b"\t")
            name = f[0]
            out[f[5]] = (int(f[4]), max(int(f[8]), 0), int(f[9]))
    return name, out


def sweep_table(fractions, tables):
    """tables[q]: the main coverage table of the separate run at fractions[q]; the samples and their order are those of tables[0];
    a sample that a smaller fraction's run does not list (none of its hits left) has zeros there"""
    name, first = main_rows(tables[0])
    per = [main_rows(t)[1] for t in tables]
    sizes = [next(iter(p.values()))[0] if p else 0 for p in per]
    out = [HEADER + b"\n"]
    for s in first:
        for q, f in enumerate(fractions):
            _, u, n = per[q].get(s, (0, 0, 0))
            out.append(b"%s\t%s\t%s\t%d\t%d\t%d\n" % (name, s, f.encode(), sizes[q], u, n))
    return b"".join(out)


def parse_sweep(table):
    rows = table.split(b"\n")
    assert rows[0] == HEADER and rows[-1] == b""
    out = {}
    for ln in rows[1:-1]:
        f = ln.split(b"\t")
        assert len(f) == 6
        out.setdefault(f[1], []).append((f[2].decode(), int(f[3]), int(f[4]), int(f[5])))
    return out


def numbers_by_class(depth, cls, ncls):
    """per row its depth counter and its class -> (unique[ncls], total[ncls], stray): fraction q counts the non-zero rows of class
    q + 1 .. ncls; non-zero rows of class 0 or above ncls are stray"""
    depth = np.asarray(depth, dtype=np.uint64)
    cls = np.asarray(cls, dtype=np.int64)
    nz = depth > 0
    ok = nz & (cls >= 1) & (cls <= ncls)
    uq = np.array([int((ok & (cls >= q + 1)).sum()) for q in range(ncls)], dtype=np.uint64)
    tot = np.array([int(depth[ok & (cls >= q + 1)].sum()) for q in range(ncls)], dtype=np.uint64)
    return uq, tot, int((nz & ~ok).sum())


def joint_classes(pan, meta, gone, n_scrub):
    """sk_filter_classes_joint in numpy: the stable descending sort of the scores, a prefix of n_scrub[q] rows gone per fraction"""
    pan, meta, gone = np.asarray(pan, dtype=np.int64), np.asarray(meta, dtype=np.int64), np.asarray(gone, dtype=np.uint8)
    n = len(pan)
    ps, ms = int(pan[pan > 0].sum()), int(meta[meta > 0].sum())
    score = np.zeros(n)
    with np.errstate(divide="ignore", invalid="ignore"):
        if ms:
            score = np.maximum(score, np.where(meta > 0, meta / float(ms), 0.0))
        if ps:
            score = np.maximum(score, np.where(pan > 0, pan / float(ps), 0.0))
    alive = np.flatnonzero(gone == 0)
    order = alive[np.argsort(-score[alive], kind="stable")]
    cl = np.zeros(n, dtype=np.uint8)
    kept = []
    for k in n_scrub:
        keep = np.zeros(n, dtype=bool)
        keep[order[int(k):]] = True
        cl += keep.astype(np.uint8)
        kept.append(int(keep.sum()))
    return cl, np.array(kept, dtype=np.uint64), ps, ms


def above_classes(pan, meta, gone, pan_thr, meta_thr):
    pan, meta, gone = np.asarray(pan, dtype=np.int64), np.asarray(meta, dtype=np.int64), np.asarray(gone, dtype=np.uint8)
    cl = np.zeros(len(pan), dtype=np.uint8)
    kept = []
    for tp, tm in zip(pan_thr, meta_thr):
        keep = ~((gone != 0) | ((pan > 0) & (pan > tp)) | ((meta > 0) & (meta > tm)))
        cl += keep.astype(np.uint8)
        kept.append(int(keep.sum()))
    return cl, np.array(kept, dtype=np.uint64)
