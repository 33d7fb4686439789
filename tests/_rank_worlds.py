"""Crafted worlds for step 2's ranking (sk_filter.hip) and step 4's hit-list counters (sk_cover.hip), with the models they are
checked against.  Nothing here needs a GPU; tests/test_rank_worlds_host.py proves that every world has the property it is built for.

score_model / joint_model / classes_model   the script's score (int -> double by round-to-nearest-even, IEEE division, max of the two
                                            shares) and its stable descending sort, in numpy
tie_params / tie_world / tie_table          rows that tie ACROSS the two columns: 3k / 3S and k / S are one double under a correctly
                                            rounded division and two under a reciprocal multiply or a float32 division
ulp_ladder / digit_ladder / nibble_ladder / exponent_ladder   keys one apart, and keys that differ in one byte of one radix pass
one_world / zero_world / bigint_world / eq_scan_world         a score of 1.0, alive rows of score 0, integers that meet as doubles,
                                            a tie run over the shares of flt_eq_scan's threads
hist_column                                 a column for flt_hist's LDS / global split
cov_mix / probe_walk / segment_slots        sk_cover.hip's hash, its linear probe and the host's segment sizes
end_keys / segment_world / recurrence_world keys that home in the last slots of a segment, so that the probe must wrap
first_seen_model / general_hits             the script's global `seen` rule, and a hit list that switches to general mode late

Every builder is deterministic from its seed."""
import numpy as np

U64 = np.uint64


class World:
    """a bag of named arrays and numbers"""

    def __init__(self, **kw):
        self.__dict__.update(kw)


# ---------------------------------------------------------------------------------------------------------------------------------
# step 2: the models
# ---------------------------------------------------------------------------------------------------------------------------------
def _share(count, total, how="true"):
    """count / total for positive counts, 0.0 otherwise; how: "true" (the script), "recip" (count * (1 / total)), "f32" (a float32
    division): the two wrong ones are what the tie world tells apart from the right one"""
    count = np.asarray(count, dtype=np.int64)
    c = count.astype(np.float64)                               # (int64 -> double: round to nearest, ties to even)
    t = np.float64(float(int(total)))
    out = np.zeros(len(count), dtype=np.float64)
    pos = count > 0
    if not pos.any():
        return out
    if how == "true":
        out[pos] = c[pos] / t
    elif how == "recip":
        out[pos] = c[pos] * (np.float64(1.0) / t)
    elif how == "f32":
        out[pos] = (c[pos].astype(np.float32) / np.float32(t)).astype(np.float64)
    else:
        raise ValueError(how)
    return out


def score_model(pan, meta, pan_sum, meta_sum, how="true"):
    """the script's score of every row: max(pan / pan_sum, meta / meta_sum) over the positive counts in float64, 0.0 otherwise"""
    return np.maximum(_share(pan, pan_sum, how), _share(meta, meta_sum, how))


def key_model(score):
    """flt_score's key of an alive row: the score's bit pattern + 1"""
    return np.asarray(score, dtype=np.float64).view(U64) + U64(1)


def rank_order(score, gone):
    """the alive rows in the script's order: a stable descending sort by score"""
    alive = np.flatnonzero(np.asarray(gone) == 0)
    return alive[np.argsort(-np.asarray(score)[alive], kind="stable")]


def marks_from_order(order, gone, n_scrub):
    """marks = gone, plus the first n_scrub rows of `order` (rank_order's: computed once per world, shared by every cut)"""
    assert 0 <= n_scrub <= len(order)
    out = (np.asarray(gone) != 0).astype(np.uint8)
    out[order[: int(n_scrub)]] = 1
    return out


def joint_model(pan, meta, gone, pan_sum, meta_sum, n_scrub, how="true"):
    """sk_filter_joint: marks = gone, plus the first n_scrub alive rows of the stable descending sort"""
    gone = np.asarray(gone, dtype=np.uint8)
    return marks_from_order(rank_order(score_model(pan, meta, pan_sum, meta_sum, how), gone), gone, n_scrub)


def classes_model(pan, meta, gone, pan_sum, meta_sum, n_scrub):
    """sk_filter_classes_joint with the sums handed in: (class bytes, kept per entry of n_scrub)"""
    gone = np.asarray(gone, dtype=np.uint8)
    return classes_from_order(rank_order(score_model(pan, meta, pan_sum, meta_sum), gone), gone, n_scrub)


def classes_from_order(order, gone, n_scrub):
    cl = np.zeros(len(gone), dtype=np.uint8)
    kept = []
    for k in n_scrub:
        keep = np.zeros(len(gone), dtype=bool)
        keep[order[int(k):]] = True
        cl += keep.astype(np.uint8)
        kept.append(int(keep.sum()))
    return cl, np.array(kept, dtype=np.uint64)


def script_n_scrub(min_fraction, all_kmers, drug_scrubbed, n_alive):
    """the rows the script's joint loop takes off the top (scripts/kmer_scrub_filter.py, joint_scrub)"""
    num, k = float(drug_scrubbed), 0
    while k < n_alive and (1 - ((num + 1) / float(all_kmers))) > min_fraction:
        num += 1.0
        k += 1
    return k


# ---------------------------------------------------------------------------------------------------------------------------------
# step 2: the tie world
# ---------------------------------------------------------------------------------------------------------------------------------
def tie_forms(k, S):
    """the two forms of one score, (pan = 3k of 3S) and (meta = k of S), under the three divisions: {how: (pan form, meta form)}"""
    out = {}
    for how in ("true", "recip", "f32"):
        out[how] = (float(_share([3 * k], 3 * S, how)[0]), float(_share([k], S, how)[0]))
    return out


def tie_ok(k, S):
    f = tie_forms(k, S)
    return f["true"][0] == f["true"][1] and f["recip"][0] != f["recip"][1] and f["f32"][0] != f["f32"][1]


def tie_params(seed=1, nk=3, group=1000):
    """(S, [k descending]): found by search, never taken on faith -- every k ties under true division and splits under the other two,
    and the meta forms of all groups leave room for a positive balancing row (group // 2 + 1 rows of k each stay below S)"""
    rng = np.random.default_rng(seed)
    start = [1777, 1501, 333]
    for j in range(64):
        S = 1000003 + 999983 * j
        ks = []
        for k in start + [int(x) for x in rng.integers(100, 5000, 200)]:
            if k not in ks and tie_ok(k, S):
                ks.append(k)
            if len(ks) == nk:
                break
        if len(ks) == nk and sum(ks) * (group // 2 + 1) < S:
            return S, sorted(ks, reverse=True)
    raise AssertionError("no tie parameters found")


def _tie_rows(S, ks, group, seed, p_gone, extra_top):
    """rows in a shuffled order: per k a group of `group` rows in both forms; the first alive row of a group (in row order) has the
    form that a reciprocal multiply ranks lower and the last alive row the form it ranks higher, so that a cut one row into a group
    or one row before its end tells the two divisions apart as well as a cut in its middle does"""
    rng = np.random.default_rng(seed)
    n = group * len(ks) + extra_top
    kk = np.concatenate([np.full(extra_top, 0, dtype=np.int64)] + [np.full(group, k, dtype=np.int64) for k in ks])
    grp = np.concatenate([np.full(extra_top, -1, dtype=np.int64)] + [np.full(group, g, dtype=np.int64) for g in range(len(ks))])
    form = (np.arange(n) % 2).astype(np.int64)                 # 0: (pan = 3k, meta = 0); 1: (pan = 0, meta = k)
    perm = rng.permutation(n)
    kk, grp = kk[perm], grp[perm]
    form = form[rng.permutation(n)]
    gone = (rng.random(n) < p_gone).astype(np.uint8)
    gone[grp < 0] = 0
    for g, k in enumerate(ks):
        f = tie_forms(k, S)["recip"]
        low, high = (0, 1) if f[0] < f[1] else (1, 0)
        rows = np.flatnonzero((grp == g) & (gone == 0))
        form[rows[0]], form[rows[-1]] = low, high
    pan = np.where(form == 0, 3 * kk, 0).astype(np.int64)
    meta = np.where(form == 1, kk, 0).astype(np.int64)
    return pan, meta, gone, grp, form


def _tie_groups(grp, gone, nk, first_rank):
    """[(a, b)]: group g holds the ranks a .. b - 1 of the alive rows"""
    out, a = [], first_rank
    for g in range(nk):
        size = int(((grp == g) & (gone == 0)).sum())
        out.append((a, a + size))
        a += size
    return out


def tie_cuts(groups, n_alive):
    """(inside, edge): n_scrub values strictly inside a tie group -- one row into it, a third, half, one row before its end -- and
    those at its first row and one past its last"""
    inside, edge = [], []
    for a, b in groups:
        inside += [a + 1, a + (b - a) // 3, (a + b) // 2, b - 1]
        edge += [a, b] + ([b + 1] if b + 1 <= n_alive else [])
    return sorted(set(inside)), sorted(set(edge) - set(inside))


def tie_world(seed=7, group=1000, p_gone=0.07):
    """the primitive route's tie world: sums (3S, S) are handed to sk_filter_joint as they are"""
    S, ks = tie_params(group=group)
    pan, meta, gone, grp, form = _tie_rows(S, ks, group, seed, p_gone, 0)
    groups = _tie_groups(grp, gone, len(ks), 0)
    inside, edge = tie_cuts(groups, int((gone == 0).sum()))
    return World(S=S, ks=ks, pan=pan, meta=meta, gone=gone, grp=grp, form=form, pan_sum=3 * S, meta_sum=S, groups=groups,
                 inside=inside, edge=edge)


TABLE_RUNS = [(False, 0.6), (False, 0.2), (True, 0.3), (True, 0.45)]      # (drug column, -m): every cut lies inside a tie group


def tie_table(seed=8, group=1000, drug=False):
    """the program route's tie world: one balancing row (the first of the table, and of the ranking) makes the TRUE column sums
    3S and S; with drug, a drug column marks about 3 % of the tie rows.  text: the count table; rows as the table lists them"""
    S, ks = tie_params(group=group)
    pan, meta, gone, grp, form = _tie_rows(S, ks, group, seed, 0.03 if drug else 0.0, 1)
    top = int(np.flatnonzero(grp < 0)[0])
    meta[top] = S - int(meta.sum())
    pan[top] = 3 * S - int(pan.sum())
    assert meta[top] > 0 and pan[top] > 0 and int(pan.sum()) == 3 * int(meta.sum()) == 3 * S
    rng = np.random.default_rng(seed + 1000)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    kmers = []
    seen = set()
    while len(kmers) < len(pan):
        k = acgt[rng.integers(0, 4, 31)].tobytes()
        if k not in seen:
            seen.add(k)
            kmers.append(k)
    head = b"#kmer\treference_count\tpangenome_count\tmetagenome_count" + (b"\tdrug_count\n" if drug else b"\n")
    text = head + b"".join(b"%s\t1\t%d\t%d" % (kmers[i], pan[i], meta[i]) + (b"\t%d\n" % gone[i] if drug else b"\n") for i in range(len(pan)))
    groups = _tie_groups(grp, gone, len(ks), 1)
    return World(S=S, ks=ks, pan=pan, meta=meta, gone=gone, grp=grp, form=form, pan_sum=3 * S, meta_sum=S, groups=groups, kmers=kmers,
                 text=text, all_kmers=len(pan), drug_scrubbed=int(gone.sum()))


# ---------------------------------------------------------------------------------------------------------------------------------
# step 2: ladders and single-purpose worlds (each: counts, the column sum to hand in, and a row order that is not the rank order)
# ---------------------------------------------------------------------------------------------------------------------------------
def _two_columns(counts, seed, both):
    """rows in a shuffled order; both: every value twice, once through pan and once through meta (the sums are equal)"""
    rng = np.random.default_rng(seed)
    counts = np.asarray(counts, dtype=np.int64)
    if both:
        pan = np.concatenate([counts, np.zeros(len(counts), dtype=np.int64)])
        meta = np.concatenate([np.zeros(len(counts), dtype=np.int64), counts])
    else:
        pick = rng.random(len(counts)) < 0.5
        pan, meta = np.where(pick, counts, 0), np.where(pick, 0, counts)
    perm = rng.permutation(len(pan))
    return pan[perm].astype(np.int64), meta[perm].astype(np.int64)


def ulp_ladder(seed=11, steps=512):
    """scores exactly one ulp apart: (2^52 + j) / 2^53 = 0.5 + j * 2^-53 for j < steps; every value twice, through either column"""
    counts = (1 << 52) + np.arange(steps, dtype=np.int64)
    pan, meta = _two_columns(counts, seed, True)
    return World(pan=pan, meta=meta, pan_sum=1 << 53, meta_sum=1 << 53, counts=counts)


def digit_ladder(p, seed=12):
    """keys that differ in the byte radix pass p (2 .. 7) looks at and nowhere above it: counts 2^52 + (d << 8 (7 - p)), d = 0 .. 255,
    of 2^53"""
    assert 2 <= p <= 7
    counts = (1 << 52) + (np.arange(256, dtype=np.int64) << np.int64(8 * (7 - p)))
    pan, meta = _two_columns(counts, seed + p, False)
    return World(pan=pan, meta=meta, pan_sum=1 << 53, meta_sum=1 << 53, counts=counts, p=p)


def nibble_ladder(seed=13):
    """pass 1: the sixteen values of the mantissa's top four bits"""
    counts = (1 << 52) + (np.arange(16, dtype=np.int64) << np.int64(48))
    pan, meta = _two_columns(counts, seed, False)
    return World(pan=pan, meta=meta, pan_sum=1 << 53, meta_sum=1 << 53, counts=counts)


def exponent_ladder(seed=14):
    """passes 0 and 1: counts 2^e, e = 0 .. 62, of 2^62 -- the scores 2^-62 .. 1.0 differ in the exponent alone"""
    counts = np.int64(1) << np.arange(63, dtype=np.int64)
    pan, meta = _two_columns(counts, seed, False)
    return World(pan=pan, meta=meta, pan_sum=1 << 62, meta_sum=1 << 62, counts=counts)


def one_world(seed=15):
    """a score of exactly 1.0 (count == sum) next to (2^53 - 1) / 2^53, whose key carries through thirteen F digits into 1.0's
    bit pattern; each value through both columns and twice"""
    top = 1 << 53
    counts = np.array([top, top - 1, top - 2, top, top - 1, 1, top >> 1], dtype=np.int64)
    pan, meta = _two_columns(counts, seed, True)
    return World(pan=pan, meta=meta, pan_sum=top, meta_sum=top, counts=counts)


def zero_world(seed=16, n=700):
    """alive rows of score 0 -- both counts zero, or negative (-2^31 and -1 among them), or one of each -- among rows with a score
    and rows that are gone: the zero rows rank last, in row order"""
    rng = np.random.default_rng(seed)
    pan = rng.integers(1, 50, n).astype(np.int64)
    meta = rng.integers(1, 900, n).astype(np.int64)
    kind = rng.integers(0, 6, n)
    pan[kind == 1], meta[kind == 1] = 0, 0
    pan[kind == 2], meta[kind == 2] = -(1 << 31), -1
    pan[kind == 3], meta[kind == 3] = -1, 0
    pan[kind == 4], meta[kind == 4] = 0, -(1 << 31)
    gone = (rng.random(n) < 0.1).astype(np.uint8)
    zero = (pan <= 0) & (meta <= 0) & (gone == 0)
    return World(pan=pan, meta=meta, gone=gone, pan_sum=int(pan[pan > 0].sum()), meta_sum=int(meta[meta > 0].sum()), zero=zero)


BIG_EQUAL = [((1 << 53), (1 << 53) + 1), ((1 << 53) + 3, (1 << 53) + 4), ((1 << 63) - 512, (1 << 63) - 1),
             ((1 << 60) + 1, (1 << 60) + 127), ((1 << 62) - 255, (1 << 62) - 1)]
# neighbours that stay apart: 2^53 + 3 lies half way between two doubles and goes UP to the even one, so it leaves 2^53 + 2 behind
# (a conversion that truncates would join them, and part them from 2^53 + 4)
BIG_APART = [((1 << 53) + 2, (1 << 53) + 3), ((1 << 53) + 1, (1 << 53) + 2), ((1 << 63) - 1025, (1 << 63) - 512)]


def bigint_world(seed=17, copies=3):
    """counts above 2^53 of a sum of 2^63 - 1: unequal integers that are one double tie and go in row order"""
    vals = sorted({v for pair in BIG_EQUAL + BIG_APART for v in pair})
    counts = np.array(vals * copies, dtype=np.int64)
    pan, meta = _two_columns(counts, seed, False)
    return World(pan=pan, meta=meta, pan_sum=(1 << 63) - 1, meta_sum=(1 << 63) - 1, counts=counts)


FLT_CHUNK = 4096
FLT_THREADS = 256


def eq_scan_world(seed=18):
    """257 * 4096 + 1 rows: 258 chunks, so every thread of flt_eq_scan sums two chunk counts (per = 2); one tie run covers rows
    6000 .. 13999 (chunks 1 to 3: the shares of threads 0 and 1) and the last row, the only one of chunk 257"""
    n = 257 * FLT_CHUNK + 1
    rng = np.random.default_rng(seed)
    pan = rng.integers(1, 1000, n).astype(np.int64)
    pan[pan == 500] = 501
    meta = np.zeros(n, dtype=np.int64)
    pan[6000:14000] = 500
    pan[n - 1] = 500
    gone = np.zeros(n, dtype=np.uint8)
    gone[6000:14000:5] = 1
    above = int(((pan > 500) & (gone == 0)).sum())
    run = int(((pan == 500) & (gone == 0)).sum())
    return World(pan=pan, meta=meta, gone=gone, pan_sum=int(pan.sum()), meta_sum=1, above=above, run=run, n=n)


def hist_column(seed=19, top=2060):
    """every value 0 .. top with its own multiplicity, and negatives: the column max is `top`"""
    rng = np.random.default_rng(seed)
    mult = rng.integers(1, 6, top + 1)
    col = np.concatenate([np.repeat(np.arange(top + 1, dtype=np.int64), mult), -rng.integers(1, 1 << 31, 300).astype(np.int64)])
    return col[rng.permutation(len(col))]


def hist_model(col, lo, nbins):
    col = np.asarray(col, dtype=np.int64)
    pos = col[(col > 0) & (col >= lo)]
    return np.bincount(np.minimum(pos - lo, nbins), minlength=nbins + 1).astype(U64)


# ---------------------------------------------------------------------------------------------------------------------------------
# step 4: the hash, the probe, the segments
# ---------------------------------------------------------------------------------------------------------------------------------
COV_MIX_MULTIPLIERS = (0xFF51AFD7ED558CCD, 0xC4CEB9FE1A85EC53)
COV_MIX_SHIFT = 33


def cov_mix(x):
    """sk_cover.hip's cov_mix on uint64 arrays"""
    x = np.atleast_1d(np.asarray(x, dtype=U64)).copy()
    s = U64(COV_MIX_SHIFT)
    x ^= x >> s
    x *= U64(COV_MIX_MULTIPLIERS[0])
    x ^= x >> s
    x *= U64(COV_MIX_MULTIPLIERS[1])
    x ^= x >> s
    return x


def segment_slots(lines, floor=2):
    """the host's segment size: the next power of two >= 2 * lines, at least `floor` (2 per sample; 64 for the recurrence's one set)"""
    c = floor
    while c < 2 * lines:
        c <<= 1
    return c


def probe_walk(keys_in_order, mask):
    """the linear probe of the insert kernels, one key after the other: (home slot per line, final slot per line, steps walked per
    line, whether any walk stepped from the last slot to slot 0).  The order decides who sits where, never which slots are taken."""
    keys = np.asarray(keys_in_order, dtype=U64)
    home = (cov_mix(keys) & U64(mask)).astype(np.int64)
    table, slot, steps, wrapped = {}, [], [], False
    for k, h in zip(keys.tolist(), home.tolist()):
        s, w = h, 0
        while s in table and table[s] != k:
            if s == mask:
                wrapped = True
            s = (s + 1) & mask
            w += 1
            assert w <= mask, "the segment is full"
        table[s] = k
        slot.append(s)
        steps.append(w)
    return home, np.array(slot, dtype=np.int64), np.array(steps, dtype=np.int64), wrapped


def end_keys(seed, count, mask, last, lo=None):
    """`count` distinct keys below 2^62 whose home slot under `mask` is one of the last `last` (or, with lo, one of the first lo)"""
    rng = np.random.default_rng(seed)
    out = np.zeros(0, dtype=U64)
    while len(out) < count:
        cand = rng.integers(0, 1 << 62, 1 << 20, dtype=np.uint64)
        h = cov_mix(cand) & U64(mask)
        pick = h < U64(lo) if lo is not None else h >= U64(mask + 1 - last)
        out = np.unique(np.concatenate([out, cand[pick]]))
    return out[np.random.default_rng(seed + 1).permutation(len(out))[:count]]


SEG_TINY, SEG_A, SEG_B, SEG_C, SEG_EMPTY, SEG_D = range(6)
SEG_LAST = 6                                                   # the crafted keys home in the last 6 slots


def segment_world(seed=21, large=True):
    """samples in segment order:
      0  two lines, two keys that both home in slot 3 of 4
      1  (large) 2048 lines: 1024 keys, each twice, that home in the last 6 of 4096 slots -- one cluster that wraps past slot 0
      2  (large) 1024 lines: the same 1024 key values, once each, in a segment of 2048 slots, where they home in the last 6 too
         (a key's home under a smaller mask is its home's low bits: the values of sample 1 cannot home at a segment's start)
      3  (large) 512 lines: 256 other keys, each twice, that home in the first 16 of 1024 slots -- where a walk that left sample 2's
         segment would land
      4  no line
      5  200 ordinary keys, some three times
    lines in a shuffled order; cls (1 .. 3, one per (sample, key) pair) and totals (class c <=> total above the first c of
    THRESHOLDS) for the calls that want them"""
    rng = np.random.default_rng(seed)
    tiny = end_keys(seed + 1, 2, 3, 1)
    keys, sample = [tiny], [np.full(2, SEG_TINY)]
    if large:
        a = end_keys(seed + 2, 1024, 4095, SEG_LAST)
        c = end_keys(seed + 3, 256, 1023, None, lo=16)
        keys += [a, a, a, c, c]
        sample += [np.full(2048, SEG_A), np.full(1024, SEG_B), np.full(512, SEG_C)]
    d = rng.integers(0, 1 << 62, 200, dtype=np.uint64)
    keys += [d, d[:50], d[:50]]
    sample += [np.full(300, SEG_D)]
    keys, sample = np.concatenate(keys).astype(U64), np.concatenate(sample).astype(np.uint32)
    cls_of = {}
    cls = np.zeros(len(keys), dtype=np.uint8)
    for i, pair in enumerate(zip(sample.tolist(), keys.tolist())):
        if pair not in cls_of:
            cls_of[pair] = int(rng.integers(1, 4))
        cls[i] = cls_of[pair]
    perm = rng.permutation(len(keys))
    keys, sample, cls = keys[perm], sample[perm], cls[perm]
    totals = np.array([0, 5, 9, 20], dtype=np.uint32)[cls]
    return World(keys=keys, sample=sample, cls=cls, totals=totals, nsamples=6, large=large)


THRESHOLDS = [0, 6, 10]


def recurrence_world(seed=23, large=True):
    """one shared set: (large) 2048 lines over 4 samples, 1024 keys that home in the last 6 of the set's 4096 slots; (small) two
    lines, two keys that home in slot 63 of the smallest set, 64 slots"""
    rng = np.random.default_rng(seed)
    if large:
        k = end_keys(seed + 2, 1024, 4095, SEG_LAST)
        keys = np.concatenate([k, k])
        sample = rng.integers(0, 4, len(keys)).astype(np.uint32)
        perm = rng.permutation(len(keys))
        return World(keys=keys[perm], sample=sample[perm], nsamples=4, mask=4095)
    return World(keys=end_keys(seed + 4, 2, 63, 1), sample=np.array([1, 0], dtype=np.uint32), nsamples=3, mask=63)


# ---------------------------------------------------------------------------------------------------------------------------------
# step 4: first sightings
# ---------------------------------------------------------------------------------------------------------------------------------
def first_seen_model(ids, sample, nsamples):
    """sk_first_seen_count by the script's rule: every line counts for its sample; an id counts once, for the sample of its first
    line"""
    uniq, total = np.zeros(nsamples, dtype=U64), np.zeros(nsamples, dtype=U64)
    seen = set()
    for i, s in zip(np.asarray(ids).tolist(), np.asarray(sample).tolist()):
        total[s] += U64(1)
        if i not in seen:
            seen.add(i)
            uniq[s] += U64(1)
    return uniq, total


GENERAL_SAMPLES = [b"s", b"s1", b"s11", b"s1A"]


def general_hits(seed=31, lines=200_000, clean=0.55):
    """a hit list that is clean (A/C/G/T 31-mers) for `clean` of its lines and ragged after: the k-mer text then starts with a digit
    or a letter that a longer sample name ends with, so that two (sample, k-mer) pairs join to one string ("s" + "11ACG" =
    "s1" + "1ACG" = "s11" + "ACG"; "s1" + "AACG" = "s1A" + "ACG").  Returns (text, rows): rows = [(sample, hits PE1, hits PE2,
    k-mer text)] of the hit lines in file order"""
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    pool = [acgt[rng.integers(0, 4, 31)].tobytes() for _ in range(20_000)]
    words = [acgt[rng.integers(0, 4, int(rng.integers(3, 29)))].tobytes() for _ in range(3_000)]
    split = {b"s11": [(b"s", b"11"), (b"s1", b"1"), (b"s11", b"")], b"s1A": [(b"s", b"1A"), (b"s1", b"A"), (b"s1A", b"")]}
    nclean = int(lines * clean)
    smp = rng.integers(0, 4, lines)
    a, c = rng.integers(0, 4, lines), rng.integers(0, 3, lines)
    pick = rng.integers(0, len(pool), lines)
    wpick = rng.integers(0, len(words), lines)
    how = rng.integers(0, 6, lines)
    rows, out = [], []
    for i in range(lines):
        if i < nclean:
            s, k = GENERAL_SAMPLES[smp[i]], pool[pick[i]]
        else:
            s, lead = split[(b"s11", b"s1A")[how[i] & 1]][how[i] // 2]
            k = lead + words[wpick[i]]
        rows.append((s, int(a[i]), int(c[i]), k))
        out.append(b"reads/%s\t%d\t%d\t%d\t%d\t%s\n" % (s, a[i], rng.integers(0, 3), c[i], rng.integers(0, 2), k))
    for j, s in enumerate(GENERAL_SAMPLES):
        out.append(b"#reads/%s\ttotal_kmer_evaluated\t%d\n#reads/%s\ttotal_reads_evaluated\t%d\n#reads/%s\ttotal_genome_kmers\t5000000\n"
                   b"#reads/%s\ttotal_genome_informative_kmers\t30000\n" % (s, 10 ** 9 + j, s, 10 ** 7 + j, s, s))
    return b"".join(out), rows, nclean


def script_counts(rows, min_hits=1):
    """scripts/coverage_depth.py, count_passed_kmers: {sample: [unique or -1, total]} in the order of the samples' first passing
    line -- a global `seen` set of sample + k-mer text, the first line's sample takes the credit"""
    seen, cover, depth = set(), {}, {}
    for s, a, c, k in rows:
        if a + c > min_hits:
            if s + k not in seen:
                seen.add(s + k)
                cover[s] = cover.get(s, 0) + 1
            depth[s] = depth.get(s, 0) + 1
    return {s: [cover.get(s, -1), n] for s, n in depth.items()}


def table_counts(stdout):
    """a main coverage table -> {metagenome: [unique, total]} in its order"""
    out = {}
    for ln in stdout.split(b"\n")[1:]:
        if ln:
            f = ln.split(b"\t")
            out[f[5]] = [int(f[8]), int(f[9])]
    return out
