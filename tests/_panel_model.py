"""The panel's shared k-mers (sk_union_share, strain_detect -S --panel-share; include/strainer_kmer.h has the rule) in Python:
the model every panel-share test compares against.  The reference has no counterpart.

canonical(w)              a 31-base word's key text: the larger of the word and its reverse complement
share(keys, inf, ..)      per member a set of keys and its informative subset -> the three matrices, by plain set operations
table(names, m0, m1, m2)  the table's bytes
table_from_files(..)      the table of a -S panel from its genome files and -a lists"""
import gzip
import os

import numpy as np

import strainer2_amd as sk

HEADER = b"strain_a\tstrain_b\tkmers_a\tinformative_a\tshared_kmers\tinformative_a_in_b\tinformative_both\n"
_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def canonical(w: bytes) -> bytes:
    return max(w, w.translate(_COMP)[::-1])


def share(keys_a, inf_a, keys_b=None, inf_b=None):
    """keys_a[i]: member i's set of keys, inf_a[i]: the subset that is informative in it (keys_b None: b is a).
    -> (m0, m1, m2) uint64 [len(a), len(b)]: keys both hold, keys informative in i that j holds, keys informative in both"""
    if keys_b is None:
        keys_b, inf_b = keys_a, inf_a
    keys_a, keys_b = [set(k) for k in keys_a], [set(k) for k in keys_b]
    inf_a, inf_b = [set(k) for k in inf_a], [set(k) for k in inf_b]
    for k, i in list(zip(keys_a, inf_a)) + list(zip(keys_b, inf_b)):
        assert i <= k, "an informative key is a key of the member"
    m = np.zeros((3, len(keys_a), len(keys_b)), dtype=np.uint64)
    for i in range(len(keys_a)):
        for j in range(len(keys_b)):
            m[0, i, j] = len(keys_a[i] & keys_b[j])
            m[1, i, j] = len(inf_a[i] & keys_b[j])
            m[2, i, j] = len(inf_a[i] & inf_b[j])
    return m[0], m[1], m[2]


def strain_name(hits_file_name):
    """the coverage tables' strain name: the file's basename without a trailing '<any>kmer_hits<any>gz'"""
    n = os.path.basename(hits_file_name)
    return n[:-13] if len(n) >= 13 and n[-12:-3] == "kmer_hits" and n[-2:] == "gz" else n


def table(names, m0, m1, m2):
    """one line per ordered pair, a outer and b inner, a == b included"""
    out = [HEADER]
    for a, na in enumerate(names):
        for b, nb in enumerate(names):
            out.append(b"%s\t%s\t%d\t%d\t%d\t%d\t%d\n" % (na.encode(), nb.encode(), int(m0[a, a]), int(m1[a, a]), int(m0[a, b]), int(m1[a, b]),
                                                         int(m2[a, b])))
    return b"".join(out)


def keys_of_genome(path):
    ks = sk.Keyset.from_file(str(path))
    try:
        return set(ks.keys())
    finally:
        ks.close()


def keys_of_list(path):
    """the k-mers a -a list names as keys: one a line, exactly 31 upper-case letters ('#' lines are comments, a line of another
    length or with a lower-case letter flags nothing; plain or .gz)"""
    raw = open(path, "rb").read()
    if raw[:2] == b"\x1f\x8b":
        raw = gzip.decompress(raw)
    return {canonical(ln) for ln in raw.split(b"\n") if len(ln) == 31 and not ln.startswith(b"#") and ln == ln.upper()}


def table_from_files(strains):
    """strains: [(genome file, -a list, -o file)] in the -S file's order.  A k-mer of the list that the genome does not hold is no
    row of the strain and counts nowhere."""
    keys = [keys_of_genome(g) for g, _, _ in strains]
    inf = [keys_of_list(a) & k for (_, a, _), k in zip(strains, keys)]
    return table([strain_name(o) for _, _, o in strains], *share(keys, inf))
