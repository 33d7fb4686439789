"""Small deterministic input generators shared by the tests."""
import json
import os
import random

COMP = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")


def revcomp(s: bytes) -> bytes:
    return s.translate(COMP)[::-1]


def rand_dna(rng: random.Random, n: int) -> bytes:
    return bytes(rng.choice(b"ACGT") for _ in range(n))


def fuzz_stream(rng: random.Random, strain: bytes, nreads: int, junk=b"NnRYKMUu-. acgt\rX*", p_junk=0.02,
                min_len=0, max_len=200) -> bytes:
    """Reads drawn from `strain` (either strand), random reads, random junk bytes, any case."""
    out = []
    for _ in range(nreads):
        ln = rng.randint(min_len, max_len)
        if rng.random() < 0.6 and len(strain) > ln + 1:
            a = rng.randrange(0, len(strain) - ln)
            r = bytearray(strain[a:a + ln])
            if rng.random() < 0.5:
                r = bytearray(revcomp(bytes(r)))
        else:
            r = bytearray(rand_dna(rng, ln))
        for i in range(len(r)):
            x = rng.random()
            if x < p_junk:
                r[i] = rng.choice(junk)
            elif x < p_junk * 2:
                r[i] = rng.choice(b"ACGT")
            elif x < p_junk * 3:
                r[i] = r[i] | 0x20
        out.append(bytes(r))
    return b"\n".join(out) + b"\n"


def oracle_fuzz_world(seed: int, d) -> list:
    """Random FASTA/FASTQ soup (junk bytes, CRLF, blank lines, multi-line, '>'/'@'/'+' traps) for one kmer_scrub_count
    job, written into directory `d`; returns the job's argv (paths relative to `d`).  What the reference printed for
    it is in tests/golden/fuzz_facts.json (tests/golden/make_fuzz_facts.py)."""
    rng = random.Random(seed)
    strain = rand_dna(rng, 3000)
    lines = [b">s1 c\n"]
    for i in range(0, len(strain), 70):
        lines.append(strain[i:i + 70] + b"\n")
    with open(os.path.join(d, "strain.fa"), "wb") as f:
        f.write(b"".join(lines))
    files = []
    for fi in range(3):
        recs = fuzz_stream(rng, strain, 200, p_junk=0.01, min_len=0, max_len=160).split(b"\n")[:-1]
        body = bytearray()
        for i, r in enumerate(recs):
            style = rng.randrange(5)
            r = r.replace(b"\r", b"A")
            if style == 0:
                body += b">r%d\n" % i + r + b"\n"
            elif style == 1:
                w = rng.choice([20, 50, 61])
                body += b">r%d desc\r\n" % i + b"\r\n".join(r[j:j + w] for j in range(0, len(r), w)) + b"\r\n"
            elif style == 2:
                q = bytes(rng.choice(b"@+>IJK#") for _ in r)
                body += b"@q%d\n" % i + r + b"\n+\n" + q + b"\n"
            elif style == 3:
                body += b">r%d\n\n" % i + r[:len(r) // 2] + b"\n\n" + r[len(r) // 2:] + b"\n"
            else:
                body += b"junk before header\n>r%d\t x\n" % i + r + b"\n"
        name = "m%d.fx" % fi
        with open(os.path.join(d, name), "wb") as f:
            f.write(bytes(body))
        files.append(name)
    with open(os.path.join(d, "A.txt"), "w") as f:
        f.write(files[0] + "\n")
    with open(os.path.join(d, "B.txt"), "w") as f:
        f.write("\n".join(files[1:]) + "\n")
    return ["-r", "strain.fa", "-A", "A.txt", "-B", "B.txt"]


def reader_soup(seed: int, d):
    """A file thrown together from header, sequence, '+', quality and blank lines in every order -- equal and unequal
    quality lengths, wrapped sequences, CR line ends, '@' and '>' opening quality lines, a missing last newline, plain
    or gzipped, perhaps cut short -- written into directory `d`; returns (the strain its sequence comes from, the path)."""
    import gzip
    rng = random.Random(9000 + seed)
    nl = rng.choice([b"\n", b"\n", b"\r\n"])
    strain = rand_dna(rng, 3000)
    out = []
    for _ in range(rng.randrange(1, 400)):
        kind = rng.random()
        n = rng.choice([0, 1, 2, 30, 31, 40, 150, 151])
        a = rng.randrange(0, len(strain) - n)
        seq = strain[a:a + n]                              # (pieces of the strain: which bytes count as sequence shows in the table)
        if seed % 3 == 0:                                  # every third soup is mostly one-line FASTA: the parser's other whole-record shortcut
            kind = 0.6 if kind < 0.6 else kind
        if kind < 0.55:                                    # a well-formed four-line record (now and then not quite)
            q = bytes(rng.choice(b"FFFF:,#@>+I") for _ in range(n if rng.random() < 0.9 else rng.choice([0, 1, max(0, n - 1), n + 1])))
            out += [b"@r%d some text" % len(out), seq, b"+" + (b"r" if rng.random() < 0.2 else b""), q]
        elif kind < 0.62:                                  # FASTA, the sequence on one line, '>' or '@' header
            out += [(b">" if rng.random() < 0.8 else b"@") + b"o%d len=%d" % (len(out), n), seq]
        elif kind < 0.7:                                   # FASTA, wrapped
            out += [b">c%d" % len(out)] + [seq[i:i + 60] for i in range(0, n, 60)]
        elif kind < 0.8:                                   # FASTQ with wrapped sequence and quality
            q = b"I" * n
            out += [b"@w%d" % len(out)] + [seq[i:i + 50] for i in range(0, n, 50)] + [b"+"] + [q[i:i + 70] for i in range(0, n, 70)]
        else:                                              # loose lines
            out.append(rng.choice([b"", b"+", b"@", b">", b"\r", seq, b"@" + seq, b"+" + seq, b" ", b"\t@x"]))
    text = nl.join(out) + (nl if rng.random() < 0.8 else b"")
    if rng.random() < 0.3:
        text = text[:rng.randrange(len(text) + 1)]
    path = os.path.join(d, "soup.fq.gz" if seed % 2 else "soup.fq")
    with open(path, "wb") as f:
        f.write(gzip.compress(text, 6, mtime=0) if seed % 2 else text)
    return strain, path


def soup_job(strain: bytes, soup: str, d) -> list:
    """the kmer_scrub_count job that scans a reader soup against its strain (-A and -B both name the soup)"""
    with open(os.path.join(d, "strain.fa"), "wb") as f:
        f.write(b">s\n" + strain + b"\n")
    with open(os.path.join(d, "A.txt"), "w") as f:
        f.write(soup + "\n")
    return ["-r", os.path.join(d, "strain.fa"), "-A", os.path.join(d, "A.txt"), "-B", os.path.join(d, "A.txt")]



def two_expansions_strain(golden, tmp_path):
    """the 9.2 Mbp strain of tests/golden/make_two_expansions_facts.py, written again by that script's own function; None if this
    numpy draws another sequence than the one the reference saw (the facts carry the file's md5)"""
    import hashlib
    import importlib.util
    facts = json.load(open(os.path.join(golden, "two_expansions_facts.json")))
    spec = importlib.util.spec_from_file_location("make_two_expansions_facts", os.path.join(golden, "make_two_expansions_facts.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    path = str(tmp_path / "strain.fa")
    mod.write_strain(path)
    if hashlib.md5(open(path, "rb").read()).hexdigest() != facts["strain"]["md5"]:
        return None, facts
    return path, facts


# ---- TALLY worlds (tests/test_tally_forms_gpu.py, tests/test_tally_ref.py) ------------------------------------------
def mutate(rng: random.Random, seq: bytes, rate: float) -> bytes:
    b = bytearray(seq)
    for i in range(len(b)):
        if rng.random() < rate:
            b[i] = rng.choice(b"ACGT")
    return bytes(b)


def u_window(rng: random.Random, strain: bytes):
    """(a 31-byte window holding U or u that hits `strain` for certain, the strain k-mer it hits), or None.  A strain
    k-mer w that is its own canonical form (w > revcomp(w)) is reverse-complemented and a T behind the first base where
    the two differ becomes U: the window's reverse complement is then w again and the larger of the two, so the key
    looked up is pure A/C/G/T -- the byte-string kernel's one way to a table hit on such a window"""
    for _ in range(200):
        a = rng.randrange(len(strain) - 30)
        w = strain[a:a + 31].upper()
        u = u_window_of(rng, w)
        if u:
            return u, w
    return None


def u_window_of(rng: random.Random, w: bytes):
    """u_window for one given k-mer w (31 upper-case bytes), in the table or not: the window holding U or u through which the
    byte-string kernel looks w up, or None where w has none (a byte that is no base, w <= revcomp(w), or no T behind the first
    base where the two differ)"""
    if len(w) != 31 or set(w) - set(b"ACGT"):
        return None
    r = revcomp(w)
    if w <= r:
        return None
    d = next(i for i in range(31) if w[i] != r[i])
    ts = [i for i in range(d + 1, 31) if r[i] == ord("T")]
    if not ts:
        return None
    i = rng.choice(ts)
    return r[:i] + rng.choice([b"U", b"u"]) + r[i + 1:]


def tally_strains(rng: random.Random, kind: int, n: int, sizes=(400, 3000, 12000)) -> list:
    """n strains that share keys: the same strain again, diverged copies, unrelated ones, the other strand of a part,
    a repeated segment (with an N)"""
    base = rand_dna(rng, rng.choice(sizes))
    out = []
    for s in range(n):
        pick = (s + kind) % 5
        if pick == 0:
            g = base
        elif pick == 1:
            g = mutate(rng, base, rng.choice([0.002, 0.01, 0.05]))
        elif pick == 2:
            g = rand_dna(rng, rng.choice([200, 5000, 9000]))
        elif pick == 3:
            g = revcomp(base[len(base) // 3:]) + rand_dna(rng, 500)
        else:
            cut = len(base) // 2
            g = base[:cut] + base[cut // 2:cut] + base[cut:]
            g = g[:50] + b"N" + g[51:]
        out.append(g)
    return out


def tally_reads(rng: random.Random, strains: list, nreads: int, junk: bool) -> tuple:
    """(records, the strain k-mers that U windows were made from).  Pieces of the strains (either strand, some
    mutated), random reads, reads shorter than k and empty ones, lower case; junk: also U windows that hit for
    certain (u_window), and IUPAC letters, U and '\\r' sprinkled in.  Without junk the bytes are A/C/G/T, N and lower case."""
    recs, uk = [], []
    for _ in range(nreads):
        x = rng.random()
        if x < 0.04:
            recs.append(b"")
            continue
        if x < 0.1:
            recs.append(rand_dna(rng, rng.randrange(1, 31)))
            continue
        ln = rng.choice([31, 32, 47, 64, 100, 150, 151, 250, 700])
        g = strains[rng.randrange(len(strains))]
        if rng.random() < 0.75 and len(g) > ln:
            a = rng.randrange(len(g) - ln)
            seq = mutate(rng, g[a:a + ln], rng.choice([0.0, 0.0, 0.01, 0.05]))
            if rng.random() < 0.5:
                seq = revcomp(seq)
        else:
            seq = rand_dna(rng, ln)
        if junk and rng.random() < 0.15:
            u = u_window(rng, g)
            if u:
                cut = rng.randrange(len(seq) + 1)
                seq = seq[:cut] + u[0] + seq[cut:]
                uk.append(u[1])
        b = bytearray(seq)
        if rng.random() < 0.1:
            for _ in range(rng.randrange(1, 3)):
                b[rng.randrange(len(b))] = rng.choice(b"RYKMSWBDHVUu\r" if junk else b"Nn")
        if rng.random() < 0.05:
            b = b.lower()
        recs.append(bytes(b))
    return recs, uk


# ---- byte-alphabet worlds (tests/test_byte_alphabet_gpu.py, tests/test_byte_alphabet_host.py) -----------------------
# Every decision the scan makes about a byte (base, hard breaker, or a byte for the byte-string kernel) is a function of the byte:
# these worlds hand it all 256 values, at every position of the 16-byte chunk and next to every kind of neighbour.
ALPHABET_READ = 93                     # bases of a read: 46, the foreign byte, 46 -- 16 windows end before it, 31 hold it, 16 start behind it
ALPHABET_AT = 46
# World B's representative bytes, one per hazard: the separator and NUL, N, bases and U in both cases, IUPAC letters, symbols of the
# complement map, '*' ('\n' + bit 5), bytes one bit from a letter or from NUL, the ends of the letter ranges, 0x7F, and bytes at or
# above 0x80 that equal '\n', 'A', 'N' or nothing in their low seven bits
ALPHABET_PAIR_SET = bytes([0x00, 0x0A]) + b"NnAcGtUuRK.-*" + bytes([0x01, 0x21, 0x40, 0x60, 0x5B, 0x7B, 0x49, 0x51, 0x7F,
                                                                   0x80, 0x8A, 0xC1, 0xCE, 0xE3, 0xFF])


def _alphabet_piece(rng: random.Random, strain: bytes, want=None) -> bytes:
    """ALPHABET_READ bases of the strain, either strand; want: the base at ALPHABET_AT must be this one"""
    while True:
        a = rng.randrange(len(strain) - ALPHABET_READ + 1)
        r = strain[a:a + ALPHABET_READ]
        if rng.random() < 0.5:
            r = revcomp(r)
        if want is None or r[ALPHABET_AT] == want:
            return r


def _alphabet_place(rng: random.Random, recs: list, off: int, read: bytes, mod16: int) -> int:
    """append `read` behind a filler record of 1..16 random bases (too short for a window) sized so that the read's byte
    ALPHABET_AT lands on a stream offset that is mod16 modulo 16; returns the offset behind the read's newline"""
    f = (mod16 - off - 1 - ALPHABET_AT) % 16 or 16
    recs += [rand_dna(rng, f), read]
    return off + f + 1 + len(read) + 1


def alphabet_world_a(seed=4601, phases=range(16), leave_out=b""):
    """World A: one foreign byte, every value, every chunk phase.  Returns (strain, records, cases): the strain is 600 random
    bases; for every byte b (but those in leave_out) and every phase j of `phases` one read of 93 strain bases (either strand)
    with b at index 46, placed so that b's offset in b"\\n".join(records) + b"\\n" is j modulo 16; cases[i] = (b, j, index of
    the read in records, the base b replaced).  The U and u reads replace a T, so that some of their windows can hit; at the even
    phases a base replaces itself (either case: all windows hit), and a byte that equals a base in its low seven bits and for the
    case bit replaces that base (taken for the base, it would make 31 windows hit that must not)."""
    rng = random.Random(seed)
    strain = rand_dna(rng, 600)
    recs, cases, off = [], [], 0
    for b in range(256):
        if b in leave_out:
            continue
        for j in phases:
            want = None
            if b in b"Uu":
                want = ord("T")
            elif j % 2 == 0 and b & 0x5F in b"ACGT":                # a base, or a byte that equals one in its low seven bits with the case folded
                want = b & 0x5F
            r = bytearray(_alphabet_piece(rng, strain, want))
            was = r[ALPHABET_AT]
            r[ALPHABET_AT] = b
            off = _alphabet_place(rng, recs, off, bytes(r), j)
            cases.append((b, j, len(recs) - 1, was))
    return strain, recs, cases


def alphabet_world_b(seed=4602):
    """World B: two foreign bytes side by side, every ordered pair of ALPHABET_PAIR_SET at indices 46 and 47 of a read, the first
    on every byte of its 32-bit word (the fourth: the second byte opens the next word, for every fourth pair the next chunk).
    Returns (strain, records, cases) with cases[i] = (b1, b2, offset of b1 modulo 16)."""
    rng = random.Random(seed)
    strain = rand_dna(rng, 600)
    recs, cases, off, n = [], [], 0, 0
    for b1 in ALPHABET_PAIR_SET:
        for b2 in ALPHABET_PAIR_SET:
            for w in range(4):
                r = bytearray(_alphabet_piece(rng, strain))
                r[ALPHABET_AT], r[ALPHABET_AT + 1] = b1, b2
                mod16 = w + 4 * (n % 4)
                n += w == 3
                off = _alphabet_place(rng, recs, off, bytes(r), mod16)
                cases.append((b1, b2, mod16))
    return strain, recs, cases


def alphabet_world_c(seed=4603):
    """World C, the strain's side: for every byte b but NUL and the separator one strain record of 45 random bases, b, 45 random
    bases.  Returns [(b, record)]."""
    rng = random.Random(seed)
    return [(b, rand_dna(rng, 45) + bytes([b]) + rand_dna(rng, 45)) for b in range(1, 256) if b != 0x0A]


def alphabet_world_c_reads(records, reverse: bool, cs=range(256)) -> bytes:
    """World C's reads: every record of alphabet_world_c with its byte 45 replaced by every c of `cs`; reverse: the record
    reversed and its A/C/G/T complemented first (45 is its own mirror image in 91 bytes).  One read a line, record after
    record, c ascending."""
    import numpy as np
    cs = np.array(list(cs), dtype=np.uint8)
    out = np.empty((len(records), len(cs), 92), dtype=np.uint8)
    for i, (_b, rec) in enumerate(records):
        out[i, :, :91] = np.frombuffer(revcomp(rec) if reverse else rec, dtype=np.uint8)
    out[:, :, 45] = cs
    out[:, :, 91] = 0x0A
    return out.tobytes()
