/* hash_craft.c -- TEST INFRASTRUCTURE (tests/_craft.py builds it with gcc as a shared object and loads it with ctypes).
 *
 * Brute-force search, from a seeded generator, for keys whose place in the library's hash-addressed structures is chosen
 * instead of left to chance: packed 31-mers by their first table slot, byte-string keys by their first index slot, a 16-mer by
 * its key in the partitioned pipeline's bins.  Every hash is the library's own (sk_common.h): nothing of one is restated here,
 * so a hash that changes takes this helper along.  And a model of a table filled by linear probing from given first slots,
 * which says how far a key's walk goes and whether it runs over the last slot into slot 0.
 */
#include <stdint.h>
#include <string.h>

#include "../../strainer2_amd/csrc/sk_common.h"

/* xorshift64: the search's generator (any stream of bits will do; no key depends on more than "seeded") */
static uint64_t hc_next(uint64_t *s)
{
    uint64_t x = *s;
    x ^= x << 13; x ^= x >> 7; x ^= x << 17;
    return *s = x;
}

static uint64_t hc_seed(uint64_t seed)
{
    uint64_t s = seed ^ 0x5DEECE66DULL;
    int i;
    if (!s) s = 1;
    for (i = 0; i < 8; i++) (void)hc_next(&s);
    return s;
}

/* the precondition of tests/_synth.py's U windows on a canonical key w: w > revcomp(w), and revcomp(w) holds a T behind the
 * first base where the two differ; *t_mask gets the positions (bit i = base i of revcomp(w)) where a U may stand */
static int hc_u_reachable(uint64_t w, uint32_t *t_mask)
{
    const uint64_t r = sk_revcomp62(w);
    uint32_t m = 0;
    int i, d = -1;
    if (w <= r) return 0;
    for (i = 0; i < 31; i++) {
        const uint32_t bw = (uint32_t)(w >> (2 * (30 - i))) & 3u, br = (uint32_t)(r >> (2 * (30 - i))) & 3u;
        if (d < 0) { if (bw != br) d = i; continue; }
        if (br == 3u) m |= 1u << i;
    }
    if (t_mask) *t_mask = m;
    return m != 0;
}

/* n distinct canonical packed 31-mers (k >= revcomp(k)) whose first slot in a table of 1 << lg slots lies in [lo, hi];
 * need_u: they also satisfy hc_u_reachable.  Returns the number of candidates tried (0: gave up after max_tries). */
uint64_t hc_craft_keys(uint64_t seed, uint32_t lg, uint32_t lo, uint32_t hi, int need_u, uint64_t *out, uint32_t n, uint64_t max_tries)
{
    const uint32_t mask = (uint32_t)(((uint64_t)1 << lg) - 1);
    uint64_t s = hc_seed(seed), tries = 0;
    uint32_t got = 0, j;
    while (got < n) {
        uint64_t k;
        uint32_t slot;
        if (tries++ >= max_tries) return 0;
        k = hc_next(&s) & SK_KMASK62;
        slot = sk_slot0(sk_khash(k), mask);                /* (the cheap question first: one candidate in 2^20 gets past it) */
        if (slot < lo || slot > hi) continue;
        if (k < sk_revcomp62(k)) continue;
        if (need_u && !hc_u_reachable(k, NULL)) continue;
        for (j = 0; j < got && out[j] != k; j++) { }
        if (j == got) out[got++] = k;
    }
    return tries;
}

/* first slots of packed keys in a table of 1 << lg slots */
void hc_slot0(const uint64_t *keys, uint32_t n, uint32_t lg, uint32_t *out)
{
    const uint32_t mask = (uint32_t)(((uint64_t)1 << lg) - 1);
    uint32_t i;
    for (i = 0; i < n; i++) out[i] = sk_slot0(sk_khash(keys[i]), mask);
}

/* U-window data of canonical keys: ok[i] = hc_u_reachable, t_mask[i] = where the U may stand */
void hc_u_info(const uint64_t *keys, uint32_t n, uint8_t *ok, uint32_t *t_mask)
{
    uint32_t i;
    for (i = 0; i < n; i++) { t_mask[i] = 0; ok[i] = (uint8_t)hc_u_reachable(keys[i], &t_mask[i]); }
}

/* ---- byte-string keys ---------------------------------------------------------------------------------------------------- */
/* the orientation the library stores a 31-byte window in: the window itself or its reverse complement by the reference's
 * complement map, whichever is larger as signed chars (the window on ties) */
static void hc_wide_canon(const char *u, char *o)
{
    static signed char comp[256];
    static int have = 0;
    int i, sign = 0;
    if (!have) { sk_fill_complement(comp); have = 1; }
    for (i = 0; i < 31 && sign == 0; i++) {
        const signed char f = (signed char)u[i], r = comp[(uint8_t)u[30 - i]];
        sign = (f > r) - (r > f);
    }
    if (sign >= 0) memcpy(o, u, 31);
    else for (i = 0; i < 31; i++) o[30 - i] = (char)comp[(uint8_t)u[i]];
}

/* first index slots of 31-byte keys (32 bytes apart) under wmask */
void hc_wide_slot0(const char *keys32, uint32_t n, uint32_t wmask, uint32_t *out)
{
    uint32_t i;
    for (i = 0; i < n; i++) out[i] = sk_hash_wide(keys32 + (size_t)i * 32) & wmask;
}

/* n distinct byte-string keys (32 bytes apart, NUL behind each): A/C/G/T with one to three letters of `letters` (IUPAC codes
 * whose complement is an IUPAC code again), in the stored orientation, whose first index slot under wmask lies in [lo, hi] */
uint64_t hc_craft_wide(uint64_t seed, uint32_t wmask, uint32_t lo, uint32_t hi, const char *letters, char *out32, uint32_t n, uint64_t max_tries)
{
    const uint32_t nl = (uint32_t)strlen(letters);
    uint64_t s = hc_seed(seed), tries = 0;
    uint32_t got = 0, j;
    while (got < n) {
        char u[32], o[32];
        uint64_t x;
        uint32_t slot, i, m;
        if (tries++ >= max_tries) return 0;
        x = hc_next(&s);
        for (i = 0; i < 31; i++) u[i] = "ACGT"[(x >> (2 * i)) & 3u];
        x = hc_next(&s);
        m = 1u + (uint32_t)(x % 3u);
        for (i = 0; i < m; i++) { x = hc_next(&s); u[(x >> 8) % 31u] = letters[(x >> 40) % nl]; }
        hc_wide_canon(u, o);
        o[31] = 0;
        slot = sk_hash_wide(o) & wmask;
        if (slot < lo || slot > hi) continue;
        for (j = 0; j < got && memcmp(out32 + (size_t)j * 32, o, 31); j++) { }
        if (j == got) memcpy(out32 + (size_t)got++ * 32, o, 32);
    }
    return tries;
}

/* ---- the partitioned pipeline's bins ---------------------------------------------------------------------------------------- */
/* a packed 16-mer (first base in the top bits, as a chunk of the stream is packed) whose bin key -- of its canonical form, as
 * sk_bin takes it -- is `want_key`; *part gets its partition.  Returns the tries (0: none found). */
uint64_t hc_craft_bin16(uint64_t seed, uint32_t want_key, uint32_t *out16, uint32_t *part, uint64_t max_tries)
{
    uint64_t s = hc_seed(seed), tries = 0;
    for (;;) {
        uint32_t f, r, h;
        if (tries++ >= max_tries) return 0;
        f = (uint32_t)(hc_next(&s) >> 16);
        r = sk_revcomp16(f);
        h = sk_grid3_hash(sk_gmix(f < r ? f : r));
        if (sk_grid3_key(h) != want_key) continue;
        *out16 = f;
        *part = sk_grid3_part(h);
        return tries;
    }
}

void hc_bin16_of(uint32_t f, uint32_t *key, uint32_t *part)
{
    const uint32_t r = sk_revcomp16(f), h = sk_grid3_hash(sk_gmix(f < r ? f : r));
    *key = sk_grid3_key(h);
    *part = sk_grid3_part(h);
}

/* ---- the model ---------------------------------------------------------------------------------------------------------------- */
/* keys 0..n-1 with first slots slot0[] go, in this order, into `table` (nslots words, all zero: 0 = empty, else key + 1) by
 * linear probing; final[i] = where key i came to rest.  The SET of occupied slots does not depend on the order. */
void hc_model_insert(const uint32_t *slot0, uint32_t n, uint32_t nslots, uint32_t *table, uint32_t *final)
{
    uint32_t i;
    for (i = 0; i < n; i++) {
        uint32_t s = slot0[i];
        while (table[s]) s = s + 1 == nslots ? 0 : s + 1;
        table[s] = i + 1;
        final[i] = s;
    }
}

/* the walk of query q from q_slot0[q]: it ends at the slot that holds key q_id[q] (-1: an absent key) or at the first empty
 * slot.  len[q] = slots looked at, that last one included; wrapped[q] = the walk stepped from the last slot to slot 0. */
void hc_model_walk(const uint32_t *table, uint32_t nslots, const uint32_t *q_slot0, const int64_t *q_id, uint32_t nq,
                   uint32_t *len, uint8_t *wrapped)
{
    uint32_t q;
    for (q = 0; q < nq; q++) {
        uint32_t s = q_slot0[q], l = 1;
        uint8_t w = 0;
        while (table[s] && (int64_t)table[s] - 1 != q_id[q] && l <= nslots) {
            if (s + 1 == nslots) { s = 0; w = 1; } else s++;
            l++;
        }
        len[q] = l;
        wrapped[q] = w;
    }
}
