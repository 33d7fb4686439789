/* sk_host_rarefaction.c -- the host side of rarefaction (include/strainer_kmer.h has the rule in full): the list parser, the draw, a
 * pair's class, the fold of one strain's and target's hit lines on the host, and the table writer.  Nothing here touches a device;
 * the accumulator's kernels (sk_covacc.hip) compute the same draw and the same class.  The file needs the public header only, so
 * tests/native/rarefaction_check.c includes it and runs it as a stand-alone program. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../include/strainer_kmer.h"

uint32_t skh_rarefaction_draw(uint64_t pair, uint32_t seed)
{
    uint32_t x = (uint32_t)pair ^ ((uint32_t)(pair >> 32) * 0x9E3779B9u) ^ seed;
    x ^= x >> 16; x *= 0x85EBCA6Bu;
    x ^= x >> 13; x *= 0xC2B2AE35u;
    x ^= x >> 16;
    return x;
}

uint32_t skh_rarefaction_class(const skh_rarefaction *r, uint64_t pair)
{
    uint32_t q, c = 0;
    uint64_t u;
    if (!r) return 0;
    u = skh_rarefaction_draw(pair, r->seed);
    for (q = 0; q < r->n && q < SK_COVACC_RAREFACTION_MAX; q++) c += u < r->T[q] ? 1u : 0u;
    return c;
}

/* one field of the list: a plain decimal number (digits, at most one '.', an optional exponent), 0 < f <= 1 */
static int rar_field(const char *s, size_t len, uint64_t *T)
{
    char buf[40], *end;
    size_t i, digits = 0, dots = 0;
    double f;
    if (!len || len >= sizeof buf) return SK_E_ARG;
    memcpy(buf, s, len); buf[len] = 0;
    for (i = 0; i < len && buf[i] != 'e' && buf[i] != 'E'; i++) {
        if (buf[i] >= '0' && buf[i] <= '9') digits++;
        else if (buf[i] == '.' && !dots) dots++;
        else return SK_E_ARG;
    }
    if (!digits) return SK_E_ARG;
    if (i < len) {                                             /* the exponent: e[+-]digits */
        size_t ed = 0;
        i++;
        if (i < len && (buf[i] == '+' || buf[i] == '-')) i++;
        for (; i < len; i++, ed++) if (buf[i] < '0' || buf[i] > '9') return SK_E_ARG;
        if (!ed) return SK_E_ARG;
    }
    f = strtod(buf, &end);
    if (*end || !(f > 0.0) || !(f <= 1.0)) return SK_E_ARG;    /* (an underflow to 0 is refused here too) */
    *T = (uint64_t)(f * 4294967296.0);                         /* a double times 2^32 is exact; the cast floors */
    return SK_OK;
}

int skh_rarefaction_parse(const char *list, uint32_t seed, skh_rarefaction *out)
{
    const char *p = list ? list : SKH_RAREFACTION_DEFAULT;
    if (!out) return SK_E_ARG;
    memset(out, 0, sizeof *out);
    out->seed = seed;
    for (;;) {
        const char *e = strchr(p, ',');
        const size_t len = e ? (size_t)(e - p) : strlen(p);
        uint64_t T;
        if (out->n == SK_COVACC_RAREFACTION_MAX || rar_field(p, len, &T) != SK_OK) { memset(out, 0, sizeof *out); return SK_E_ARG; }
        if (out->n && T >= out->T[out->n - 1]) { memset(out, 0, sizeof *out); return SK_E_ARG; }   /* not descending, or two equal T */
        out->T[out->n] = T;
        memcpy(out->text[out->n], p, len);
        out->n++;
        if (!e) break;
        p = e + 1;
    }
    return SK_OK;
}

int skh_rarefaction_fold(const skh_rarefaction *r, int64_t min_kmer_hits, uint32_t nrows, const uint64_t *pair, const uint32_t *row,
                         const uint32_t *total_hits, uint64_t n, uint64_t first_pair, uint64_t npairs,
                         uint64_t *out_pairs, uint64_t *out_unique, uint64_t *out_total)
{
    uint64_t lines[SK_COVACC_RAREFACTION_MAX + 1], rows[SK_COVACC_RAREFACTION_MAX + 1], prs[SK_COVACC_RAREFACTION_MAX + 1], i, u, t, p;
    unsigned char *best;                                       /* every row's highest class */
    uint32_t q;
    if (!r || !r->n || r->n > SK_COVACC_RAREFACTION_MAX || !out_pairs || !out_unique || !out_total || (n && (!pair || !row || !total_hits)))
        return SK_E_ARG;
    for (i = 0; i < n; i++) if (row[i] >= nrows) return SK_E_ARG;
    if (!(best = (unsigned char *)calloc(nrows ? nrows : 1u, 1))) return SK_E_NOMEM;
    memset(lines, 0, sizeof lines); memset(rows, 0, sizeof rows); memset(prs, 0, sizeof prs);
    for (i = 0; i < n; i++) {
        uint32_t c;
        if (!((int64_t)total_hits[i] > min_kmer_hits)) continue;
        c = skh_rarefaction_class(r, pair[i]);
        lines[c]++;
        if (c > best[row[i]]) best[row[i]] = (unsigned char)c;
    }
    for (i = 0; i < nrows; i++) rows[best[i]]++;
    for (i = 0; i < npairs; i++) prs[skh_rarefaction_class(r, first_pair + i)]++;
    free(best);
    for (q = r->n, u = t = p = 0; q-- > 0u; ) {                /* class c counts for the subsamples 0 .. c - 1: suffix sums */
        t += lines[q + 1]; u += rows[q + 1]; p += prs[q + 1];
        out_total[q] = t; out_unique[q] = u; out_pairs[q] = p;
    }
    return SK_OK;
}

int skh_rarefaction_write(FILE *f, const skh_rarefaction *r, const char *strain, const char *metagenome,
                          const uint64_t *pairs, const uint64_t *unique, const uint64_t *total)
{
    uint32_t q;
    if (!f || !r) return SK_E_ARG;
    if (!metagenome) {
        if (fprintf(f, "%smetagenome\tfraction\tpairs\tunique_kmers\ttotal_hits\n", strain ? "strain_name\t" : "") < 0) return SK_E_OPEN;
        return SK_OK;
    }
    if (!pairs || !unique || !total) return SK_E_ARG;
    for (q = 0; q < r->n && q < SK_COVACC_RAREFACTION_MAX; q++) {
        if (strain && fprintf(f, "%s\t", strain) < 0) return SK_E_OPEN;
        if (fprintf(f, "%s\t%s\t%llu\t%llu\t%llu\n", metagenome, r->text[q], (unsigned long long)pairs[q],
                    (unsigned long long)unique[q], (unsigned long long)total[q]) < 0) return SK_E_OPEN;
    }
    return SK_OK;
}
