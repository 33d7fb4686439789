/* sk_host_cov.c -- host side of the coverage/depth table: the drop-in for reference
 * scripts/coverage_depth.py (step 4 of test/example.sh).
 *
 * The script reads strain_detect's hit list (<metagenome> <hits PE1> <informative PE1> <hits PE2>
 * <informative PE2> <k-mer>, plus four "#<metagenome> <name> <value>" trailer lines per metagenome) and
 * prints, per metagenome, how many hit lines pass the read filter, how many different k-mers they name
 * and the two ratios to the strain's informative k-mer count.  Here the lines are parsed into
 * (sample, packed k-mer) pairs and both counts are taken on the device (sk_distinct_count,
 * sk_cover.hip); this file keeps the script's dictionaries (their insertion order is the order of the
 * printed rows) and its number formatting.
 */
#define _GNU_SOURCE
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <zlib.h>
#include "../../include/strainer_kmer.h"
#include "sk_common.h"
#include "sk_pyfmt.h"
#include "sk_sweep.h"
#include "sk_internal.h"

/* ------------------------------------------------------------------ a small insertion-ordered name table */
typedef struct {
    char   **name; uint32_t n, cap;
    /* per sample, the script's dictionaries; have_* = key present */
    int64_t *kmer_eval, *read_eval, *g_total, *g_inf;
    uint8_t *have_eval, *have_reads, *have_total, *have_inf, *in_depth;
    uint32_t *slot; uint32_t nslot;
} names;

static uint64_t name_hash(const char *s, size_t len)
{
    uint64_t h = 1469598103934665603ull;
    size_t i;
    for (i = 0; i < len; i++) h = (h ^ (unsigned char)s[i]) * 1099511628211ull;
    return h;
}

static int64_t name_get(names *t, const char *s, size_t len)
{
    uint32_t i, g;
    if (!t->slot) {
        t->nslot = 256;
        if (!(t->slot = calloc(t->nslot, sizeof *t->slot))) return -1;
    }
    i = (uint32_t)name_hash(s, len) & (t->nslot - 1);
    while ((g = t->slot[i]) != 0) {
        if (strlen(t->name[g - 1]) == len && !memcmp(t->name[g - 1], s, len)) return g - 1;
        i = (i + 1) & (t->nslot - 1);
    }
    if (t->n == t->cap) {
        const uint32_t cap = t->cap ? t->cap * 2 : 64;
#define GROW(field) do { void *p_ = realloc(t->field, (size_t)cap * sizeof *t->field); if (!p_) return -1; t->field = p_; } while (0)
        GROW(name); GROW(kmer_eval); GROW(read_eval); GROW(g_total); GROW(g_inf);
        GROW(have_eval); GROW(have_reads); GROW(have_total); GROW(have_inf); GROW(in_depth);
#undef GROW
        t->cap = cap;
    }
    g = t->n++;
    if (!(t->name[g] = malloc(len + 1))) return -1;
    memcpy(t->name[g], s, len);
    t->name[g][len] = 0;
    t->kmer_eval[g] = t->read_eval[g] = t->g_total[g] = t->g_inf[g] = 0;
    t->have_eval[g] = t->have_reads[g] = t->have_total[g] = t->have_inf[g] = t->in_depth[g] = 0;
    t->slot[i] = g + 1;
    if (t->n * 2 > t->nslot) {                        /* rebuild at four times the size */
        uint32_t ns = t->nslot * 4, *s2 = calloc(ns, sizeof *s2), k;
        if (!s2) return -1;
        for (k = 0; k < t->n; k++) {
            uint32_t j = (uint32_t)name_hash(t->name[k], strlen(t->name[k])) & (ns - 1);
            while (s2[j]) j = (j + 1) & (ns - 1);
            s2[j] = k + 1;
        }
        free(t->slot);
        t->slot = s2; t->nslot = ns;
    }
    return g;
}

static void names_free(names *t)
{
    uint32_t i;
    for (i = 0; i < t->n; i++) free(t->name[i]);
    free(t->name); free(t->kmer_eval); free(t->read_eval); free(t->g_total); free(t->g_inf);
    free(t->have_eval); free(t->have_reads); free(t->have_total); free(t->have_inf); free(t->in_depth); free(t->slot);
    memset(t, 0, sizeof *t);
}

static const char *base_of(const char *s, const char *end)
{
    const char *p = end;
    while (p > s && p[-1] != '/') p--;
    return p;
}

/* ------------------------------------------------------------------ the hit list */
typedef struct {
    names     smp;
    uint64_t *key; uint32_t *sample; uint64_t n, cap;   /* hit lines that passed the read filter */
    uint32_t *depth_order; uint32_t ndepth;            /* samples in the order their first passing line came */
    uint32_t *eval_order; uint32_t neval;              /* samples in the order their total_kmer_evaluated line came */
    names     text;                                    /* general mode: the script's unique strings -> ids */
    uint32_t *gid, *gsample; uint64_t gn, gcap;        /* general mode: per passing line, in file order: joined-string number, sample */
    int       general;
    size_t    klen;                                    /* k-mer field length seen so far (0 = none yet) */
    uint64_t *given_u, *given_t; uint32_t ngiven; int given;   /* counts handed in per sample (skc_add_counts) instead of hits */
    uint64_t **reg_u, **reg_t; uint32_t nreg_s, reg_bins;      /* ... and per sample and region (skc_add_region_counts): reg_bins each, or NULL */
    uint64_t **sp_n, *sp_deep; uint32_t nsp_s, sp_bins;        /* the depth spectrum per sample: n[1..D], n[>D] (sp_bins = D + 1 each, or NULL) and hits[>D] */
    uint64_t *rc_hist, *rc_pairs; uint32_t *rc_smp, rc_T;      /* recurrence handed in (skc_add_recurrence_counts): n[0..T] (entry 0 unused), shared[T x T] or NULL,
                                                                  both by the caller's sample ordinals; rc_smp[ordinal] = the sample */
    /* thresholds (th_nt = 0: off): the list; every hit line above t[0], whatever the main filter does with it, with its pair's total;
     * th_bad: a k-mer field among them that is no A/C/G/T word of the one length; per sample the numbers handed in (th_nt each, or NULL) */
    int64_t   th_t[SK_COVACC_THRESHOLDS_MAX]; uint32_t th_nt;
    uint64_t *th_key; uint32_t *th_sample, *th_tot; uint64_t th_n, th_cap; size_t th_klen; int th_bad;
    uint64_t **th_u, **th_tt; uint32_t nth_s;
    /* the scrub sweep (cl_F = 0: off): the fractions' texts and the sets' sizes; per sample the numbers per fraction (cl_F each, or NULL) */
    uint32_t  cl_F; char cl_frac[SK_SCRUB_SWEEP_MAX][SKW_TEXT_MAX]; uint64_t cl_size[SK_SCRUB_SWEEP_MAX];
    uint64_t **cl_u, **cl_t; uint32_t ncl_s;
} hitlist;

enum { COV_OK = 0, COV_OPEN, COV_FIELDS, COV_INT, COV_NOMEM };

/* the script keys its uniqueness test by <sample name><k-mer text> joined without a separator (:88-93).
 * With k-mer fields of one length made of A/C/G/T -- all strain_detect ever writes -- that is the pair
 * (sample, packed k-mer), counted on the device.  Any other k-mer text (ragged lengths, other letters)
 * switches the file to "general" mode, because two different pairs may then join to the same string: the
 * joined strings are numbered here (a dictionary of texts, as the parse needs anyway) and the device credits
 * every string to the sample of the first line that shows it (sk_first_seen_count), which is what the
 * script's global "seen" dictionary does. */
static int general_count(hitlist *h, uint32_t g, const char *ktext, size_t klen)
{
    const char *sn = h->smp.name[g];
    const size_t sl = strlen(sn);
    char *u = malloc(sl + klen + 1);
    int64_t id;
    if (!u) return COV_NOMEM;
    memcpy(u, sn, sl); memcpy(u + sl, ktext, klen);
    id = name_get(&h->text, u, sl + klen);            /* number of the joined string */
    free(u);
    if (id < 0) return COV_NOMEM;
    if (h->gn == h->gcap) {
        const uint64_t cap = h->gcap ? h->gcap * 2 : 1u << 12;
        uint32_t *a = realloc(h->gid, cap * sizeof *a), *b;
        if (!a) return COV_NOMEM;
        h->gid = a;
        if (!(b = realloc(h->gsample, cap * sizeof *b))) return COV_NOMEM;
        h->gsample = b;
        h->gcap = cap;
    }
    h->gid[h->gn] = (uint32_t)id;
    h->gsample[h->gn++] = g;
    return COV_OK;
}

static int to_general(hitlist *h)
{
    uint64_t i;
    char buf[32];
    for (i = 0; i < h->n; i++) {                      /* replay what was packed so far, in file order */
        size_t j;
        int rc;
        for (j = 0; j < h->klen; j++) buf[j] = "ACGT"[(h->key[i] >> (2 * (h->klen - 1 - j))) & 3u];
        if ((rc = general_count(h, h->sample[i], buf, h->klen)) != COV_OK) return rc;
    }
    h->n = 0;
    h->general = 1;
    return COV_OK;
}

/* one hit that passed the read filter: sample = basename of the metagenome, key = packed k-mer or row */
static int64_t cov_sample(hitlist *h, const char *sn, size_t slen)
{
    const int64_t g = name_get(&h->smp, sn, slen);
    if (g >= 0 && !h->smp.in_depth[g]) {
        uint32_t *o = realloc(h->depth_order, ((size_t)h->ndepth + 1) * sizeof *o);
        if (!o) return -1;
        h->depth_order = o;
        o[h->ndepth++] = (uint32_t)g;
        h->smp.in_depth[g] = 1;
    }
    return g;
}

static int cov_push(hitlist *h, uint32_t g, uint64_t key)
{
    if (h->n == h->cap) {
        const uint64_t cap = h->cap ? h->cap * 2 : 1u << 16;
        uint64_t *k2 = realloc(h->key, cap * sizeof *k2);
        uint32_t *s2;
        if (!k2) return COV_NOMEM;
        h->key = k2;
        if (!(s2 = realloc(h->sample, cap * sizeof *s2))) return COV_NOMEM;
        h->sample = s2;
        h->cap = cap;
    }
    h->key[h->n] = key;
    h->sample[h->n++] = g;
    return COV_OK;
}

/* thresholds: how many of the list a pair's total exceeds (0: the line counts at no threshold) */
static uint32_t th_class(const hitlist *h, int64_t total)
{
    uint32_t q, c = 0;
    for (q = 0; q < h->th_nt; q++) c += total > h->th_t[q];
    return c;
}

/* ... and one line of class >= 1: its sample, key and total (totals beyond 32 bits exceed every threshold alike) */
static int th_push(hitlist *h, uint32_t g, uint64_t key, int64_t total)
{
    if (h->th_n == h->th_cap) {
        const uint64_t cap = h->th_cap ? h->th_cap * 2 : 1u << 16;
        uint64_t *k2 = realloc(h->th_key, cap * sizeof *k2);
        uint32_t *s2, *t2;
        if (!k2) return COV_NOMEM;
        h->th_key = k2;
        if (!(s2 = realloc(h->th_sample, cap * sizeof *s2))) return COV_NOMEM;
        h->th_sample = s2;
        if (!(t2 = realloc(h->th_tot, cap * sizeof *t2))) return COV_NOMEM;
        h->th_tot = t2;
        h->th_cap = cap;
    }
    h->th_key[h->th_n] = key;
    h->th_sample[h->th_n] = g;
    h->th_tot[h->th_n++] = total > 0xFFFFFFFFll ? 0xFFFFFFFFu : (uint32_t)total;
    return COV_OK;
}

/* ... of a hit list's text: the k-mer field packed, if it is an A/C/G/T word of the length of all the others; th_bad otherwise */
static int th_push_text(hitlist *h, uint32_t g, const char *ktext, size_t klen, int64_t total)
{
    uint64_t key = 0;
    size_t j;
    int plain = klen >= 1 && klen <= 31 && (h->th_klen == 0 || h->th_klen == klen);
    for (j = 0; plain && j < klen; j++) {
        const unsigned cde = sk_code((uint8_t)ktext[j]);
        if (ktext[j] != "ACGT"[cde]) plain = 0;
        key = (key << 2) | (cde & 3u);
    }
    if (!plain) { h->th_bad = 1; return COV_OK; }
    h->th_klen = klen;
    return th_push(h, g, key, total);
}

static int hit_line(hitlist *h, char *s, size_t len, int64_t min_hits)
{
    char *f[7], *end = s + len, *p;
    int nf = 1;
    uint32_t cls;
    int64_t a, b, c, d, g;
    const char *sn, *kend;
    size_t klen, j;
    uint64_t key = 0;
    f[0] = s;
    for (p = s; p < end; p++)
        if (*p == '\t') { if (nf < 7) f[nf] = p + 1; nf++; }
    if (nf < 6) return COV_FIELDS;
    if (!skp_int(f[1], f[2] - 1, &a) || !skp_int(f[2], f[3] - 1, &b) || !skp_int(f[3], f[4] - 1, &c) || !skp_int(f[4], f[5] - 1, &d))
        return COV_INT;
    cls = th_class(h, a + c);
    if (!(a + c > min_hits)) {                        /* hits of the read pair, informative or not (:83-86) */
        if (!cls) return COV_OK;
        sn = base_of(f[0], f[1] - 1);                 /* (thresholds: a line below the main filter and above t[0]; it names its sample
                                                         and changes nothing else of what the main table is made from) */
        if ((g = name_get(&h->smp, sn, (size_t)(f[1] - 1 - sn))) < 0) return COV_NOMEM;
        kend = nf > 6 ? f[6] - 1 : end;
        return th_push_text(h, (uint32_t)g, f[5], (size_t)(kend - f[5]), a + c);
    }
    sn = base_of(f[0], f[1] - 1);
    if ((g = cov_sample(h, sn, (size_t)(f[1] - 1 - sn))) < 0) return COV_NOMEM;
    kend = nf > 6 ? f[6] - 1 : end;
    klen = (size_t)(kend - f[5]);
    if (cls) { const int rc = th_push_text(h, (uint32_t)g, f[5], klen, a + c); if (rc) return rc; }
    if (!h->general) {
        int plain = klen >= 1 && klen <= 31 && (h->klen == 0 || h->klen == klen);
        for (j = 0; plain && j < klen; j++) {
            const unsigned cde = sk_code((uint8_t)f[5][j]);
            if (f[5][j] != "ACGT"[cde]) plain = 0;     /* upper-case A/C/G/T only */
            key = (key << 2) | (cde & 3u);
        }
        if (plain) h->klen = klen;
        else { int rc = to_general(h); if (rc) return rc; }
    }
    if (h->general) return general_count(h, (uint32_t)g, f[5], klen);
    return cov_push(h, (uint32_t)g, key);
}

/* one trailer value of a sample (:104-116) */
static int cov_trailer(hitlist *h, const char *sn, size_t slen, const char *var, size_t vlen, int64_t v)
{
    const int64_t g = name_get(&h->smp, sn, slen);
    if (g < 0) return COV_NOMEM;
#define IS(word) (vlen == sizeof(word) - 1 && !memcmp(var, word, sizeof(word) - 1))
    if (IS("total_kmer_evaluated")) {
        if (!h->smp.have_eval[g]) {
            uint32_t *o = realloc(h->eval_order, ((size_t)h->neval + 1) * sizeof *o);
            if (!o) return COV_NOMEM;
            h->eval_order = o;
            o[h->neval++] = (uint32_t)g;
        }
        h->smp.kmer_eval[g] = v; h->smp.have_eval[g] = 1;
    }
    else if (IS("total_reads_evaluated")) { h->smp.read_eval[g] = v; h->smp.have_reads[g] = 1; }
    else if (IS("total_genome_kmers")) { h->smp.g_total[g] = v; h->smp.have_total[g] = 1; }
    else if (IS("total_genome_informative_kmers")) { h->smp.g_inf[g] = v; h->smp.have_inf[g] = 1; }
#undef IS
    return COV_OK;
}

/* "#<metagenome>\t<name>\t<value>" (:101-116) */
static int trailer_line(hitlist *h, char *s, size_t len)
{
    char *f[4], *end, *p;
    int nf = 1;
    int64_t v;
    const char *sn;
    while (len && isspace((unsigned char)s[len - 1])) len--;      /* line.rstrip() */
    end = s + len;
    f[0] = s;
    for (p = s; p < end; p++)
        if (*p == '\t') { if (nf < 4) f[nf] = p + 1; nf++; }
    if (nf < 3) return COV_FIELDS;
    sn = base_of(f[0], f[1] - 1);
    if (sn < f[1] - 1 && *sn == '#') sn++;
    if (!skp_int(f[2], nf > 3 ? f[3] - 1 : end, &v)) return COV_INT;
    return cov_trailer(h, sn, (size_t)(f[1] - 1 - sn), f[1], (size_t)(f[2] - 1 - f[1]), v);
}

static int read_hits(hitlist *h, const char *path, int64_t min_hits)
{
    gzFile gz = gzopen(path, "rb");
    size_t cap = 1u << 20, have = 0;
    char *buf;
    int n, rc = COV_OK;
    if (!gz) return COV_OPEN;
    gzbuffer(gz, 1u << 20);
    if (!(buf = malloc(cap))) { gzclose(gz); return COV_NOMEM; }
    for (;;) {
        char *line, *nl, *end;
        if (have == cap) {
            char *b = realloc(buf, cap * 2);
            if (!b) { rc = COV_NOMEM; break; }
            buf = b; cap *= 2;
        }
        n = gzread(gz, buf + have, (unsigned)(cap - have));
        if (n < 0) { rc = COV_OPEN; break; }
        have += (size_t)n;
        end = buf + have;
        line = buf;
        while (line < end && ((nl = memchr(line, '\n', (size_t)(end - line))) != NULL || n == 0)) {
            size_t len = nl ? (size_t)(nl - line) : (size_t)(end - line);
            if (len && line[len - 1] == '\r' && nl) len--;
            rc = (len && line[0] == '#') ? trailer_line(h, line, len) : hit_line(h, line, len, min_hits);
            if (rc) goto out;
            line = nl ? nl + 1 : end;
        }
        have = (size_t)(end - line);
        memmove(buf, line, have);
        if (n == 0) break;
    }
out:
    free(buf);
    gzclose(gz);
    return rc;
}

/* ------------------------------------------------------------------ the program */
static int cov_opt(int argc, char **argv, int *i, const char *shortn, const char *longn, const char **val, FILE *err, int *bad)
{
    const char *a = argv[*i];
    const size_t ll = strlen(longn);
    if (!strcmp(a, shortn) || !strcmp(a, longn)) {
        if (*i + 1 >= argc) { fprintf(err, "coverage_depth: error: argument %s/%s: expected one argument\n", longn, shortn); *bad = 1; return 1; }
        *val = argv[++*i];
        return 1;
    }
    if (!strncmp(a, longn, ll) && a[ll] == '=') { *val = a + ll + 1; return 1; }
    if (!strncmp(a, shortn, 2) && a[2]) { *val = a + 2; return 1; }
    return 0;
}

/* metagenomes that only have trailer lines come after those with passing hits (:121-124); -1: out of memory */
static int cov_order_trailers(hitlist *h)
{
    uint32_t k, s;
    for (k = 0; k < h->neval; k++)
        if (!h->smp.in_depth[s = h->eval_order[k]]) {
            uint32_t *o = realloc(h->depth_order, ((size_t)h->ndepth + 1) * sizeof *o);
            if (!o) return -1;
            h->depth_order = o;
            o[h->ndepth++] = s;
            h->smp.in_depth[s] = 1;
        }
    return 0;
}

/* everything after the hit list is read: trailer-only samples, the counts (device), the table (:121-124,200-271).
 * `kfile` only names the strain.  Returns the exit status. */
static int cov_report(hitlist *h, sk_ctx *ctx, const char *kfile, const char *bfile, FILE *out, FILE *err)
{
    names bg;
    uint64_t *uniq = NULL, *total = NULL;
    char *strain = NULL, *species = NULL, *genus = NULL, *us;
    size_t sl;
    uint32_t s, k;
    int rc, status = 1;
    memset(&bg, 0, sizeof bg);
    if (cov_order_trailers(h)) { fprintf(err, "coverage_depth: out of memory\n"); goto done; }
    if (h->smp.n) {
        if (!(uniq = calloc(h->smp.n, sizeof *uniq)) || !(total = calloc(h->smp.n, sizeof *total))) { fprintf(err, "coverage_depth: out of memory\n"); goto done; }
        if (h->given) {                              /* counted already (strain_detect --coverage-only: on the device, target by target) */
            for (s = 0; s < h->ngiven && s < h->smp.n; s++) { uniq[s] = h->given_u[s]; total[s] = h->given_t[s]; }
        } else if (h->general) {                     /* out-of-domain k-mer text: first sightings of the joined strings */
            rc = sk_first_seen_count(ctx, h->gid, h->gsample, h->gn, h->text.n, h->smp.n, uniq, total);
            if (rc != SK_OK) { fprintf(err, "coverage_depth: %s (%s)\n", sk_strerror(rc), sk_last_error(ctx)); goto done; }
        } else {
            rc = sk_distinct_count(ctx, h->key, h->sample, h->n, h->smp.n, uniq, total);
            if (rc != SK_OK) { fprintf(err, "coverage_depth: %s (%s)\n", sk_strerror(rc), sk_last_error(ctx)); goto done; }
        }
    }
    /* names derived from the file name (:203-213): strip "<any>kmer_hits<any>gz" at the end, split at '_' */
    strain = strdup(base_of(kfile, kfile + strlen(kfile)));
    sl = strlen(strain);
    if (sl >= 13 && !memcmp(strain + sl - 12, "kmer_hits", 9) && !memcmp(strain + sl - 2, "gz", 2)) strain[sl - 13] = 0;
    species = strdup(strain);
    genus = strdup(strain);
    if ((us = strchr(genus, '_')) != NULL) {
        *us = 0;
        if ((us = strchr(species + strlen(genus) + 1, '_')) != NULL) *us = 0;
    }
    if (bfile) {                                     /* :131-140 */
        FILE *bf = fopen(bfile, "r");
        char *line = NULL;
        size_t cap = 0;
        ssize_t n;
        if (!bf) { fprintf(err, "coverage_depth: could not read %s\n", bfile); goto done; }
        while ((n = getline(&line, &cap, bf)) >= 0) {
            while (n > 0 && line[n - 1] == '\n') line[--n] = 0;
            if (name_get(&bg, line, (size_t)n) < 0) { fclose(bf); free(line); goto done; }
        }
        free(line);
        fclose(bf);
    }
    fputs("strain_name\tspecies_name\tgenus_name\tgenome_num_total_kmers\tgenome_num_informative_kmers\tmetagenome\t"
          "num_metagenomic_reads\tnum_metagenome_kmers\tunique_observed_informative_kmers\ttotal_observed_informative_kmers\t"
          "kmer_coverage\tkmer_depth\tkmer_depth_per_20B_kmer\tbackground\n", out);
    for (k = 0; k < h->ndepth; k++) {                /* :227-271 */
        const names *t = &h->smp;
        const char *m;
        int64_t observed, unique, evaluated, reads, gt, gi;
        int in_bg = 0;
        uint32_t j;
        char c1[32], c2[32], c3[32];
        s = h->depth_order[k];
        m = t->name[s];
        observed = (int64_t)total[s];
        /* general mode only: a sample all of whose joined strings were first seen under another sample
         * never enters the script's coverage dictionary and prints the -1 placeholder (:236-243) */
        unique = (h->general && total[s] && !uniq[s]) ? -1 : (int64_t)uniq[s];
        evaluated = t->have_eval[s] ? t->kmer_eval[s] : -1;
        reads = t->have_eval[s] ? (t->have_reads[s] ? t->read_eval[s] : 0) : -1;
        gt = t->have_total[s] ? t->g_total[s] : -1;
        gi = t->have_inf[s] ? t->g_inf[s] : -1;
        if (gi == 0) { fflush(out); fprintf(err, "ZeroDivisionError: float division by zero\n"); goto done; }
        skp_float_str((double)unique / (double)gi, c1);
        skp_float_str((double)observed / (double)gi, c2);
        if (evaluated == 0) strcpy(c3, "0");
        else skp_float_str(((double)observed / (double)gi) * (2000000000 / (double)evaluated), c3);
        for (j = 0; j < bg.n && !in_bg; j++) in_bg = !strcmp(bg.name[j], m);
        fprintf(out, "%s\t%s\t%s\t%lld\t%lld\t%s\t%lld\t%lld\t%lld\t%lld\t%s\t%s\t%s\t%d\n", strain, species, genus, (long long)gt,
                (long long)gi, m, (long long)reads, (long long)evaluated, (long long)unique, (long long)observed, c1, c2, c3, in_bg);
    }
    status = 0;
done:
    fflush(out);
    free(uniq); free(total); free(strain); free(species); free(genus);
    names_free(&bg);
    return status;
}

static void hitlist_free(hitlist *h)
{
    uint32_t s;
    for (s = 0; s < h->nreg_s; s++) { free(h->reg_u[s]); free(h->reg_t[s]); }
    free(h->reg_u); free(h->reg_t);
    for (s = 0; s < h->nsp_s; s++) free(h->sp_n[s]);
    free(h->sp_n); free(h->sp_deep);
    free(h->given_u); free(h->given_t);
    free(h->rc_hist); free(h->rc_pairs); free(h->rc_smp);
    for (s = 0; s < h->nth_s; s++) { free(h->th_u[s]); free(h->th_tt[s]); }
    free(h->th_u); free(h->th_tt); free(h->th_key); free(h->th_sample); free(h->th_tot);
    for (s = 0; s < h->ncl_s; s++) { free(h->cl_u[s]); free(h->cl_t[s]); }
    free(h->cl_u); free(h->cl_t);
    free(h->key); free(h->sample); free(h->depth_order); free(h->eval_order); free(h->gid); free(h->gsample);
    names_free(&h->smp); names_free(&h->text);
    memset(h, 0, sizeof *h);
}

/* ---- the same accumulator fed directly by strain_detect (fused steps 3 -> 4; sk_internal.h) ---- */
struct skc_acc { hitlist h; int64_t min_hits; };

skc_acc *skc_create(int64_t min_hits)
{
    skc_acc *a = calloc(1, sizeof *a);
    if (a) a->min_hits = min_hits;
    return a;
}

void skc_destroy(skc_acc *a) { if (a) { hitlist_free(&a->h); free(a); } }

/* what one hit line of the -o file would contribute: metagenome path, the pair's hit counts of PE1 and PE2
 * (fields 2 and 4), and the k-mer named by its row */
int skc_add_hit(skc_acc *a, const char *metagenome, int64_t hits_pe1, int64_t hits_pe2, uint32_t row)
{
    const char *sn;
    int64_t g;
    if (a->h.th_nt && th_class(&a->h, hits_pe1 + hits_pe2)) {         /* thresholds: the line above t[0], kept with its total */
        sn = base_of(metagenome, metagenome + strlen(metagenome));
        if ((g = name_get(&a->h.smp, sn, strlen(sn))) < 0 || th_push(&a->h, (uint32_t)g, (uint64_t)row, hits_pe1 + hits_pe2) != COV_OK) return -1;
    }
    if (!(hits_pe1 + hits_pe2 > a->min_hits)) return 0;
    sn = base_of(metagenome, metagenome + strlen(metagenome));
    if ((g = cov_sample(&a->h, sn, strlen(sn))) < 0) return -1;
    return cov_push(&a->h, (uint32_t)g, (uint64_t)row) == COV_OK ? 0 : -1;
}

/* a metagenome's two numbers, counted elsewhere: `total` hit lines that passed the read filter, on `unique` distinct rows.  Called
 * where the metagenome's first passing line would have come (before its trailers), so that the order of the table's lines is the
 * script's; an accumulator takes either hits or counts, and a metagenome's counts once (the caller sees to both). */
int skc_add_counts(skc_acc *a, const char *metagenome, uint64_t unique, uint64_t total)
{
    hitlist *h = &a->h;
    const char *sn = base_of(metagenome, metagenome + strlen(metagenome));
    const int64_t g = total ? cov_sample(h, sn, strlen(sn)) : name_get(&h->smp, sn, strlen(sn));
    if (g < 0) return -1;
    h->given = 1;
    if ((uint64_t)g >= h->ngiven) {
        const uint32_t n2 = (uint32_t)g + 16u;
        uint64_t *u2 = realloc(h->given_u, (size_t)n2 * sizeof *u2), *t2;
        if (!u2) return -1;
        h->given_u = u2;
        if (!(t2 = realloc(h->given_t, (size_t)n2 * sizeof *t2))) return -1;
        h->given_t = t2;
        memset(u2 + h->ngiven, 0, (size_t)(n2 - h->ngiven) * sizeof *u2);
        memset(t2 + h->ngiven, 0, (size_t)(n2 - h->ngiven) * sizeof *t2);
        h->ngiven = n2;
    }
    h->given_u[g] += unique; h->given_t[g] += total;
    return 0;
}

int skc_add_trailer(skc_acc *a, const char *metagenome, const char *name, int64_t value)
{
    const char *sn = base_of(metagenome, metagenome + strlen(metagenome));
    return cov_trailer(&a->h, sn, strlen(sn), name, strlen(name), value) == COV_OK ? 0 : -1;
}

int skc_report(skc_acc *a, sk_ctx *ctx, const char *hits_file_name, FILE *out, FILE *err)
{
    return cov_report(&a->h, ctx, hits_file_name, NULL, out, err);
}

/* ---- the same numbers per region of the strain's genome (strain_detect --coverage-regions; include/strainer_kmer.h has the rule) ---- */
static int reg_room(hitlist *h, uint32_t g, uint32_t nbins)
{
    if (h->reg_bins && h->reg_bins != nbins) return -1;
    h->reg_bins = nbins;
    if (g >= h->nreg_s) {
        const uint32_t n2 = g + 16u;
        uint64_t **u2 = realloc(h->reg_u, (size_t)n2 * sizeof *u2), **t2;
        if (!u2) return -1;
        h->reg_u = u2;
        memset(u2 + h->nreg_s, 0, (size_t)(n2 - h->nreg_s) * sizeof *u2);
        if (!(t2 = realloc(h->reg_t, (size_t)n2 * sizeof *t2))) return -1;       /* (reg_u is longer than nreg_s says: harmless) */
        h->reg_t = t2;
        memset(t2 + h->nreg_s, 0, (size_t)(n2 - h->nreg_s) * sizeof *t2);
        h->nreg_s = n2;
    }
    if (!h->reg_u[g] && !(h->reg_u[g] = calloc(nbins ? nbins : 1, sizeof **h->reg_u))) return -1;
    if (!h->reg_t[g] && !(h->reg_t[g] = calloc(nbins ? nbins : 1, sizeof **h->reg_t))) return -1;
    return 0;
}

/* a metagenome's numbers per region, counted elsewhere (nbins = the strain's regions + 1, "unplaced" last): called next to
 * skc_add_counts, after it, so that the sample exists */
int skc_add_region_counts(skc_acc *a, const char *metagenome, const uint64_t *unique, const uint64_t *total, uint32_t nbins)
{
    hitlist *h = &a->h;
    const char *sn = base_of(metagenome, metagenome + strlen(metagenome));
    const int64_t g = name_get(&h->smp, sn, strlen(sn));
    uint32_t r;
    if (g < 0 || reg_room(h, (uint32_t)g, nbins)) return -1;
    for (r = 0; r < nbins; r++) { h->reg_u[g][r] += unique[r]; h->reg_t[g][r] += total[r]; }
    return 0;
}

static int cmp_u64(const void *x, const void *y)
{
    const uint64_t a = *(const uint64_t *)x, b = *(const uint64_t *)y;
    return a < b ? -1 : a > b;
}

/* The table: one line per metagenome of the main table (in its order: call this after skc_report) and region with an informative
 * row.  row_region[row] < nbins for the strain's nrows rows, reg_inf[r] = informative rows of region r.  An accumulator that was
 * fed hits folds its (sample, row) list here; one that was fed counts prints what skc_add_region_counts left. */
int skc_report_regions(skc_acc *a, const char *hits_file_name, const skh_regions *rg, const uint32_t *row_region, uint32_t nrows,
                       const uint64_t *reg_inf, FILE *out, FILE *err)
{
    hitlist *h = &a->h;
    const uint32_t nbins = rg->n + 1u;
    char *strain;
    size_t sl;
    uint32_t k, s, r;
    if (cov_order_trailers(h)) { fprintf(err, "coverage_depth: out of memory\n"); return 1; }      /* (what cov_report did already, when it ran) */
    if (!h->given && h->n) {
        uint64_t *v = malloc((size_t)h->n * sizeof *v), i, j;
        if (!v) { fprintf(err, "coverage_depth: out of memory\n"); return 1; }
        for (i = 0; i < h->n; i++) v[i] = ((uint64_t)h->sample[i] << 32) | (h->key[i] & 0xFFFFFFFFu);
        qsort(v, (size_t)h->n, sizeof *v, cmp_u64);
        for (i = 0; i < h->n; i = j) {
            const uint32_t g = (uint32_t)(v[i] >> 32), row = (uint32_t)v[i];
            const uint32_t bin = row < nrows && row_region[row] < nbins ? row_region[row] : nbins - 1u;
            for (j = i + 1; j < h->n && v[j] == v[i]; j++) ;
            if (reg_room(h, g, nbins)) { free(v); fprintf(err, "coverage_depth: out of memory\n"); return 1; }
            h->reg_u[g][bin] += 1; h->reg_t[g][bin] += j - i;
        }
        free(v);
    }
    if (!(strain = strdup(base_of(hits_file_name, hits_file_name + strlen(hits_file_name))))) return 1;
    sl = strlen(strain);
    if (sl >= 13 && !memcmp(strain + sl - 12, "kmer_hits", 9) && !memcmp(strain + sl - 2, "gz", 2)) strain[sl - 13] = 0;
    fputs("strain_name\tmetagenome\tregion\trecord_name\tregion_informative_kmers\tunique_observed_informative_kmers\t"
          "total_observed_informative_kmers\tkmer_coverage\tkmer_depth\n", out);
    for (k = 0; k < h->ndepth; k++) {
        s = h->depth_order[k];
        for (r = 0; r < nbins; r++) {
            const uint64_t u = s < h->nreg_s && h->reg_u[s] ? h->reg_u[s][r] : 0, t = s < h->nreg_s && h->reg_t[s] ? h->reg_t[s][r] : 0;
            char c1[32], c2[32];
            if (!reg_inf[r]) continue;
            skp_float_str((double)u / (double)reg_inf[r], c1);
            skp_float_str((double)t / (double)reg_inf[r], c2);
            if (r < rg->n)
                fprintf(out, "%s\t%s\t%u:%llu-%llu\t%s\t%llu\t%llu\t%llu\t%s\t%s\n", strain, h->smp.name[s], rg->record[r],
                        (unsigned long long)rg->rec_off[r], (unsigned long long)(rg->rec_off[r] + rg->len[r]), rg->name[r],
                        (unsigned long long)reg_inf[r], (unsigned long long)u, (unsigned long long)t, c1, c2);
            else
                fprintf(out, "%s\t%s\tunplaced\t-\t%llu\t%llu\t%llu\t%s\t%s\n", strain, h->smp.name[s],
                        (unsigned long long)reg_inf[r], (unsigned long long)u, (unsigned long long)t, c1, c2);
        }
    }
    free(strain);
    fflush(out);
    return 0;
}

/* ---- the depth spectrum (strain_detect --coverage-spectrum, coverage_depth --spectrum; include/strainer_kmer.h has the rule) ---- */
static int sp_room(hitlist *h, uint32_t g, uint32_t nbins)
{
    if (h->sp_bins && h->sp_bins != nbins) return -1;
    h->sp_bins = nbins;
    if (g >= h->nsp_s) {
        const uint32_t n2 = g + 16u;
        uint64_t **n = realloc(h->sp_n, (size_t)n2 * sizeof *n), *d;
        if (!n) return -1;
        h->sp_n = n;
        if (!(d = realloc(h->sp_deep, (size_t)n2 * sizeof *d))) return -1;
        h->sp_deep = d;
        memset(n + h->nsp_s, 0, (size_t)(n2 - h->nsp_s) * sizeof *n);
        memset(d + h->nsp_s, 0, (size_t)(n2 - h->nsp_s) * sizeof *d);
        h->nsp_s = n2;
    }
    if (!h->sp_n[g] && !(h->sp_n[g] = calloc(nbins, sizeof **h->sp_n))) return -1;
    return 0;
}

/* a metagenome's bins, counted elsewhere (nbins = D + 1: n[1..D], n[>D]; deep_total = hits[>D]): called next to skc_add_counts,
 * after it, so that the sample exists */
int skc_add_spectrum_counts(skc_acc *a, const char *metagenome, const uint64_t *spec, uint64_t deep_total, uint32_t nbins)
{
    hitlist *h = &a->h;
    const char *sn = base_of(metagenome, metagenome + strlen(metagenome));
    const int64_t g = name_get(&h->smp, sn, strlen(sn));
    uint32_t d;
    if (g < 0 || !nbins || sp_room(h, (uint32_t)g, nbins)) return -1;
    for (d = 0; d < nbins; d++) h->sp_n[g][d] += spec[d];
    h->sp_deep[g] += deep_total;
    return 0;
}

/* the table of what sp_n / sp_deep hold, samples in the main table's order; I comes from the sample's trailer */
static void spectrum_print(const hitlist *h, const char *hits_file_name, uint32_t max_depth, FILE *out)
{
    char *strain = strdup(base_of(hits_file_name, hits_file_name + strlen(hits_file_name)));
    const size_t sl = strain ? strlen(strain) : 0;
    uint32_t k, d;
    if (sl >= 13 && !memcmp(strain + sl - 12, "kmer_hits", 9) && !memcmp(strain + sl - 2, "gz", 2)) strain[sl - 13] = 0;
    fputs("strain_name\tmetagenome\tdepth\tinformative_kmers\tobserved_hits\n", out);
    for (k = 0; k < h->ndepth; k++) {
        const uint32_t s = h->depth_order[k];
        const uint64_t *n = s < h->nsp_s ? h->sp_n[s] : NULL;
        uint64_t seen = 0;
        for (d = 0; n && d <= max_depth; d++) seen += n[d];
        if (h->smp.have_inf[s])
            fprintf(out, "%s\t%s\t0\t%lld\t0\n", strain ? strain : "", h->smp.name[s], (long long)(h->smp.g_inf[s] - (int64_t)seen));
        for (d = 1; n && d <= max_depth; d++)
            if (n[d - 1])
                fprintf(out, "%s\t%s\t%u\t%llu\t%llu\n", strain ? strain : "", h->smp.name[s], d, (unsigned long long)n[d - 1],
                        (unsigned long long)(n[d - 1] * d));
        if (n && n[max_depth])
            fprintf(out, "%s\t%s\t>%u\t%llu\t%llu\n", strain ? strain : "", h->smp.name[s], max_depth, (unsigned long long)n[max_depth],
                    (unsigned long long)h->sp_deep[s]);
    }
    free(strain);
    fflush(out);
}

/* The table: call it after skc_report.  An accumulator that was fed hits folds its (sample, row) list here by sort and run lengths;
 * one that was fed counts prints what skc_add_spectrum_counts left. */
int skc_report_spectrum(skc_acc *a, const char *hits_file_name, uint32_t max_depth, FILE *out, FILE *err)
{
    hitlist *h = &a->h;
    if (max_depth < 1u || max_depth > SK_COVACC_SPECTRUM_MAX || (h->sp_bins && h->sp_bins != max_depth + 1u)) return 1;
    if (cov_order_trailers(h)) { fprintf(err, "coverage_depth: out of memory\n"); return 1; }
    if (!h->given && h->n) {
        uint64_t *v = malloc((size_t)h->n * sizeof *v), i, j;
        if (!v) { fprintf(err, "coverage_depth: out of memory\n"); return 1; }
        for (i = 0; i < h->n; i++) v[i] = ((uint64_t)h->sample[i] << 32) | (h->key[i] & 0xFFFFFFFFu);
        qsort(v, (size_t)h->n, sizeof *v, cmp_u64);
        for (i = 0; i < h->n; i = j) {
            const uint32_t g = (uint32_t)(v[i] >> 32);
            for (j = i + 1; j < h->n && v[j] == v[i]; j++) ;
            if (sp_room(h, g, max_depth + 1u)) { free(v); fprintf(err, "coverage_depth: out of memory\n"); return 1; }
            if (j - i <= max_depth) h->sp_n[g][j - i - 1]++;
            else { h->sp_n[g][max_depth]++; h->sp_deep[g] += j - i; }
        }
        free(v);
    }
    spectrum_print(h, hits_file_name, max_depth, out);
    return 0;
}

/* ---- thresholds (strain_detect --coverage-thresholds, coverage_depth --thresholds; include/strainer_kmer.h has the rule) ---- */
/* "t1,t2,...": 0 on success; otherwise `why` says what is wrong with the list */
int skc_parse_threshold_list(const char *text, int64_t *t, uint32_t *n, char *why, size_t why_cap)
{
    const char *p = text;
    *n = 0;
    for (;;) {
        const char *e = p;
        int64_t v;
        while (*e && *e != ',') e++;
        if (e == p) { snprintf(why, why_cap, "an empty field"); return 1; }
        if (*n == SK_COVACC_THRESHOLDS_MAX) { snprintf(why, why_cap, "more than %u thresholds", SK_COVACC_THRESHOLDS_MAX); return 1; }
        if (e - p > 18 || !skp_int(p, e, &v)) { snprintf(why, why_cap, "'%.*s' is no integer from 0 to 2147483646", (int)(e - p > 40 ? 40 : e - p), p); return 1; }
        if (v < 0 || v > 0x7FFFFFFEll) { snprintf(why, why_cap, "%lld is out of range (0 to 2147483646)", (long long)v); return 1; }
        if (*n && v <= t[*n - 1]) { snprintf(why, why_cap, "%lld after %lld: the list must ascend strictly", (long long)v, (long long)t[*n - 1]); return 1; }
        t[(*n)++] = v;
        if (!*e) return 0;
        p = e + 1;
    }
}

int skc_set_thresholds(skc_acc *a, const int64_t *t, uint32_t n)
{
    uint32_t q;
    if (!a || n > SK_COVACC_THRESHOLDS_MAX || (n && !t) || a->h.th_n) return -1;
    for (q = 0; q < n; q++) {
        if (t[q] < 0 || t[q] > 0x7FFFFFFEll || (q && t[q] <= t[q - 1])) return -1;
        a->h.th_t[q] = t[q];
    }
    a->h.th_nt = n;
    return 0;
}

static int th_room(hitlist *h, uint32_t g)
{
    if (g >= h->nth_s) {
        const uint32_t n2 = g + 16u;
        uint64_t **u = realloc(h->th_u, (size_t)n2 * sizeof *u), **t;
        if (!u) return -1;
        h->th_u = u;
        memset(u + h->nth_s, 0, (size_t)(n2 - h->nth_s) * sizeof *u);
        if (!(t = realloc(h->th_tt, (size_t)n2 * sizeof *t))) return -1;       /* (nth_s stays: the new th_u entries are NULL and unread) */
        h->th_tt = t;
        memset(t + h->nth_s, 0, (size_t)(n2 - h->nth_s) * sizeof *t);
        h->nth_s = n2;
    }
    if (!h->th_u[g] && !(h->th_u[g] = calloc(SK_COVACC_THRESHOLDS_MAX, sizeof **h->th_u))) return -1;
    if (!h->th_tt[g] && !(h->th_tt[g] = calloc(SK_COVACC_THRESHOLDS_MAX, sizeof **h->th_tt))) return -1;
    return 0;
}

/* a metagenome's numbers per threshold, counted elsewhere (n = the list's length): called next to skc_add_counts */
int skc_add_threshold_counts(skc_acc *a, const char *metagenome, const uint64_t *unique, const uint64_t *total, uint32_t n)
{
    hitlist *h = &a->h;
    const char *sn = base_of(metagenome, metagenome + strlen(metagenome));
    const int64_t g = name_get(&h->smp, sn, strlen(sn));
    uint32_t q;
    if (g < 0 || n != h->th_nt || th_room(h, (uint32_t)g)) return -1;
    for (q = 0; q < n; q++) { h->th_u[g][q] += unique[q]; h->th_tt[g][q] += total[q]; }
    return 0;
}

/* the table of what th_u / th_tt hold, samples in the main table's order: one line per sample and threshold, zeros included */
static void thresholds_print(const hitlist *h, const char *hits_file_name, FILE *out)
{
    char *strain = strdup(base_of(hits_file_name, hits_file_name + strlen(hits_file_name)));
    const size_t sl = strain ? strlen(strain) : 0;
    uint32_t k, q;
    if (sl >= 13 && !memcmp(strain + sl - 12, "kmer_hits", 9) && !memcmp(strain + sl - 2, "gz", 2)) strain[sl - 13] = 0;
    fputs("strain_name\tmetagenome\tmin_kmer_hits\tunique_observed_informative_kmers\ttotal_observed_informative_kmers\n", out);
    for (k = 0; k < h->ndepth; k++) {
        const uint32_t s = h->depth_order[k];
        const uint64_t *u = s < h->nth_s ? h->th_u[s] : NULL, *t = s < h->nth_s ? h->th_tt[s] : NULL;
        for (q = 0; q < h->th_nt; q++)
            fprintf(out, "%s\t%s\t%lld\t%llu\t%llu\n", strain ? strain : "", h->smp.name[s], (long long)h->th_t[q],
                    (unsigned long long)(u ? u[q] : 0u), (unsigned long long)(t ? t[q] : 0u));
    }
    free(strain);
    fflush(out);
}

typedef struct { uint64_t v; uint32_t cls; } th_item;
static int cmp_th_item(const void *x, const void *y)
{
    const th_item *a = x, *b = y;
    return a->v < b->v ? -1 : a->v > b->v ? 1 : 0;
}

/* The table: call it after skc_report.  An accumulator that was fed hits folds its kept lines here -- a line of class c counts for
 * the thresholds below c, a (sample, row) pair for those below its highest class -- one that was fed counts prints what
 * skc_add_threshold_counts left. */
int skc_report_thresholds(skc_acc *a, const char *hits_file_name, FILE *out, FILE *err)
{
    hitlist *h = &a->h;
    if (!h->th_nt) return 1;
    if (cov_order_trailers(h)) { fprintf(err, "coverage_depth: out of memory\n"); return 1; }
    if (!h->given && h->th_n) {
        th_item *v = malloc((size_t)h->th_n * sizeof *v);
        uint64_t i, j;
        uint32_t q;
        if (!v) { fprintf(err, "coverage_depth: out of memory\n"); return 1; }
        for (i = 0; i < h->th_n; i++) {
            v[i].v = ((uint64_t)h->th_sample[i] << 32) | (h->th_key[i] & 0xFFFFFFFFu);
            v[i].cls = th_class(h, (int64_t)h->th_tot[i]);
        }
        qsort(v, (size_t)h->th_n, sizeof *v, cmp_th_item);
        for (i = 0; i < h->th_n; i = j) {
            const uint32_t g = (uint32_t)(v[i].v >> 32);
            uint32_t top = 0;
            if (th_room(h, g)) { free(v); fprintf(err, "coverage_depth: out of memory\n"); return 1; }
            for (j = i; j < h->th_n && v[j].v == v[i].v; j++) {
                for (q = 0; q < v[j].cls; q++) h->th_tt[g][q]++;
                if (v[j].cls > top) top = v[j].cls;
            }
            for (q = 0; q < top; q++) h->th_u[g][q]++;
        }
        free(v);
        h->th_n = 0;                                 /* (folded: a second report prints the same table) */
    }
    thresholds_print(h, hits_file_name, out);
    return 0;
}

/* ---- the scrub sweep (strain_detect --coverage-scrub-sweep, coverage_depth --scrub-sweep; include/strainer_kmer.h has the rule) ---- */
void skc_classes_free(skc_classes *c)
{
    if (!c) return;
    free(c->arena); free(c->off); free(c->cls);
    memset(c, 0, sizeof *c);
}

/* a class file's k-mer line: text (len bytes) and class */
static int classes_push(skc_classes *c, uint64_t *cap, uint64_t *acap, const char *text, size_t len, uint8_t cls)
{
    if (c->n == *cap) {
        const uint64_t cap2 = *cap ? *cap * 2 : 1u << 12;
        uint64_t *o = realloc(c->off, cap2 * sizeof *o);
        uint8_t *k;
        if (!o) return 1;
        c->off = o;
        if (!(k = realloc(c->cls, cap2))) return 1;
        c->cls = k;
        *cap = cap2;
    }
    if (c->arena_len + len + 1 > *acap) {
        uint64_t cap2 = *acap ? *acap * 2 : 1u << 16;
        char *a;
        while (cap2 < c->arena_len + len + 1) cap2 *= 2;
        if (!(a = realloc(c->arena, cap2))) return 1;
        c->arena = a;
        *acap = cap2;
    }
    memcpy(c->arena + c->arena_len, text, len);
    c->arena[c->arena_len + len] = 0;
    c->off[c->n] = c->arena_len;
    c->cls[c->n++] = cls;
    c->arena_len += len + 1;
    return 0;
}

int skc_classes_read(const char *path, skc_classes *c, char *why, size_t why_cap)
{
    gzFile g;
    char line[1024];
    uint64_t cap = 0, acap = 0, lineno = 0, per[SK_SCRUB_SWEEP_MAX + 1u], run;
    uint32_t q;
    int seen = 0;
    FILE *probe = fopen(path, "rb");
    memset(c, 0, sizeof *c);
    memset(per, 0, sizeof per);
    if (!probe) { snprintf(why, why_cap, "could not read it"); return 1; }
    fclose(probe);
    if (!(g = gzopen(path, "rb"))) { snprintf(why, why_cap, "could not read it"); return 1; }
    while (gzgets(g, line, (int)sizeof line)) {
        size_t len = strlen(line);
        lineno++;
        if (!len || line[len - 1] != '\n') {
            if (len + 1 == sizeof line) { snprintf(why, why_cap, "line %llu is too long", (unsigned long long)lineno); goto bad; }
        } else line[--len] = 0;
        if (lineno == 1) {
            skw_list l;
            char w[120];
            if (strncmp(line, "#min_fractions\t", 15)) { snprintf(why, why_cap, "its first line is not #min_fractions<TAB>f0,f1,..."); goto bad; }
            if (skw_parse_list(line + 15, &l, w, sizeof w)) { snprintf(why, why_cap, "its fraction list: %s", w); goto bad; }
            c->F = l.n;
            memcpy(c->frac, l.text, sizeof c->frac);
            continue;
        }
        if (lineno == 2) {
            const char *p = line + 18;
            if (strncmp(line, "#post_scrub_kmers\t", 18)) { snprintf(why, why_cap, "its second line is not #post_scrub_kmers<TAB>n0,n1,..."); goto bad; }
            for (q = 0; q < c->F; q++) {
                const char *e = p;
                int64_t v;
                while (*e && *e != ',') e++;
                if (e == p || e - p > 18 || !skp_int(p, e, &v) || v < 0 || (q + 1 < c->F) != (*e == ',') || (q && (uint64_t)v > c->size[q - 1])) {
                    snprintf(why, why_cap, "its second line does not give %u set sizes that do not grow", c->F);
                    goto bad;
                }
                c->size[q] = (uint64_t)v;
                p = e + 1;
            }
            seen = 1;
            continue;
        }
        {
            const char *tab = strchr(line, '\t');
            int64_t v;
            if (!tab || tab == line || strchr(tab + 1, '\t') || !skp_int(tab + 1, line + len, &v) || v < 1 || v > (int64_t)c->F) {
                snprintf(why, why_cap, "line %llu is not kmer<TAB>class with a class from 1 to %u", (unsigned long long)lineno, c->F);
                goto bad;
            }
            if (classes_push(c, &cap, &acap, line, (size_t)(tab - line), (uint8_t)v)) { snprintf(why, why_cap, "out of memory"); goto bad; }
            per[v]++;
        }
    }
    if (!seen) { snprintf(why, why_cap, "its two header lines are missing"); goto bad; }
    for (run = 0, q = c->F; q-- > 0u; ) {              /* set q holds the rows of class >= q + 1 */
        run += per[q + 1u];
        if (run != c->size[q]) {
            snprintf(why, why_cap, "%llu lines have class %u or more, its header says %llu", (unsigned long long)run, q + 1u, (unsigned long long)c->size[q]);
            goto bad;
        }
    }
    gzclose(g);
    return 0;
bad:
    gzclose(g);
    skc_classes_free(c);
    return 1;
}

int skc_set_classes(skc_acc *a, const skc_classes *c)
{
    if (!a || !c || c->F < 1u || c->F > SK_SCRUB_SWEEP_MAX) return -1;
    a->h.cl_F = c->F;
    memcpy(a->h.cl_frac, c->frac, sizeof a->h.cl_frac);
    memcpy(a->h.cl_size, c->size, sizeof a->h.cl_size);
    return 0;
}

static int cl_room(hitlist *h, uint32_t g)
{
    if (g >= h->ncl_s) {
        const uint32_t n2 = g + 16u;
        uint64_t **u = realloc(h->cl_u, (size_t)n2 * sizeof *u), **t;
        if (!u) return -1;
        h->cl_u = u;
        memset(u + h->ncl_s, 0, (size_t)(n2 - h->ncl_s) * sizeof *u);
        if (!(t = realloc(h->cl_t, (size_t)n2 * sizeof *t))) return -1;        /* (ncl_s stays: the new cl_u entries are NULL and unread) */
        h->cl_t = t;
        memset(t + h->ncl_s, 0, (size_t)(n2 - h->ncl_s) * sizeof *t);
        h->ncl_s = n2;
    }
    if (!h->cl_u[g] && !(h->cl_u[g] = calloc(SK_SCRUB_SWEEP_MAX, sizeof **h->cl_u))) return -1;
    if (!h->cl_t[g] && !(h->cl_t[g] = calloc(SK_SCRUB_SWEEP_MAX, sizeof **h->cl_t))) return -1;
    return 0;
}

/* a metagenome's numbers per fraction, counted elsewhere (F = the list's length): called next to skc_add_counts */
int skc_add_class_counts(skc_acc *a, const char *metagenome, const uint64_t *unique, const uint64_t *total, uint32_t F)
{
    hitlist *h = &a->h;
    const char *sn = base_of(metagenome, metagenome + strlen(metagenome));
    const int64_t g = name_get(&h->smp, sn, strlen(sn));
    uint32_t q;
    if (g < 0 || F != h->cl_F || cl_room(h, (uint32_t)g)) return -1;
    for (q = 0; q < F; q++) { h->cl_u[g][q] += unique[q]; h->cl_t[g][q] += total[q]; }
    return 0;
}

/* the table of what cl_u / cl_t hold, samples in the main table's order: one line per sample and fraction, zeros included */
static void classes_print(const hitlist *h, const char *hits_file_name, FILE *out)
{
    char *strain = strdup(base_of(hits_file_name, hits_file_name + strlen(hits_file_name)));
    const size_t sl = strain ? strlen(strain) : 0;
    uint32_t k, q;
    if (sl >= 13 && !memcmp(strain + sl - 12, "kmer_hits", 9) && !memcmp(strain + sl - 2, "gz", 2)) strain[sl - 13] = 0;
    fputs("strain_name\tmetagenome\tmin_fraction\tgenome_num_informative_kmers\tunique_observed_informative_kmers\t"
          "total_observed_informative_kmers\n", out);
    for (k = 0; k < h->ndepth; k++) {
        const uint32_t s = h->depth_order[k];
        const uint64_t *u = s < h->ncl_s ? h->cl_u[s] : NULL, *t = s < h->ncl_s ? h->cl_t[s] : NULL;
        for (q = 0; q < h->cl_F; q++)
            fprintf(out, "%s\t%s\t%s\t%llu\t%llu\t%llu\n", strain ? strain : "", h->smp.name[s], h->cl_frac[q],
                    (unsigned long long)h->cl_size[q], (unsigned long long)(u ? u[q] : 0u), (unsigned long long)(t ? t[q] : 0u));
    }
    free(strain);
    fflush(out);
}

/* The table: call it after skc_report.  An accumulator that was fed hits folds its (sample, row) list here -- a row of class c counts
 * for the fractions below c -- one that was fed counts prints what skc_add_class_counts left. */
int skc_report_classes(skc_acc *a, const char *hits_file_name, const uint8_t *row_class, uint32_t nrows, FILE *out, FILE *err)
{
    hitlist *h = &a->h;
    if (!h->cl_F) return 1;
    if (cov_order_trailers(h)) { fprintf(err, "coverage_depth: out of memory\n"); return 1; }
    if (!h->given && h->n && !h->ncl_s) {            /* (folded already: a second report prints the same table) */
        uint64_t *v = malloc((size_t)h->n * sizeof *v), i, j;
        uint32_t q;
        if (!v || !row_class) { free(v); fprintf(err, "coverage_depth: out of memory\n"); return 1; }
        for (i = 0; i < h->n; i++) v[i] = ((uint64_t)h->sample[i] << 32) | (h->key[i] & 0xFFFFFFFFu);
        qsort(v, (size_t)h->n, sizeof *v, cmp_u64);
        for (i = 0; i < h->n; i = j) {
            const uint32_t g = (uint32_t)(v[i] >> 32), row = (uint32_t)v[i];
            const uint32_t c = row < nrows ? row_class[row] : 0u;
            for (j = i + 1; j < h->n && v[j] == v[i]; j++) ;
            if (c < 1u || c > h->cl_F) {
                free(v);
                fprintf(err, "coverage_depth: internal error: a hit on row %u, which is in none of the scrub sweep's sets\n", row);
                return 1;
            }
            if (cl_room(h, g)) { free(v); fprintf(err, "coverage_depth: out of memory\n"); return 1; }
            for (q = 0; q < c; q++) { h->cl_u[g][q] += 1; h->cl_t[g][q] += j - i; }
        }
        free(v);
    }
    classes_print(h, hits_file_name, out);
    return 0;
}

/* ---- recurrence (strain_detect --coverage-recurrence, coverage_depth --recurrence; include/strainer_kmer.h has the rule) ---- */
/* a run's tables, counted elsewhere: T samples by the caller's ordinals (metagenome[i] names ordinal i; every one of them has been
 * handed to skc_add_counts or skc_add_trailer, so the sample exists), hist[T + 1] (entry 0 is not used) and pairs[T x T] or NULL.
 * Once per accumulator. */
int skc_add_recurrence_counts(skc_acc *a, const char *const *metagenome, uint32_t T, const uint64_t *hist, const uint64_t *pairs)
{
    hitlist *h = &a->h;
    uint32_t i;
    if (h->rc_hist || !T) return -1;
    if (!(h->rc_hist = malloc(((size_t)T + 1u) * sizeof *h->rc_hist)) || !(h->rc_smp = malloc((size_t)T * sizeof *h->rc_smp))) return -1;
    if (pairs && !(h->rc_pairs = malloc((size_t)T * T * sizeof *h->rc_pairs))) return -1;
    memcpy(h->rc_hist, hist, ((size_t)T + 1u) * sizeof *hist);
    if (pairs) memcpy(h->rc_pairs, pairs, (size_t)T * T * sizeof *pairs);
    for (i = 0; i < T; i++) {
        const char *sn = base_of(metagenome[i], metagenome[i] + strlen(metagenome[i]));
        const int64_t g = name_get(&h->smp, sn, strlen(sn));
        if (g < 0) return -1;
        h->rc_smp[i] = (uint32_t)g;
    }
    h->rc_T = T;
    return 0;
}

/* both tables of hist[T + 1] (entry 0 is computed here) and shared[T x T] by position in the main table's order (NULL: no pair table) */
static void recurrence_print(const hitlist *h, const char *hits_file_name, uint32_t T, const uint64_t *hist, const uint64_t *shared,
                             FILE *out, FILE *out_pairs)
{
    char *strain = strdup(base_of(hits_file_name, hits_file_name + strlen(hits_file_name)));
    const size_t sl = strain ? strlen(strain) : 0;
    const char *nm;
    uint64_t seen = 0;
    uint32_t k, m, i, j;
    if (sl >= 13 && !memcmp(strain + sl - 12, "kmer_hits", 9) && !memcmp(strain + sl - 2, "gz", 2)) strain[sl - 13] = 0;
    nm = strain ? strain : "";
    fputs("strain_name\tsamples\tseen_in\tinformative_kmers\n", out);
    for (m = 1; m <= T; m++) seen += hist[m];
    for (k = 0; k < h->ndepth; k++)                  /* I: the trailer of the first sample of the table that has one */
        if (h->smp.have_inf[h->depth_order[k]]) {
            fprintf(out, "%s\t%u\t0\t%lld\n", nm, T, (long long)(h->smp.g_inf[h->depth_order[k]] - (int64_t)seen));
            break;
        }
    for (m = 1; m <= T; m++)
        if (hist[m]) fprintf(out, "%s\t%u\t%u\t%llu\n", nm, T, m, (unsigned long long)hist[m]);
    fflush(out);
    if (out_pairs && (shared || !T)) {
        fputs("strain_name\tmetagenome_a\tmetagenome_b\tshared_informative_kmers\teither_informative_kmers\n", out_pairs);
        for (i = 0; i < T; i++)
            for (j = i; j < T; j++) {
                const uint64_t sh = shared[(size_t)i * T + j];
                fprintf(out_pairs, "%s\t%s\t%s\t%llu\t%llu\n", nm, h->smp.name[h->depth_order[i]], h->smp.name[h->depth_order[j]],
                        (unsigned long long)sh, (unsigned long long)(shared[(size_t)i * T + i] + shared[(size_t)j * T + j] - sh));
            }
        fflush(out_pairs);
    }
    free(strain);
}

typedef struct { uint64_t key; uint32_t pos; } rc_item;
static int cmp_rc_item(const void *x, const void *y)
{
    const rc_item *a = x, *b = y;
    return a->key < b->key ? -1 : a->key > b->key ? 1 : a->pos < b->pos ? -1 : a->pos > b->pos;
}

/* the fold of a (sample, key) list: pos_of[sample] = its position among T, hist[T + 1] and shared[T x T] (NULL: not wanted) zeroed
 * by the caller.  Sort by key, then position; a key's distinct positions give its m and its pairs. */
static int recurrence_fold(const uint64_t *key, const uint32_t *sample, uint64_t n, const uint32_t *pos_of, uint32_t T, uint64_t *hist,
                           uint64_t *shared)
{
    rc_item *v;
    uint32_t *at;
    uint64_t i, j;
    if (!n) return 0;
    if (!(v = malloc((size_t)n * sizeof *v))) return -1;
    if (!(at = malloc(((size_t)T + 1u) * sizeof *at))) { free(v); return -1; }
    for (i = 0; i < n; i++) { v[i].key = key[i]; v[i].pos = pos_of[sample[i]]; }
    qsort(v, (size_t)n, sizeof *v, cmp_rc_item);
    for (i = 0; i < n; i = j) {
        uint32_t m = 0, x, y;
        for (j = i; j < n && v[j].key == v[i].key; j++)
            if (v[j].pos < T && (!m || at[m - 1] != v[j].pos)) at[m++] = v[j].pos;
        hist[m]++;
        for (x = 0; shared && x < m; x++)
            for (y = x; y < m; y++) {
                shared[(size_t)at[x] * T + at[y]]++;
                if (x != y) shared[(size_t)at[y] * T + at[x]]++;
            }
    }
    hist[0] = 0;
    free(at); free(v);
    return 0;
}

/* The tables: call it after skc_report.  T = the samples of the main table, in its order.  An accumulator that was fed hits folds
 * its (sample, row) list here; one that was fed counts prints what skc_add_recurrence_counts left.  out_pairs NULL: no pair table. */
int skc_report_recurrence(skc_acc *a, const char *hits_file_name, FILE *out, FILE *out_pairs, FILE *err)
{
    hitlist *h = &a->h;
    uint64_t *hist = NULL, *shared = NULL;
    uint32_t *pos_of = NULL, T, k, i, j;
    int status = 1;
    if (cov_order_trailers(h)) { fprintf(err, "coverage_depth: out of memory\n"); return 1; }
    T = h->ndepth;
    if (T > SK_RECUR_SAMPLES_MAX || (out_pairs && T > SK_RECUR_PAIRS_MAX)) {
        fprintf(err, "coverage_depth: %u samples: recurrence takes at most %u, its pair table %u\n", T, SK_RECUR_SAMPLES_MAX, SK_RECUR_PAIRS_MAX);
        return 1;
    }
    if (!(hist = calloc((size_t)T + 1u, sizeof *hist)) || !(pos_of = malloc(((size_t)h->smp.n + 1u) * sizeof *pos_of)) ||
        (out_pairs && !(shared = calloc((size_t)T * T + 1u, sizeof *shared)))) { fprintf(err, "coverage_depth: out of memory\n"); goto done; }
    for (k = 0; k < h->smp.n; k++) pos_of[k] = T;    /* (a sample outside the table: never) */
    for (k = 0; k < T; k++) pos_of[h->depth_order[k]] = k;
    if (h->rc_hist) {
        if (h->rc_T != T || (out_pairs && !h->rc_pairs)) { fprintf(err, "coverage_depth: the recurrence counts are of %u samples, the table has %u\n", h->rc_T, T); goto done; }
        memcpy(hist, h->rc_hist, ((size_t)T + 1u) * sizeof *hist);
        for (i = 0; out_pairs && i < T; i++)
            for (j = 0; j < T; j++) {
                const uint32_t pi = pos_of[h->rc_smp[i]], pj = pos_of[h->rc_smp[j]];
                if (pi < T && pj < T) shared[(size_t)pi * T + pj] = h->rc_pairs[(size_t)i * T + j];
            }
    } else if (!h->given && recurrence_fold(h->key, h->sample, h->n, pos_of, T, hist, shared)) { fprintf(err, "coverage_depth: out of memory\n"); goto done; }
    recurrence_print(h, hits_file_name, T, hist, shared, out, out_pairs);
    status = 0;
done:
    free(hist); free(shared); free(pos_of);
    return status;
}

/* (the host-only test builds link this file without sk_cover.hip's newer entry points: without them --spectrum / --recurrence are refused) */
#pragma weak sk_distinct_recurrence
/* coverage_depth --recurrence [--recurrence-pairs]: the (sample, packed k-mer) pairs through the device's bit planes, to the tables
 * at `path` and `pairs_path` (NULL: no pair table) */
static int cov_recurrence_files(hitlist *h, sk_ctx *ctx, const char *kfile, const char *path, const char *pairs_path, FILE *err)
{
    const uint32_t T = h->ndepth;
    uint64_t *hist = NULL, *shared = NULL, i;
    uint32_t *pos_of = NULL, *smp = NULL, k;
    FILE *f = NULL, *fp = NULL;
    int rc, status = 1;
    if (T > SK_RECUR_SAMPLES_MAX || (pairs_path && T > SK_RECUR_PAIRS_MAX)) {
        fprintf(err, "coverage_depth: %u samples: --recurrence takes at most %u, --recurrence-pairs %u\n", T, SK_RECUR_SAMPLES_MAX, SK_RECUR_PAIRS_MAX);
        return 1;
    }
    if (!(hist = calloc((size_t)T + 1u, sizeof *hist)) || !(pos_of = malloc(((size_t)h->smp.n + 1u) * sizeof *pos_of)) ||
        !(smp = malloc(((size_t)h->n + 1u) * sizeof *smp)) || (pairs_path && !(shared = calloc((size_t)T * T + 1u, sizeof *shared)))) {
        fprintf(err, "coverage_depth: out of memory\n");
        goto done;
    }
    for (k = 0; k < h->smp.n; k++) pos_of[k] = 0;
    for (k = 0; k < T; k++) pos_of[h->depth_order[k]] = k;   /* (every sample of a passing line is in the table) */
    for (i = 0; i < h->n; i++) smp[i] = pos_of[h->sample[i]];
    if (T) {
        rc = sk_distinct_recurrence(ctx, h->key, smp, h->n, T, hist, shared);
        if (rc != SK_OK) { fprintf(err, "coverage_depth: %s (%s)\n", sk_strerror(rc), sk_last_error(ctx)); goto done; }
    }
    if (!(f = fopen(path, "w"))) { fprintf(err, "coverage_depth: could not write %s\n", path); goto done; }
    if (pairs_path && !(fp = fopen(pairs_path, "w"))) { fprintf(err, "coverage_depth: could not write %s\n", pairs_path); goto done; }
    recurrence_print(h, kfile, T, hist, shared, f, fp);
    status = ferror(f) || (fp && ferror(fp)) ? 1 : 0;
done:
    if (f && fclose(f)) status = 1;
    if (fp && fclose(fp)) status = 1;
    free(hist); free(shared); free(pos_of); free(smp);
    return status;
}

/* where a table goes: the explicit name, or the hits file's path with a trailing ".kmer_hits.gz" replaced by `suffix` */
static char *cov_table_path(const char *explicit_path, const char *kfile, const char *suffix)
{
    char *p;
    size_t n = strlen(kfile);
    if (explicit_path && *explicit_path) return strdup(explicit_path);
    if (!(p = malloc(n + strlen(suffix) + 1))) return NULL;
    strcpy(p, kfile);
    if (n >= 13 && !strcmp(p + n - 13, ".kmer_hits.gz")) p[n - 13] = 0;
    strcat(p, suffix);
    return p;
}

#pragma weak sk_distinct_spectrum
/* coverage_depth --spectrum: the multiplicities of the (sample, packed k-mer) pairs, counted on the device, to the table at `path` */
static int cov_spectrum_file(hitlist *h, sk_ctx *ctx, const char *kfile, uint32_t max_depth, const char *path, FILE *err)
{
    const uint32_t ns = h->smp.n, nb = max_depth + 1u;
    uint64_t *buf = NULL;
    FILE *f;
    uint32_t s, d;
    int rc, status = 1;
    if (ns) {
        if (!(buf = calloc((size_t)ns * (nb + 3u), sizeof *buf))) { fprintf(err, "coverage_depth: out of memory\n"); return 1; }
        rc = sk_distinct_spectrum(ctx, h->key, h->sample, h->n, ns, max_depth, buf, buf + ns, buf + 3u * (size_t)ns, buf + 2u * (size_t)ns);
        if (rc != SK_OK) { fprintf(err, "coverage_depth: %s (%s)\n", sk_strerror(rc), sk_last_error(ctx)); goto done; }
        for (s = 0; s < ns; s++) {
            const uint64_t *n = buf + 3u * (size_t)ns + (size_t)s * nb;
            if (!buf[s]) continue;                   /* (a sample without a passing line keeps no bins) */
            if (sp_room(h, s, nb)) { fprintf(err, "coverage_depth: out of memory\n"); goto done; }
            for (d = 0; d < nb; d++) h->sp_n[s][d] = n[d];
            h->sp_deep[s] = buf[2u * (size_t)ns + s];
        }
    }
    if (!(f = fopen(path, "w"))) { fprintf(err, "coverage_depth: could not write %s\n", path); goto done; }
    spectrum_print(h, kfile, max_depth, f);
    status = ferror(f) ? 1 : 0;
    if (fclose(f)) status = 1;
done:
    free(buf);
    return status;
}

#pragma weak sk_distinct_thresholds
/* coverage_depth --thresholds: the kept lines' (sample, packed k-mer, total) triples, counted on the device, to the table at `path` */
static int cov_thresholds_file(hitlist *h, sk_ctx *ctx, const char *kfile, const char *path, FILE *err)
{
    const uint32_t ns = h->smp.n, nt = h->th_nt;
    uint64_t *buf = NULL;
    FILE *f;
    uint32_t s, q;
    int rc, status = 1;
    if (ns) {
        if (!(buf = calloc((size_t)ns * nt * 2u, sizeof *buf))) { fprintf(err, "coverage_depth: out of memory\n"); return 1; }
        rc = sk_distinct_thresholds(ctx, h->th_key, h->th_sample, h->th_tot, h->th_n, ns, h->th_t, nt, buf, buf + (size_t)ns * nt);
        if (rc != SK_OK) { fprintf(err, "coverage_depth: %s (%s)\n", sk_strerror(rc), sk_last_error(ctx)); goto done; }
        for (s = 0; s < ns; s++) {
            if (!buf[(size_t)ns * nt + (size_t)s * nt]) continue;      /* (no line above t[0]: zeros are printed without) */
            if (th_room(h, s)) { fprintf(err, "coverage_depth: out of memory\n"); goto done; }
            for (q = 0; q < nt; q++) { h->th_u[s][q] = buf[(size_t)s * nt + q]; h->th_tt[s][q] = buf[(size_t)ns * nt + (size_t)s * nt + q]; }
        }
    }
    if (!(f = fopen(path, "w"))) { fprintf(err, "coverage_depth: could not write %s\n", path); goto done; }
    thresholds_print(h, kfile, f);
    status = ferror(f) ? 1 : 0;
    if (fclose(f)) status = 1;
done:
    free(buf);
    return status;
}

#pragma weak sk_distinct_classes
typedef struct { uint64_t key; uint8_t cls; } cl_key;
static int cmp_cl_key(const void *x, const void *y)
{
    const cl_key *a = x, *b = y;
    return a->key < b->key ? -1 : a->key > b->key;
}

/* coverage_depth --scrub-sweep, before anything is printed: every passing line's class by its packed k-mer; *out_cls has h->n bytes.
 * 1 with one line on err: a k-mer of the class file that is no A/C/G/T word of the hit list's length, one named twice, or a hit
 * line whose k-mer the class file does not name. */
static int cov_sweep_classes(const hitlist *h, const skc_classes *c, const char *kfile, const char *cfile, uint8_t **out_cls, FILE *err)
{
    cl_key *v = malloc((size_t)(c->n ? c->n : 1) * sizeof *v);
    uint8_t *cls = malloc((size_t)(h->n ? h->n : 1));
    uint64_t i;
    if (!v || !cls) { fprintf(err, "coverage_depth: out of memory\n"); goto bad; }
    for (i = 0; i < c->n; i++) {
        const char *t = c->arena + c->off[i];
        const size_t len = strlen(t);
        uint64_t key = 0;
        size_t j;
        int plain = len >= 1 && len <= 31 && (h->klen == 0 || h->klen == len);
        for (j = 0; plain && j < len; j++) {
            const unsigned cde = sk_code((uint8_t)t[j]);
            if (t[j] != "ACGT"[cde]) plain = 0;
            key = (key << 2) | (cde & 3u);
        }
        if (!plain) { fprintf(err, "coverage_depth: --scrub-classes %s: k-mer %s is no A/C/G/T word of the hit list's k-mer length\n", cfile, t); goto bad; }
        v[i].key = key; v[i].cls = c->cls[i];
    }
    qsort(v, (size_t)c->n, sizeof *v, cmp_cl_key);
    for (i = 1; i < c->n; i++)
        if (v[i].key == v[i - 1].key) { fprintf(err, "coverage_depth: --scrub-classes %s names a k-mer twice\n", cfile); goto bad; }
    for (i = 0; i < h->n; i++) {
        uint64_t lo = 0, hi = c->n;
        while (lo < hi) { const uint64_t mid = lo + ((hi - lo) >> 1); if (v[mid].key < h->key[i]) lo = mid + 1; else hi = mid; }
        if (lo >= c->n || v[lo].key != h->key[i]) {
            fprintf(err, "coverage_depth: --scrub-sweep: %s has a hit on a k-mer that the class file %s does not name\n", kfile, cfile);
            goto bad;
        }
        cls[i] = v[lo].cls;
    }
    free(v);
    *out_cls = cls;
    return 0;
bad:
    free(v); free(cls);
    return 1;
}

/* ... and the passing lines' (sample, packed k-mer, class) triples, counted on the device, to the table at `path` */
static int cov_sweep_file(hitlist *h, sk_ctx *ctx, const char *kfile, const uint8_t *cls, const char *path, FILE *err)
{
    const uint32_t ns = h->smp.n, F = h->cl_F;
    uint64_t *buf = NULL;
    FILE *f;
    uint32_t s, q;
    int rc, status = 1;
    if (ns) {
        if (!(buf = calloc((size_t)ns * F * 2u, sizeof *buf))) { fprintf(err, "coverage_depth: out of memory\n"); return 1; }
        rc = sk_distinct_classes(ctx, h->key, h->sample, cls, h->n, ns, F, buf, buf + (size_t)ns * F);
        if (rc != SK_OK) { fprintf(err, "coverage_depth: %s (%s)\n", sk_strerror(rc), sk_last_error(ctx)); goto done; }
        for (s = 0; s < ns; s++) {
            if (!buf[(size_t)ns * F + (size_t)s * F]) continue;        /* (no passing line: zeros are printed without) */
            if (cl_room(h, s)) { fprintf(err, "coverage_depth: out of memory\n"); goto done; }
            for (q = 0; q < F; q++) { h->cl_u[s][q] = buf[(size_t)s * F + q]; h->cl_t[s][q] = buf[(size_t)ns * F + (size_t)s * F + q]; }
        }
    }
    if (!(f = fopen(path, "w"))) { fprintf(err, "coverage_depth: could not write %s\n", path); goto done; }
    classes_print(h, kfile, f);
    status = ferror(f) ? 1 : 0;
    if (fclose(f)) status = 1;
done:
    free(buf);
    return status;
}

int skh_coverage_depth_main(int argc, char **argv, FILE *out, FILE *err)
{
    const char *sw_file = NULL, *sw_classes = NULL;
    int want_sw = 0;
    char *sw_path = NULL;
    uint8_t *sw_cls = NULL;
    skc_classes sw_c;
    const char *th_file = NULL, *th_list = NULL;
    int want_th = 0;
    char *th_path = NULL;
    int64_t th_t[SK_COVACC_THRESHOLDS_MAX] = { 0, 1, 2, 3, 5, 10, 20, 50 };
    uint32_t th_nt = 8;
    const char *kfile = NULL, *mtext = NULL, *bfile = NULL, *env, *sp_file = NULL, *sp_max = NULL, *rc_file = NULL, *rp_file = NULL;
    int64_t min_hits = 1, sp_d = 255;
    int i, bad = 0, rc, status = 1, device = 0, want_sp = 0, want_rc = 0, want_rp = 0;
    char *sp_path = NULL, *rc_path = NULL, *rp_path = NULL;
    hitlist h;
    sk_ctx *ctx = NULL;

    for (i = 1; i < argc; i++) {                     /* :27-41 */
        if (!strcmp(argv[i], "-h") || !strcmp(argv[i], "--help")) {
            fprintf(out, "usage: coverage_depth [-h] --kmer_hits_file FILE [--min_kmer_hits N] [--background_metagenomes_file FILE]\n"
                         "                      [--spectrum[=FILE] [--spectrum-max D]] [--recurrence[=FILE] [--recurrence-pairs[=FILE]]]\n"
                         "                      [--thresholds[=FILE] [--threshold-list t1,t2,...]]\n"
                         "                      [--scrub-classes FILE --scrub-sweep[=FILE]]\n");
            return 0;
        }
        /* "--spectrum[=FILE] [--spectrum-max D]" (extension): the depth spectrum beside the table, see include/strainer_kmer.h */
        if (!strncmp(argv[i], "--spectrum", 10) && (argv[i][10] == 0 || argv[i][10] == '=')) { want_sp = 1; sp_file = argv[i][10] ? argv[i] + 11 : NULL; continue; }
        /* "--recurrence[=FILE] [--recurrence-pairs[=FILE]]" (extension): in how many samples each k-mer was seen, and what two samples share */
        if (!strncmp(argv[i], "--recurrence-pairs", 18) && (argv[i][18] == 0 || argv[i][18] == '=')) { want_rp = 1; rp_file = argv[i][18] ? argv[i] + 19 : NULL; continue; }
        if (!strncmp(argv[i], "--recurrence", 12) && (argv[i][12] == 0 || argv[i][12] == '=')) { want_rc = 1; rc_file = argv[i][12] ? argv[i] + 13 : NULL; continue; }
        if (!strcmp(argv[i], "--spectrum-max") && i + 1 < argc) { sp_max = argv[++i]; continue; }
        if (!strncmp(argv[i], "--spectrum-max=", 15)) { sp_max = argv[i] + 15; continue; }
        /* "--thresholds[=FILE] [--threshold-list t1,t2,...]" (extension): the table's two numbers at several --min_kmer_hits */
        if (!strncmp(argv[i], "--thresholds", 12) && (argv[i][12] == 0 || argv[i][12] == '=')) { want_th = 1; th_file = argv[i][12] ? argv[i] + 13 : NULL; continue; }
        if (!strcmp(argv[i], "--threshold-list") && i + 1 < argc) { th_list = argv[++i]; continue; }
        if (!strncmp(argv[i], "--threshold-list=", 17)) { th_list = argv[i] + 17; continue; }
        /* "--scrub-classes FILE --scrub-sweep[=FILE]" (extension): the table's numbers at every fraction of a class file */
        if (!strncmp(argv[i], "--scrub-sweep", 13) && (argv[i][13] == 0 || argv[i][13] == '=')) { want_sw = 1; sw_file = argv[i][13] ? argv[i] + 14 : NULL; continue; }
        if (!strcmp(argv[i], "--scrub-classes") && i + 1 < argc) { sw_classes = argv[++i]; continue; }
        if (!strncmp(argv[i], "--scrub-classes=", 16)) { sw_classes = argv[i] + 16; continue; }
        if (cov_opt(argc, argv, &i, "-k", "--kmer_hits_file", &kfile, err, &bad)) { if (bad) return 2; continue; }
        if (cov_opt(argc, argv, &i, "-m", "--min_kmer_hits", &mtext, err, &bad)) { if (bad) return 2; continue; }
        if (cov_opt(argc, argv, &i, "-b", "--background_metagenomes_file", &bfile, err, &bad)) { if (bad) return 2; continue; }
        fprintf(err, "coverage_depth: error: unrecognized arguments: %s\n", argv[i]);
        return 2;
    }
    if (!kfile) { fprintf(err, "coverage_depth: error: the following arguments are required: --kmer_hits_file/-k\n"); return 2; }
    if (mtext && !skp_int(mtext, mtext + strlen(mtext), &min_hits)) {
        fprintf(err, "coverage_depth: error: argument --min_kmer_hits/-m: invalid int value: '%s'\n", mtext);
        return 2;
    }
    if (sp_max && !want_sp) { fprintf(err, "coverage_depth: error: --spectrum-max goes with --spectrum\n"); return 2; }
    if (sp_max && (!skp_int(sp_max, sp_max + strlen(sp_max), &sp_d) || sp_d < 1 || sp_d > (int64_t)SK_COVACC_SPECTRUM_MAX)) {
        fprintf(err, "coverage_depth: error: --spectrum-max %s: a depth from 1 to %u\n", sp_max, SK_COVACC_SPECTRUM_MAX);
        return 2;
    }
    if (want_sp && !sk_distinct_spectrum) { fprintf(err, "coverage_depth: error: --spectrum: this build has no device spectrum\n"); return 2; }
    if (want_rp && !want_rc) { fprintf(err, "coverage_depth: error: --recurrence-pairs goes with --recurrence\n"); return 2; }
    if (th_list && !want_th) { fprintf(err, "coverage_depth: error: --threshold-list goes with --thresholds\n"); return 2; }
    if (th_list) {
        char why[160];
        if (skc_parse_threshold_list(th_list, th_t, &th_nt, why, sizeof why)) { fprintf(err, "coverage_depth: error: --threshold-list %s: %s\n", th_list, why); return 2; }
    }
    if (want_th && !sk_distinct_thresholds) { fprintf(err, "coverage_depth: error: --thresholds: this build has no device thresholds\n"); return 2; }
    if (want_rc && !sk_distinct_recurrence) { fprintf(err, "coverage_depth: error: --recurrence: this build has no device recurrence\n"); return 2; }
    memset(&sw_c, 0, sizeof sw_c);
    if (want_sw != (sw_classes != NULL)) { fprintf(err, "coverage_depth: error: --scrub-sweep and --scrub-classes go together\n"); return 2; }
    if (want_sw && !sk_distinct_classes) { fprintf(err, "coverage_depth: error: --scrub-sweep: this build has no device classes\n"); return 2; }
    if (want_sw) {
        char why[200];
        if (skc_classes_read(sw_classes, &sw_c, why, sizeof why)) { fprintf(err, "coverage_depth: error: --scrub-classes %s: %s\n", sw_classes, why); return 2; }
    }
    memset(&h, 0, sizeof h);
    if (want_th) { memcpy(h.th_t, th_t, sizeof h.th_t); h.th_nt = th_nt; }
    rc = read_hits(&h, kfile, min_hits);
    if (rc == COV_OPEN) { fprintf(err, "coverage_depth: could not read %s\n", kfile); goto done; }
    if (rc == COV_FIELDS) { fprintf(err, "coverage_depth: %s: a line has too few tab-separated fields\n", kfile); goto done; }
    if (rc == COV_INT) { fprintf(err, "coverage_depth: %s: a count field is not an integer\n", kfile); goto done; }
    if (rc == COV_NOMEM) { fprintf(err, "coverage_depth: out of memory\n"); goto done; }
    if (want_sp && h.general) {                      /* (before anything is printed) */
        fprintf(err, "coverage_depth: --spectrum: %s has k-mer fields that are not A/C/G/T words of one length: the depth of a k-mer is not defined there\n", kfile);
        goto done;
    }
    if (want_th && (h.general || h.th_bad)) {
        fprintf(err, "coverage_depth: --thresholds: %s has k-mer fields that are not A/C/G/T words of one length: a distinct k-mer is not defined there\n", kfile);
        goto done;
    }
    if (want_th && !(th_path = cov_table_path(th_file, kfile, ".coverage_thresholds"))) { fprintf(err, "coverage_depth: out of memory\n"); goto done; }
    if (want_sw && h.general) {
        fprintf(err, "coverage_depth: --scrub-sweep: %s has k-mer fields that are not A/C/G/T words of one length: a k-mer's class is not defined there\n", kfile);
        goto done;
    }
    if (want_sw) {
        h.cl_F = sw_c.F;
        memcpy(h.cl_frac, sw_c.frac, sizeof h.cl_frac);
        memcpy(h.cl_size, sw_c.size, sizeof h.cl_size);
        if (cov_sweep_classes(&h, &sw_c, kfile, sw_classes, &sw_cls, err)) goto done;
        if (!(sw_path = cov_table_path(sw_file, kfile, ".coverage_scrub_sweep"))) { fprintf(err, "coverage_depth: out of memory\n"); goto done; }
    }
    if (want_rc && h.general) {
        fprintf(err, "coverage_depth: --recurrence: %s has k-mer fields that are not A/C/G/T words of one length: a k-mer seen in two samples is not defined there\n", kfile);
        goto done;
    }
    if (want_rc && (!(rc_path = cov_table_path(rc_file, kfile, ".coverage_recurrence")) ||
                    (want_rp && !(rp_path = cov_table_path(rp_file, kfile, ".coverage_recurrence_pairs"))))) { fprintf(err, "coverage_depth: out of memory\n"); goto done; }
    if (want_sp) {
        if (sp_file && *sp_file) sp_path = strdup(sp_file);
        else if ((sp_path = malloc(strlen(kfile) + 32)) != NULL) {
            const size_t n = strlen(kfile);
            strcpy(sp_path, kfile);
            if (n >= 13 && !strcmp(sp_path + n - 13, ".kmer_hits.gz")) sp_path[n - 13] = 0;
            strcat(sp_path, ".coverage_spectrum");
        }
        if (!sp_path) { fprintf(err, "coverage_depth: out of memory\n"); goto done; }
    }
    if ((env = getenv("SK_DEVICE")) != NULL) device = atoi(env);
    rc = sk_ctx_create(&ctx, device);
    if (rc != SK_OK) { fprintf(err, "coverage_depth: cannot use HIP device %d: %s\n", device, sk_strerror(rc)); goto done; }
    status = cov_report(&h, ctx, kfile, bfile, out, err);
    if (status == 0 && want_sp) status = cov_spectrum_file(&h, ctx, kfile, (uint32_t)sp_d, sp_path, err);
    if (status == 0 && want_rc) status = cov_recurrence_files(&h, ctx, kfile, rc_path, rp_path, err);
    if (status == 0 && want_th) status = cov_thresholds_file(&h, ctx, kfile, th_path, err);
    if (status == 0 && want_sw) status = cov_sweep_file(&h, ctx, kfile, sw_cls, sw_path, err);
done:
    fflush(out);
    free(sp_path); free(rc_path); free(rp_path); free(th_path); free(sw_path); free(sw_cls);
    skc_classes_free(&sw_c);
    sk_ctx_destroy(ctx);
    hitlist_free(&h);
    return status;
}
