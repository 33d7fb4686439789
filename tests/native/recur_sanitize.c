/* recur_sanitize.c -- drives the HOST fold of recurrence (strainer2_amd/csrc/sk_host_cov.c: skc_report_recurrence and
 * skc_add_recurrence_counts; include/strainer_kmer.h has the rule) on crafted (sample, row) lists under AddressSanitizer + UBSan
 * and checks both tables, byte for byte, against a brute-force loop over a samples x rows matrix.  TEST CODE only, with its own
 * main and plain-C stand-ins for the device calls sk_host_cov.c names.  Built and run by tests/test_coverage_recurrence_host.py. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../include/strainer_kmer.h"
#include "../../strainer2_amd/csrc/sk_internal.h"

static int dummy_ctx;
int sk_ctx_create(sk_ctx **o, int d) { (void)d; *o = (sk_ctx *)&dummy_ctx; return SK_OK; }
void sk_ctx_destroy(sk_ctx *c) { (void)c; }
const char *sk_strerror(int c) { (void)c; return "stub"; }
const char *sk_last_error(const sk_ctx *c) { (void)c; return "stub"; }
int sk_first_seen_count(sk_ctx *ctx, const uint32_t *id, const uint32_t *sample, uint64_t n, uint32_t nids, uint32_t nsamples,
                        uint64_t *out_unique, uint64_t *out_total)
{
    (void)ctx; (void)id; (void)sample; (void)n; (void)nids; (void)nsamples; (void)out_unique; (void)out_total;
    return SK_E_ARG;
}
/* the main table's two numbers: a sample's passing lines and its distinct rows (rows are below 4096 here) */
int sk_distinct_count(sk_ctx *ctx, const uint64_t *keys, const uint32_t *sample, uint64_t n, uint32_t nsamples,
                      uint64_t *out_unique, uint64_t *out_total)
{
    uint8_t *seen = calloc((size_t)nsamples * 4096u + 1u, 1);
    uint64_t i;
    (void)ctx;
    memset(out_unique, 0, (size_t)nsamples * 8);
    memset(out_total, 0, (size_t)nsamples * 8);
    for (i = 0; i < n; i++) {
        uint8_t *c = &seen[(size_t)sample[i] * 4096u + (size_t)(keys[i] & 4095u)];
        out_total[sample[i]]++;
        if (!*c) { *c = 1; out_unique[sample[i]]++; }
    }
    free(seen);
    return SK_OK;
}

#define ROWS 512u
typedef struct { uint32_t sample, row; int passes; } hit;

static char *slurp(FILE *f)
{
    long n;
    char *s;
    fflush(f);
    n = ftell(f);
    rewind(f);
    s = calloc((size_t)n + 1u, 1);
    if (n && fread(s, 1, (size_t)n, f) != (size_t)n) { free(s); return NULL; }
    return s;
}

/* T samples named s<i>, every one with trailers; hits in list order.  given: the tables are handed in by
 * ordinal (the reverse of the table's order) instead of folded.  Returns 0 when both tables are the brute-force loop's. */
static int run_case(const char *what, uint32_t T, const hit *h, uint32_t nh, int64_t I, int pairs, int given)
{
    skc_acc *a = skc_create(1);
    FILE *fm = tmpfile(), *fh = tmpfile(), *fp = pairs ? tmpfile() : NULL;
    uint8_t *seen = calloc((size_t)T * ROWS + 1u, 1);
    uint32_t *pos = malloc(((size_t)T + 1u) * sizeof *pos), *at = malloc(((size_t)T + 1u) * sizeof *at), npos = 0, i, j, r;
    uint64_t *hist = calloc((size_t)T + 2u, sizeof *hist), *sh = calloc((size_t)T * T + 1u, sizeof *sh);
    char name[32], nb[32], *want = malloc(64u + (size_t)T * 64u), *wantp = malloc(128u + (size_t)T * T * 96u), *got, *gotp = NULL;
    size_t wl = 0, pl = 0;
    int bad = 0;
    for (i = 0; i < T; i++) pos[i] = T;
    for (i = 0; i < nh; i++) {                       /* the brute-force side: the table's order and the matrix */
        if (!h[i].passes) continue;
        if (pos[h[i].sample] == T) { at[npos] = h[i].sample; pos[h[i].sample] = npos++; }
        seen[(size_t)h[i].sample * ROWS + h[i].row] = 1;
    }
    for (i = 0; i < T; i++) if (pos[i] == T) { at[npos] = i; pos[i] = npos++; }     /* trailer-only samples follow */
    for (r = 0; r < ROWS; r++) {
        uint32_t m = 0;
        for (i = 0; i < T; i++) m += seen[(size_t)i * ROWS + r];
        hist[m]++;
        for (i = 0; i < T; i++)
            for (j = 0; j < T; j++)
                if (seen[(size_t)at[i] * ROWS + r] && seen[(size_t)at[j] * ROWS + r]) sh[(size_t)i * T + j]++;
    }
    /* the accumulator's side */
    if (!given)
        for (i = 0; i < nh; i++) {
            snprintf(name, sizeof name, "dir/s%u", h[i].sample);
            if (skc_add_hit(a, name, h[i].passes ? 2 : 1, 0, h[i].row)) bad = 1;
        }
    else
        for (i = 0; i < T; i++) {                    /* counts per sample, in the table's order, as strain_detect hands them in */
            uint64_t u = 0;
            for (r = 0; r < ROWS; r++) u += seen[(size_t)at[i] * ROWS + r];
            snprintf(name, sizeof name, "dir/s%u", at[i]);
            if (skc_add_counts(a, name, u, u)) bad = 1;
        }
    for (i = 0; i < T; i++) {
        snprintf(name, sizeof name, "dir/s%u", i);
        if (skc_add_trailer(a, name, "total_kmer_evaluated", 1000) || skc_add_trailer(a, name, "total_genome_informative_kmers", I)) bad = 1;
    }
    if (given) {                                     /* ordinals run against the table's order: the fold must map them */
        char **names = calloc((size_t)T + 1u, sizeof *names);
        uint64_t *gh = calloc((size_t)T + 2u, sizeof *gh), *gp = calloc((size_t)T * T + 1u, sizeof *gp);
        for (i = 0; i < T; i++) {
            names[i] = malloc(32);
            snprintf(names[i], 32, "other/s%u", at[T - 1u - i]);
            for (j = 0; j < T; j++) gp[(size_t)i * T + j] = sh[(size_t)(T - 1u - i) * T + (T - 1u - j)];
        }
        memcpy(gh, hist, ((size_t)T + 1u) * sizeof *gh);
        gh[0] = 12345;                               /* (entry 0 is not used) */
        if (skc_add_recurrence_counts(a, (const char *const *)names, T, gh, pairs ? gp : NULL)) bad = 1;
        for (i = 0; i < T; i++) free(names[i]);
        free(names); free(gh); free(gp);
    }
    if (skc_report(a, (sk_ctx *)&dummy_ctx, "x/Genus_species_z.kmer_hits.gz", fm, stderr)) bad = 1;
    if (skc_report_recurrence(a, "x/Genus_species_z.kmer_hits.gz", fh, fp, stderr)) bad = 1;
    /* the expected bytes */
    wl += (size_t)sprintf(want + wl, "strain_name\tsamples\tseen_in\tinformative_kmers\n");
    if (T) wl += (size_t)sprintf(want + wl, "Genus_species_z\t%u\t0\t%lld\n", T, (long long)(I - (int64_t)(ROWS - hist[0])));
    for (i = 1; i <= T; i++) if (hist[i]) wl += (size_t)sprintf(want + wl, "Genus_species_z\t%u\t%u\t%llu\n", T, i, (unsigned long long)hist[i]);
    pl += (size_t)sprintf(wantp + pl, "strain_name\tmetagenome_a\tmetagenome_b\tshared_informative_kmers\teither_informative_kmers\n");
    for (i = 0; i < T; i++)
        for (j = i; j < T; j++) {
            snprintf(name, sizeof name, "s%u", at[i]);
            snprintf(nb, sizeof nb, "s%u", at[j]);
            pl += (size_t)sprintf(wantp + pl, "Genus_species_z\t%s\t%s\t%llu\t%llu\n", name, nb, (unsigned long long)sh[(size_t)i * T + j],
                                  (unsigned long long)(sh[(size_t)i * T + i] + sh[(size_t)j * T + j] - sh[(size_t)i * T + j]));
        }
    got = slurp(fh);
    if (fp) gotp = slurp(fp);
    if (bad || !got || strcmp(got, want) || (fp && (!gotp || strcmp(gotp, wantp)))) {
        fprintf(stderr, "recur_sanitize: case %s%s differs\n--- got\n%s--- want\n%s", what, given ? " (handed in)" : "", got ? got : "(none)\n", want);
        bad = 1;
    }
    free(got); free(gotp); free(want); free(wantp); free(seen); free(pos); free(at); free(hist); free(sh);
    fclose(fm); fclose(fh);
    if (fp) fclose(fp);
    skc_destroy(a);
    return bad;
}

int main(void)
{
    enum { BIG = 300 };
    hit *h = malloc(sizeof *h * 50000u);
    uint32_t n, i, s;
    unsigned x = 12345u;
    int bad = 0, given;
    bad |= run_case("no sample at all", 0, h, 0, 40, 1, 0);
    for (given = 0; given < 2; given++) {
        /* an empty list: three samples that only have trailers */
        bad |= run_case("empty", 3, h, 0, 40, 1, given);
        /* one row in all samples, and nothing else */
        for (n = 0; n < 5; n++) { h[n].sample = 4u - n; h[n].row = 77; h[n].passes = 1; }
        bad |= run_case("one row everywhere", 5, h, n, 9, 1, given);
        /* duplicate pairs, lines that fail the read filter, a sample whose only lines fail it, rows 0 and ROWS - 1 */
        n = 0;
        for (i = 0; i < 3000; i++) {
            x = x * 1103515245u + 12345u;
            h[n].sample = (x >> 16) % 6u; h[n].row = (x >> 8) % 40u * 13u % ROWS; h[n].passes = h[n].sample != 5u && (x & 7u) != 0; n++;
            if ((x & 3u) == 0) { h[n] = h[n - 1]; n++; }
        }
        h[n].sample = 2; h[n].row = 0; h[n].passes = 1; n++;
        h[n].sample = 0; h[n].row = ROWS - 1u; h[n].passes = 1; n++;
        h[n] = h[n - 1]; n++;
        bad |= run_case("duplicates", 6, h, n, 600, 1, given);
        /* 300 samples: the histogram alone (more than the pair table takes), every m from 1 to 300 occurs */
        n = 0;
        for (i = 1; i <= BIG; i++)
            for (s = 0; s < i; s++) { h[n].sample = (s * 7u + i) % BIG; h[n].row = i; h[n].passes = 1; n++; }
        bad |= run_case("300 samples", BIG, h, n, 100000, 0, given);
        /* 256 samples with the pair table */
        n = 0;
        for (i = 0; i < 256u; i++)
            for (s = 0; s < 8u; s++) { h[n].sample = i; h[n].row = (i * 3u + s * s) % ROWS; h[n].passes = 1; n++; }
        bad |= run_case("256 samples", 256, h, n, 512, 1, given);
    }
    {   /* the pair table is refused above SK_RECUR_PAIRS_MAX samples: one line, non-zero, nothing printed */
        skc_acc *a = skc_create(1);
        FILE *f1 = tmpfile(), *f2 = tmpfile(), *fe = tmpfile();
        char name[32], *e;
        for (i = 0; i < 257u; i++) { snprintf(name, sizeof name, "s%u", i); (void)skc_add_hit(a, name, 5, 0, i); }
        if (!skc_report_recurrence(a, "z.kmer_hits.gz", f1, f2, fe)) { fprintf(stderr, "recur_sanitize: 257 samples with pairs were accepted\n"); bad = 1; }
        e = slurp(fe);
        if (!e || !strstr(e, "257 samples") || ftell(f1) != 0 || ftell(f2) != 0) { fprintf(stderr, "recur_sanitize: the refusal: %s\n", e ? e : ""); bad = 1; }
        free(e);
        fclose(f1); fclose(f2); fclose(fe);
        skc_destroy(a);
    }
    free(h);
    if (!bad) puts("recur_sanitize: ok");
    return bad;
}
