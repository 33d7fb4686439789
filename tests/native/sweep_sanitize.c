/* sweep_sanitize.c -- drives the HOST side of the scrub sweep (strainer2_amd/csrc/sk_host_cov.c: skc_classes_read, skc_set_classes,
 * skc_add_class_counts, skc_report_classes; strainer2_amd/csrc/sk_sweep.h: skw_parse_list; include/strainer_kmer.h has the rule) under
 * AddressSanitizer + UBSan: class files good and bad, and the fold of crafted (sample, row) lists checked, byte for byte, against a
 * brute-force loop over a samples x rows matrix.  TEST CODE only, with its own main and plain-C stand-ins for the device calls
 * sk_host_cov.c names.  Built and run by tests/test_scrub_sweep_host.py; argv[1] is a directory to write class files into. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <zlib.h>
#include "../../include/strainer_kmer.h"
#include "../../strainer2_amd/csrc/sk_internal.h"
#include "../../strainer2_amd/csrc/sk_sweep.h"

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

static void header_of(skc_classes *c, uint32_t F, const uint8_t *row_class)
{
    uint32_t q, r;
    memset(c, 0, sizeof *c);
    c->F = F;
    for (q = 0; q < F; q++) {
        snprintf(c->frac[q], sizeof c->frac[q], "0.%02u", 90u - 5u * q);
        for (r = 0; r < ROWS; r++) c->size[q] += row_class[r] >= q + 1u;
    }
}

/* T samples named s<i>, every one with trailers; hits in list order on rows whose class is row_class[row] (1..F where a passing hit
 * falls).  given: the numbers are handed in per sample instead of folded.  0 when the table is the brute-force loop's. */
static int run_case(const char *what, uint32_t T, uint32_t F, const uint8_t *row_class, const hit *h, uint32_t nh, int given)
{
    skc_acc *a = skc_create(1);
    skc_classes c;
    FILE *fm = tmpfile(), *fs = tmpfile();
    uint32_t *depth = calloc((size_t)T * ROWS + 1u, sizeof *depth);
    uint32_t *pos = malloc(((size_t)T + 1u) * sizeof *pos), *at = malloc(((size_t)T + 1u) * sizeof *at), npos = 0, i, q, r;
    char name[32], *want = malloc(256u + (size_t)T * F * 96u), *got;
    size_t wl = 0;
    int bad = 0;
    header_of(&c, F, row_class);
    if (skc_set_classes(a, &c)) bad = 1;
    for (i = 0; i < T; i++) pos[i] = T;
    for (i = 0; i < nh; i++) {                       /* the brute-force side: the table's order and the matrix */
        if (!h[i].passes) continue;
        if (pos[h[i].sample] == T) { at[npos] = h[i].sample; pos[h[i].sample] = npos++; }
        depth[(size_t)h[i].sample * ROWS + h[i].row]++;
    }
    for (i = 0; i < T; i++) if (pos[i] == T) { at[npos] = i; pos[i] = npos++; }     /* trailer-only samples follow */
    wl += (size_t)sprintf(want + wl, "strain_name\tmetagenome\tmin_fraction\tgenome_num_informative_kmers\tunique_observed_informative_kmers\t"
                                     "total_observed_informative_kmers\n");
    for (i = 0; i < T; i++) {
        uint64_t gu[SK_SCRUB_SWEEP_MAX], gt[SK_SCRUB_SWEEP_MAX], u0 = 0, t0 = 0;
        for (q = 0; q < F; q++) {
            uint64_t u = 0, t = 0;
            for (r = 0; r < ROWS; r++)
                if (depth[(size_t)at[i] * ROWS + r] && row_class[r] >= q + 1u) { u++; t += depth[(size_t)at[i] * ROWS + r]; }
            gu[q] = u; gt[q] = t;
            wl += (size_t)sprintf(want + wl, "Genus_species_z\ts%u\t%s\t%llu\t%llu\t%llu\n", at[i], c.frac[q], (unsigned long long)c.size[q],
                                  (unsigned long long)u, (unsigned long long)t);
        }
        if (given) {
            for (r = 0; r < ROWS; r++) if (depth[(size_t)at[i] * ROWS + r]) { u0++; t0 += depth[(size_t)at[i] * ROWS + r]; }
            snprintf(name, sizeof name, "dir/s%u", at[i]);
            if (skc_add_counts(a, name, u0, t0) || skc_add_class_counts(a, name, gu, gt, F)) bad = 1;
            if (!skc_add_class_counts(a, name, gu, gt, F + 1u)) bad = 1;             /* (another list's length is refused) */
        }
    }
    if (!given)
        for (i = 0; i < nh; i++) {
            snprintf(name, sizeof name, "dir/s%u", h[i].sample);
            if (skc_add_hit(a, name, h[i].passes ? 2 : 1, 0, h[i].row)) bad = 1;
        }
    for (i = 0; i < T; i++) {
        snprintf(name, sizeof name, "dir/s%u", i);
        if (skc_add_trailer(a, name, "total_kmer_evaluated", 1000) || skc_add_trailer(a, name, "total_genome_informative_kmers", (int64_t)c.size[0])) bad = 1;
    }
    if (skc_report(a, (sk_ctx *)&dummy_ctx, "x/Genus_species_z.kmer_hits.gz", fm, stderr)) bad = 1;
    if (skc_report_classes(a, "x/Genus_species_z.kmer_hits.gz", row_class, ROWS, fs, stderr)) bad = 1;
    if (skc_report_classes(a, "x/Genus_species_z.kmer_hits.gz", row_class, ROWS, fs, stderr)) bad = 1;      /* a second report: the same table again */
    got = slurp(fs);
    if (bad || !got || strlen(got) != 2u * wl || strncmp(got, want, wl) || strcmp(got + wl, want)) {
        fprintf(stderr, "sweep_sanitize: case %s%s differs\n--- got (twice)\n%s--- want\n%s", what, given ? " (handed in)" : "", got ? got : "(none)\n", want);
        bad = 1;
    }
    free(got); free(want); free(depth); free(pos); free(at);
    fclose(fm); fclose(fs);
    skc_destroy(a);
    return bad;
}

static int put_file(const char *path, const char *text, int gz)
{
    if (gz) {
        gzFile g = gzopen(path, "wb");
        if (!g || gzputs(g, text) < 0) return 1;
        return gzclose(g) != Z_OK;
    } else {
        FILE *f = fopen(path, "w");
        if (!f || fputs(text, f) < 0) return 1;
        return fclose(f) != 0;
    }
}

/* a class file with this text is read (expect = NULL) or refused with `expect` in the reason */
static int file_case(const char *dir, const char *what, const char *text, int gz, const char *expect)
{
    char path[600], why[240] = "";
    skc_classes c;
    int rc, bad = 0;
    snprintf(path, sizeof path, "%s/%s%s", dir, what, gz ? ".classes.gz" : ".classes");
    if (text && put_file(path, text, gz)) { fprintf(stderr, "sweep_sanitize: could not write %s\n", path); return 1; }
    rc = skc_classes_read(path, &c, why, sizeof why);
    if (expect ? (rc == 0 || !strstr(why, expect)) : rc != 0) {
        fprintf(stderr, "sweep_sanitize: class file %s: rc %d, reason '%s', expected %s\n", what, rc, why, expect ? expect : "success");
        bad = 1;
    }
    if (!rc && !expect) {
        if (c.F != 3 || strcmp(c.frac[0], "0.5") || strcmp(c.frac[2], "1e-2") || c.size[0] != 3 || c.size[2] != 1 || c.n != 3 ||
            strcmp(c.arena + c.off[1], "CCCA") || c.cls[0] != 1 || c.cls[1] != 3 || c.cls[2] != 2) {
            fprintf(stderr, "sweep_sanitize: class file %s was read wrongly\n", what);
            bad = 1;
        }
    }
    skc_classes_free(&c);
    return bad;
}

int main(int argc, char **argv)
{
    hit *h = malloc(sizeof *h * 20000u);
    uint8_t cls[ROWS];
    uint32_t n, i, F;
    unsigned x = 2024u;
    int bad = 0, given;
    const char *dir = argc > 1 ? argv[1] : ".";
    static const char good[] = "#min_fractions\t0.5,0.04,1e-2\n#post_scrub_kmers\t3,2,1\nAAAC\t1\nCCCA\t3\nGGGT\t2\n";
    char *longline = malloc(3000);
    skw_list l;
    char why[160];

    /* the list's rule */
    bad |= skw_parse_list("1,0.5,0", &l, why, sizeof why) || l.n != 3 || strcmp(l.text[1], "0.5") || l.f[0] != 1.0;
    bad |= skw_parse_list("0.04", &l, why, sizeof why) || l.n != 1;
    {
        static const char *const refused[] = { "", ",", "0.5,", ",0.5", "0.5,,0.1", "0.5,0.5", "0.1,0.5", "1.5", "-0.1", "abc", "0.5x", "nan", " 0.5",
                                               "0.9,0.8,0.7,0.6,0.5,0.4,0.3,0.2,0.1,0.09,0.08,0.07,0.06,0.05,0.04,0.03,0.02",
                                               "0.00000000000000000000000000000000000000000000000000000000000001" };
        for (i = 0; i < sizeof refused / sizeof *refused; i++)
            if (!skw_parse_list(refused[i], &l, why, sizeof why) || !why[0]) { fprintf(stderr, "sweep_sanitize: the list '%s' was accepted\n", refused[i]); bad = 1; }
    }

    /* class files */
    bad |= file_case(dir, "good", good, 0, NULL);
    bad |= file_case(dir, "good", good, 1, NULL);
    bad |= file_case(dir, "no_newline", "#min_fractions\t0.5,0.04,1e-2\n#post_scrub_kmers\t3,2,1\nAAAC\t1\nCCCA\t3\nGGGT\t2", 0, NULL);
    bad |= file_case(dir, "missing", NULL, 0, "could not read");
    bad |= file_case(dir, "empty", "", 0, "header");
    bad |= file_case(dir, "one_header", "#min_fractions\t0.5\n", 0, "header");
    bad |= file_case(dir, "no_header", "AAAC\t1\n", 0, "first line");
    bad |= file_case(dir, "headers_swapped", "#post_scrub_kmers\t1\n#min_fractions\t0.5\nAAAC\t1\n", 0, "first line");
    bad |= file_case(dir, "bad_list", "#min_fractions\t0.5,0.6\n#post_scrub_kmers\t1,1\nAAAC\t2\n", 0, "fraction list");
    bad |= file_case(dir, "sizes_short", "#min_fractions\t0.5,0.1\n#post_scrub_kmers\t1\nAAAC\t2\n", 0, "second line");
    bad |= file_case(dir, "sizes_long", "#min_fractions\t0.5,0.1\n#post_scrub_kmers\t1,1,1\nAAAC\t2\n", 0, "second line");
    bad |= file_case(dir, "sizes_grow", "#min_fractions\t0.5,0.1\n#post_scrub_kmers\t1,2\nAAAC\t2\n", 0, "second line");
    bad |= file_case(dir, "sizes_text", "#min_fractions\t0.5,0.1\n#post_scrub_kmers\t1,x\nAAAC\t2\n", 0, "second line");
    bad |= file_case(dir, "class_0", "#min_fractions\t0.5,0.1\n#post_scrub_kmers\t1,1\nAAAC\t0\n", 0, "class from 1 to 2");
    bad |= file_case(dir, "class_3", "#min_fractions\t0.5,0.1\n#post_scrub_kmers\t1,1\nAAAC\t3\n", 0, "class from 1 to 2");
    bad |= file_case(dir, "class_text", "#min_fractions\t0.5,0.1\n#post_scrub_kmers\t1,1\nAAAC\tx\n", 0, "class from 1 to 2");
    bad |= file_case(dir, "no_tab", "#min_fractions\t0.5,0.1\n#post_scrub_kmers\t1,1\nAAAC 2\n", 0, "class from 1 to 2");
    bad |= file_case(dir, "two_tabs", "#min_fractions\t0.5,0.1\n#post_scrub_kmers\t1,1\nAAAC\t2\t2\n", 0, "class from 1 to 2");
    bad |= file_case(dir, "no_kmer", "#min_fractions\t0.5,0.1\n#post_scrub_kmers\t1,1\n\t2\n", 0, "class from 1 to 2");
    bad |= file_case(dir, "count_off", "#min_fractions\t0.5,0.1\n#post_scrub_kmers\t2,1\nAAAC\t2\n", 0, "header says");
    bad |= file_case(dir, "count_off_gz", "#min_fractions\t0.5,0.1\n#post_scrub_kmers\t2,2\nAAAC\t2\nAAAG\t1\n", 1, "header says");
    memset(longline, 'A', 2999);
    longline[2999] = 0;
    memcpy(longline, "#min_fractions\t0.5\n#post_scrub_kmers\t1\n", 39);
    bad |= file_case(dir, "long_line", longline, 0, "too long");
    free(longline);

    /* the fold */
    for (F = 1; F <= SK_SCRUB_SWEEP_MAX; F += (F == 1 ? 1 : 14)) {          /* 1, 2 and 16 fractions */
        for (i = 0; i < ROWS; i++) cls[i] = (uint8_t)(i % (F + 1u));        /* class 0 rows: never hit below */
        cls[ROWS - 1u] = (uint8_t)F;
        cls[1] = 1;
        for (given = 0; given < 2; given++) {
            bad |= run_case("no sample at all", 0, F, cls, h, 0, given);
            bad |= run_case("empty", 3, F, cls, h, 0, given);
            n = 0;
            for (i = 0; i < 4000; i++) {
                x = x * 1103515245u + 12345u;
                h[n].sample = (x >> 16) % 6u; h[n].row = (x >> 8) % ROWS; h[n].passes = h[n].sample != 5u && (x & 7u) != 0;
                if (!cls[h[n].row]) h[n].row = 1;
                n++;
                if ((x & 3u) == 0) { h[n] = h[n - 1]; n++; }
            }
            h[n].sample = 2; h[n].row = 1; h[n].passes = 1; n++;
            h[n].sample = 0; h[n].row = ROWS - 1u; h[n].passes = 1; n++;
            h[n] = h[n - 1]; n++;
            bad |= run_case("duplicates", 6, F, cls, h, n, given);
        }
    }
    {   /* a hit on a row in none of the sets, and on a row beyond the strain's: one line, non-zero, nothing printed */
        for (i = 0; i < 2; i++) {
            skc_acc *a = skc_create(1);
            skc_classes c;
            FILE *fm = tmpfile(), *fs = tmpfile(), *fe = tmpfile();
            char *e;
            memset(cls, 0, sizeof cls);
            cls[7] = 1;
            header_of(&c, 1, cls);
            (void)skc_set_classes(a, &c);
            (void)skc_add_hit(a, "m", 5, 0, 7);
            (void)skc_add_hit(a, "m", 5, 0, i ? ROWS + 3u : 8u);
            (void)skc_report(a, (sk_ctx *)&dummy_ctx, "z.kmer_hits.gz", fm, stderr);
            if (!skc_report_classes(a, "z.kmer_hits.gz", cls, ROWS, fs, fe)) { fprintf(stderr, "sweep_sanitize: a stray hit was accepted\n"); bad = 1; }
            e = slurp(fe);
            if (!e || !strstr(e, "none of the scrub sweep's sets") || strchr(e, '\n') != e + strlen(e) - 1 || ftell(fs) != 0) { fprintf(stderr, "sweep_sanitize: the refusal: %s\n", e ? e : ""); bad = 1; }
            free(e);
            fclose(fm); fclose(fs); fclose(fe);
            skc_destroy(a);
        }
        {
            skc_acc *a = skc_create(1);
            FILE *fs = tmpfile();
            if (!skc_report_classes(a, "z.kmer_hits.gz", cls, ROWS, fs, stderr) || ftell(fs) != 0) { fprintf(stderr, "sweep_sanitize: a report without classes\n"); bad = 1; }
            fclose(fs);
            skc_destroy(a);
        }
    }
    free(h);
    if (!bad) puts("sweep_sanitize: ok");
    return bad;
}
