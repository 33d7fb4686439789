/* sk_host_scrub_multi.c -- kmer_scrub_count -S: step 1 of the workflow for many strains over ONE pass of the -A/-B/-C lists.
 *
 * The reference counts one strain per process (src/kmer_scrub_count.c:29-131); a drug with 8-32 strains re-reads, re-decodes
 * and re-uploads the same lists once per strain.  Here up to SK_UNION_MAX strains are resident at once and share one union table
 * (sk_union_*): each list is scanned once into the union's count column, and sk_union_counts_fold hands the counts to every
 * member's own column.  The -C rule (a line equal to the run's -r is not counted: src/genome_compare.c:115-146) is per strain:
 * the whole -C list goes to every member, then each line equal to a member's genome is scanned alone and taken back from the
 * members it names (u32 wrap makes -= after += exact).  A strain the union cannot hold (byte-string keys, no text stage) gets a
 * pass of its own through its own context, as the single-strain program would run it.
 *
 * More strains than one union holds make several unions, and the lists are decoded ONCE for all of them: every union is made
 * first, as many as fit in HBM next to the strains' own tables (an estimate of each union's bytes against the free memory less a
 * reserve; SK_SCRUB_HBM_MB stands in for the free memory, SK_SCRUB_UNIONS caps the unions per decode, 1 = one decode per union
 * as before), then one walk of -A, -B and -C (skh_scan_list_many) uploads each chunk once and scans it into every union, and
 * each union folds after each list.  A union that cannot be made next to the others closes the set -- nothing has been scanned
 * into it yet -- and the remaining groups get a decode of their own.  Outfiles, stderr and the progress file are what one pass
 * per union wrote; the -C "skipping" lines come union by union as before.
 *
 * With --scrub <min_fraction> [--independent] --detect <strain_detect arguments> each strain goes on into step 2 on its resident
 * counts (skh_scrub_filter_resident, sk_filter on the device) and its line names an informative outfile and a hit list instead of
 * a count table; then the strains go on together into step 3 (and 4) on the same resident tables: skh_strain_detect_resident_many,
 * strain_detect -S's machinery with the tables of step 1 taken over instead of rebuilt.  --scrub without --detect stays refused,
 * as before this mode existed (run the strains one by one for the informative lists alone).
 *
 * With --prevalence=SUFFIX [--prevalence-items=SUFFIX] [--prevalence-min-count m] every strain also gets its prevalence table and
 * item records beside its outfile (<outfile><SUFFIX>), byte for byte the single-strain program's: the members are loaded with three
 * more columns behind their own, every resident union gets its item slots ONCE per decode (sk_item_slots on its context, kept
 * across -A, -B, -C), the walk (skh_scan_list_many_prevalence) names a slot on every union before each submit, and where an item ends
 * sm_item_fold_hook enqueues every union's sk_union_item_fold.  The per-strain -C rule is that fold's member mask, so sm_union_skips'
 * rescans are not run with the flag on -- only its "skipping" lines are printed, at their place.  A strain the union cannot hold
 * takes skh_scan_list_prevalence on its own context.  --scrub f --scrub-by prevalence --detect .. ranks step 2 by those columns.
 *
 * Kept in a translation unit of its own: the host tests link sk_host.c, sk_host_sd.c and sk_host_cov.c against a device
 * double that has none of the union's COUNT entry points. */
#define _GNU_SOURCE
#include <pthread.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include <unistd.h>
#include "../../include/strainer_kmer.h"
#include "sk_cpus.h"
#include "sk_gzout.h"
#include "sk_internal.h"
#include "sk_sweep.h"
#pragma weak skh_resident_genomes_
#pragma weak skh_scrub_filter_resident_sweep

typedef struct {
    char      *genome, *outfile;   /* outfile: the count table, or with --scrub the informative list                        */
    char      *hits, *glist, *cov; /* --detect: the hit list, the -g list (or NULL), the --coverage-depth table (or NULL)    */
    FILE      *fp;                 /* the outfile (plain) ...                                    */
    skzo_file *zo;                 /* ... or its gzip writer (a name ending in .gz)              */
    skh_keyset ks;
    sk_ctx    *ctx;
    int        rc_keys, rc_ctx, rc_load;
    int        print_rc;
    char      *err_buf;            /* --scrub: what the filter said, replayed in list order */
    size_t     err_len;
    unsigned   made;               /* the files this run created: 1 outfile, 2 hits, 4 coverage table, 8 prevalence table, 16 item records */
    char      *prev_path, *items_path;     /* --prevalence=SUFFIX, --prevalence-items=SUFFIX: <outfile><SUFFIX> (or NULL)        */
    skh_prev_items pitems[3];      /* ... this strain's items of -A, -B, -C (a -C line equal to its genome is none)              */
} sm_strain;

typedef struct {
    sm_strain *st;
    uint32_t   n;
    int        device, with_drug, ncols;
    double     scrub_fraction;     /* >= 0: step 2 instead of the table */
    const char *scrub_list;        /* --scrub f0,f1,...: the scrub sweep -- each strain's class file goes to <informative outfile>.classes */
    int        independent;
    int        prev, scrub_by_prev;/* --prevalence=SUFFIX: the three prevalence columns lie behind the table's own, from prev_base */
    uint32_t   prev_base, prev_min;
    uint32_t   next;               /* pool: the next strain to take */
    pthread_mutex_t mu;
} sm_job;

static double sm_now(void) { struct timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec; }

static int sm_env_int(const char *a, const char *b, const char *c3, int dflt)
{
    const char *v = getenv(a);
    if (!v && b) v = getenv(b);
    if (!v && c3) v = getenv(c3);
    return v ? atoi(v) : dflt;
}

static int sm_threads(void)
{
    const char *e = getenv("SK_THREADS");
    long n = e ? atol(e) : sk_cpu_budget();
    return n < 1 ? 1 : n > 16 ? 16 : (int)n;
}

/* run fn on every strain, `nth` threads taking the next one */
static void sm_pool_run(sm_job *j, int nth, void *(*worker)(void *))
{
    pthread_t th[16];
    int k, started = 0;
    j->next = 0;
    pthread_mutex_init(&j->mu, NULL);
    if (nth > (int)j->n) nth = (int)j->n;
    for (k = 0; k < nth; k++) if (pthread_create(&th[started], NULL, worker, j) == 0) started++;
    if (!started) worker(j);
    for (k = 0; k < started; k++) pthread_join(th[k], NULL);
    pthread_mutex_destroy(&j->mu);
}

static sm_strain *sm_take(sm_job *j)
{
    sm_strain *s = NULL;
    pthread_mutex_lock(&j->mu);
    if (j->next < j->n) s = &j->st[j->next++];
    pthread_mutex_unlock(&j->mu);
    return s;
}

/* a strain opened start to finish on one worker: host key set in the reference's row order, context, table load */
static void *sm_open_worker(void *arg)
{
    sm_job *j = (sm_job *)arg;
    sm_strain *s;
    while ((s = sm_take(j)) != NULL) {
        s->rc_keys = skh_keyset_from_file(&s->ks, s->genome, SK_REF_TABLE_SLOTS, 1, 1);
        if (s->rc_keys != SK_OK) continue;
        s->rc_ctx = sk_ctx_create(&s->ctx, j->device);
        if (s->rc_ctx != SK_OK) { s->ctx = NULL; continue; }
        s->rc_load = skh_keyset_load(s->ctx, &s->ks, (uint32_t)j->ncols);     /* (strain_detect's table has six columns) */
    }
    return NULL;
}

#define SM_FILTER_FAILED 1          /* (print_rc of a strain whose filter said why itself) */

static ssize_t sm_gz_write(void *cookie, const char *buf, size_t n)
{
    skzo_append((skzo_file *)cookie, buf, n);
    return (ssize_t)n;
}

#define SM_PREV_WRITE_FAILED  2     /* (print_rc of a strain whose prevalence table could not be written ...) */
#define SM_ITEMS_WRITE_FAILED 3     /* (... or its item records) */

/* a strain's prevalence table and its items' records, the bytes `-r <genome> --prevalence=F --prevalence-items=G` writes to F and G
 * (skh_kmer_scrub_count_main) */
static int sm_print_prevalence(const sm_job *j, sm_strain *s)
{
    const uint32_t from[4] = {0, j->prev_base, j->prev_base + 1, j->prev_base + 2};
    char extra[160];
    FILE *pf = fopen(s->prev_path, "w");
    int rc;
    if (!pf) return SM_PREV_WRITE_FAILED;
    setvbuf(pf, NULL, _IOFBF, 1 << 20);
    snprintf(extra, sizeof extra, "#items\t%u\t%u\t%u\n#min_count\t%u\n", s->pitems[0].n, s->pitems[1].n, s->pitems[2].n, j->prev_min);
    rc = skh_print_table_cols_(s->ctx, &s->ks, pf, j->with_drug, from, extra);
    if (fclose(pf) != 0 && rc == SK_OK) rc = SM_PREV_WRITE_FAILED;
    if (rc != SK_OK) return rc;
    if (s->items_path) {
        uint32_t l, k;
        if (!(pf = fopen(s->items_path, "w"))) return SM_ITEMS_WRITE_FAILED;
        fputs("#list\tline\tfile\tbases\tkmers_present\tkmer_hits\n", pf);
        for (l = 0; l < 3; l++)
            for (k = 0; k < s->pitems[l].n; k++) {
                const skh_prev_item *t = &s->pitems[l].item[k];
                fprintf(pf, "%c\t%u\t%s\t%llu\t%llu\t%llu\n", "ABC"[l], t->line, t->path, (unsigned long long)t->bases,
                        (unsigned long long)t->kmers_present, (unsigned long long)t->kmer_hits);
            }
        if (fclose(pf) != 0) return SM_ITEMS_WRITE_FAILED;
    }
    return SK_OK;
}

static void *sm_print_worker(void *arg)
{
    sm_job *j = (sm_job *)arg;
    sm_strain *s;
    while ((s = sm_take(j)) != NULL) {
        FILE *f = s->fp;
        if (s->zo) {
            cookie_io_functions_t io = {NULL, sm_gz_write, NULL, NULL};
            f = fopencookie(s->zo, "w", io);
            if (!f) { s->print_rc = SK_E_NOMEM; continue; }
        }
        setvbuf(f, NULL, _IOFBF, 1 << 20);
        if (j->scrub_fraction >= 0.0) {              /* step 2: the informative list, as `-r <genome> ... --scrub f` prints it */
            FILE *me = open_memstream(&s->err_buf, &s->err_len);
            char *cp = j->scrub_list ? (char *)malloc(strlen(s->outfile) + 9) : NULL;
            if (cp) { strcpy(cp, s->outfile); strcat(cp, ".classes"); }
            const uint32_t pcols[3] = {j->prev_base, j->prev_base + 1, j->prev_base + 2};
            s->print_rc = (j->scrub_list ? (!cp || skh_scrub_filter_resident_sweep(s->ctx, &s->ks, j->with_drug, j->scrub_list, j->independent, cp, f, me ? me : stderr))
                           : j->scrub_by_prev ? skh_scrub_filter_resident_cols(s->ctx, &s->ks, j->with_drug, pcols, j->scrub_fraction, j->independent, f, me ? me : stderr)
                                         : skh_scrub_filter_resident(s->ctx, &s->ks, j->with_drug, j->scrub_fraction, j->independent, f, me ? me : stderr))
                              ? SM_FILTER_FAILED : SK_OK;
            free(cp);
            if (me) fclose(me);
        } else s->print_rc = skh_print_counts(s->ctx, &s->ks, f, j->with_drug);
        if (s->zo) { if (fclose(f) != 0 && s->print_rc == SK_OK) s->print_rc = SK_E_OPEN; }
        else if (fflush(f) != 0 && s->print_rc == SK_OK) s->print_rc = SK_E_OPEN;
        if (j->prev && s->print_rc == SK_OK) s->print_rc = sm_print_prevalence(j, s);
    }
    return NULL;
}

/* --prevalence=SUFFIX for the passes: the first of the three prevalence columns, the threshold, the item slots every resident
 * union of a decode has (made once per decode, kept across -A, -B, -C), and what SK_TIMING reports of them */
typedef struct { uint32_t base, min, nslots; int timing; double slot_mb, fold_ms; uint64_t folds; } sm_prev;

/* one strain, its own pass: what the single-strain program does (src/kmer_scrub_count.c:87-99) */
static int sm_single_pass(sm_strain *s, const char *A, const char *B, const char *C, FILE *progress, FILE *err, uint64_t *bases,
                          const sm_prev *pv)
{
    if (pv) {                                        /* (with prevalence: the single-strain program's walk, on this strain's own context) */
        if (skh_scan_list_prevalence(s->ctx, A, NULL, 1, pv->base, pv->min, &s->pitems[0], progress, err, 0, 1, bases) != SK_OK) return 1;
        if (skh_scan_list_prevalence(s->ctx, B, NULL, 2, pv->base + 1, pv->min, &s->pitems[1], progress, err, 0, 1, bases) != SK_OK) return 1;
        if (C && skh_scan_list_prevalence(s->ctx, C, s->genome, 3, pv->base + 2, pv->min, &s->pitems[2], progress, err, 0, 1, bases) != SK_OK) return 1;
        return 0;
    }
    if (skh_scan_list(s->ctx, A, NULL, 1, progress, err, 0, 1, bases) != SK_OK) return 1;
    if (skh_scan_list(s->ctx, B, NULL, 2, progress, err, 0, 1, bases) != SK_OK) return 1;
    if (C && skh_scan_list(s->ctx, C, s->genome, 3, progress, err, 0, 1, bases) != SK_OK) return 1;
    return 0;
}

#define SM_FALLBACK 2
#define SM_LATER    3

static int sm_fold(sk_union *u, uint32_t col, uint32_t mask, int subtract, FILE *err)
{
    const int rc = sk_union_counts_fold(u, 0, col, mask, subtract);
    if (rc != SK_OK) fprintf(err, "kmer_scrub_count: union fold failed: %s (%s)\n", sk_strerror(rc), sk_union_last_error(u));
    return rc;
}

/* a union of up to SK_UNION_MAX strains with its count column, resident while one decode of the lists feeds it */
typedef struct { sk_union *u; sm_strain **g; uint32_t n; } sm_union;

static uint32_t sm_all(uint32_t n) { return n >= 32 ? 0xFFFFFFFFu : (1u << n) - 1u; }

/* What a union of these strains will hold in HBM (sk_union_create + sk_union_count_enable): slots at half
 * load, keys, masks, the row map, the count column and its difference array, the two filter levels, the texts and their rank maps,
 * and the staging ring of its -C rescans.  An estimate from the layout, not a measurement. */
static uint64_t sm_union_bytes(sm_strain *const *g, uint32_t n, uint32_t item_slots)
{
    uint64_t rows = 0, bases = 0, slots = 1024, g2 = 4096;
    uint32_t k;
    for (k = 0; k < n; k++) { rows += g[k]->ks.nrows; bases += ((uint64_t)g[k]->ks.text_bases + 63u) / 64u * 64u + 64u; }
    while (slots < 2 * rows) slots <<= 1;
    while (g2 < rows * 32) g2 <<= 1;
    return slots * 16 + rows * 33 + g2 / 8 + bases / 2 + (128ull << 20) + (uint64_t)item_slots * rows * 8;     /* (item slots: --prevalence=SUFFIX) */
}

/* the union of one group with its count column.  SM_FALLBACK: a member it cannot hold (SK_E_STATE) -- the caller runs the strains
 * one by one.  SM_LATER: it did not fit next to the unions already made (`others`): nothing is lost, no list has been scanned into
 * them yet -- the caller decodes the lists for those and makes this one again afterwards */
static int sm_union_make(sm_strain **g, uint32_t n, int others, sk_union **out, FILE *err, uint32_t *item_slots)
{
    sk_ctx *m[SK_UNION_MAX];
    sk_union *u = NULL;
    uint32_t k;
    int rc;
    *out = NULL;
    for (k = 0; k < n; k++) m[k] = g[k]->ctx;
    rc = sk_union_create(m, n, 0, 0, &u);
    if (rc == SK_E_STATE) return SM_FALLBACK;
    if (rc != SK_OK) {
        if (others) return SM_LATER;
        fprintf(err, "kmer_scrub_count: union table failed: %s (%s)\n", sk_strerror(rc), sk_last_error(m[0]));
        return 1;
    }
    if ((rc = sk_union_count_enable(u, 1)) != SK_OK) {
        if (!others) fprintf(err, "kmer_scrub_count: union count column failed: %s (%s)\n", sk_strerror(rc), sk_union_last_error(u));
        sk_union_destroy(u);
        return others ? SM_LATER : 1;
    }
    if (item_slots) {
        /* the item slots, ONCE for all the lists of the decode (8 bytes x global rows each): as many as the walk has threads, or the
         * most that fit -- with fewer, a decode thread owns a slot and the other items wait; a union without room for one closes the
         * set as a failed count column does (sk_item_slots leaves no HIP error behind) */
        uint32_t want = *item_slots;
        while (want >= 1 && (rc = sk_item_slots(sk_union_context(u), want)) == SK_E_NOMEM) want /= 2;
        if (rc != SK_OK || want < 1) {
            if (!others) fprintf(err, "kmer_scrub_count: no room for an item slot of the union (--prevalence): %s (%s)\n", sk_strerror(rc), sk_union_last_error(u));
            sk_union_destroy(u);
            return others ? SM_LATER : 1;
        }
        *item_slots = want;
    }
    *out = u;
    return 0;
}

/* the -C lines a union's member would have skipped: scanned alone and taken back from that member (a line may come several times) */
static int sm_union_skips(const sm_union *r, const char *C, FILE *err)
{
    sk_ctx *uc = sk_union_context(r->u);
    FILE *fp;
    char *line = NULL, *nl;
    size_t cap = 0;
    uint32_t k;
    int rc = SK_OK;
    if (!(fp = fopen(C, "r"))) { fprintf(err, "could not read file %s in GEN_all_kmer_counts()\n", C); return 1; }
    while (rc == SK_OK && getline(&line, &cap, fp) != -1) {
        uint32_t mask = 0;
        if ((nl = strchr(line, '\n')) != NULL) *nl = '\0';
        for (k = 0; k < r->n; k++) if (strcmp(r->g[k]->genome, line) == 0) mask |= 1u << k;
        if (!mask) continue;
        rc = skh_scan_file(uc, line, 0, NULL);
        if (rc == SK_E_OPEN) fprintf(err, "could not read file %s in GEN_calculate_kmer_count()\n", line);
        else if (rc != SK_OK) fprintf(err, "kmer_scrub_count: device error while scanning %s: %s (%s)\n", line, sk_strerror(rc), sk_last_error(uc));
        if (rc == SK_OK) rc = sm_fold(r->u, 3, mask, 1, err);
        for (k = 0; rc == SK_OK && k < r->n; k++) if ((mask >> k) & 1u) fprintf(err, "skipping %s (identical match)\n", line);
    }
    free(line);
    fclose(fp);
    return rc != SK_OK;
}

/* ONE decode of the lists for every resident union: each chunk goes up once and is scanned into every union's column 0
 * (skh_scan_list_many), and after each list every union folds it into its members' column.  Then the -C lines equal to a member,
 * union by union in group order -- the order in which one pass per group said its "skipping" lines. */
static int sm_decode(const sm_union *r, uint32_t nr, const char *A, const char *B, const char *C, FILE *progress, FILE *err,
                     double *fold_ms, uint64_t *bases)
{
    sk_ctx **uc = (sk_ctx **)malloc((size_t)nr * sizeof *uc);
    const char *list[3] = {A, B, C};
    uint32_t i, l;
    double t;
    if (!uc) { fprintf(err, "kmer_scrub_count: out of memory\n"); return 1; }
    for (i = 0; i < nr; i++) uc[i] = sk_union_context(r[i].u);
    for (l = 0; l < 3 && list[l]; l++) {
        if (skh_scan_list_many(uc, nr, list[l], NULL, 0, progress, err, 0, 1, bases) != SK_OK) break;
        t = sm_now();
        for (i = 0; i < nr; i++) if (sm_fold(r[i].u, l + 1, sm_all(r[i].n), 0, err) != SK_OK) break;
        if (i < nr) break;
        if (l < 2) *fold_ms += 1e3 * (sm_now() - t);
    }
    free(uc);
    if (l < 3 && list[l]) return 1;
    for (i = 0; C && i < nr; i++) if (sm_union_skips(&r[i], C, err)) return 1;
    return 0;
}

/* ---- the decode with --prevalence=SUFFIX.  Every scan of the walk goes into an item slot of every union
 * (skh_scan_list_many_prevalence), and where an item ends every union folds that slot into its members (sk_union_item_fold):
 * the count column, the prevalence column and the record cell of (line, union, member).  The -C rule is the fold's member mask: a
 * line equal to a member's genome is folded into everybody but that member, so it is no item of that strain -- no record, not in
 * its nC, nothing in either column.  The count column is still the flag-off column bit for bit: there the line is added to every
 * member and taken back from the one (sm_union_skips), and in integer adds mod 2^32 "never added" equals "added and taken back". */
typedef struct {
    const sm_union *r; uint32_t nr;
    uint32_t col, prev_col, min;
    char **line; uint32_t nline; int is_c;
    uint64_t **d_rec;                   /* per union, device: [line][member] {kmers_present, kmer_hits} */
    FILE *err;
} sm_fold_job;

static int sm_item_fold_hook(void *user, uint32_t slot, uint32_t line)
{
    const sm_fold_job *j = (const sm_fold_job *)user;
    uint32_t i, k;
    if (line >= j->nline) return SK_E_ARG;           /* (the walk read more lines than this run did: the list changed under it) */
    for (i = 0; i < j->nr; i++) {
        const sm_union *r = &j->r[i];
        uint32_t mask = sm_all(r->n);
        int rc;
        for (k = 0; j->is_c && k < r->n; k++) if (strcmp(r->g[k]->genome, j->line[line]) == 0) mask &= ~(1u << k);
        rc = sk_union_item_fold(r->u, slot, j->col, j->prev_col, mask, j->min, j->d_rec[i] + ((size_t)line * r->n) * 2u);
        if (rc != SK_OK) return rc;
    }
    return SK_OK;
}

static void sm_lines_free(char **line, uint32_t n)
{
    uint32_t t;
    for (t = 0; line && t < n; t++) free(line[t]);
    free(line);
}

/* the list's lines as the walk reads them.  NULL with *oom 0: not readable (the walk says so); NULL with *oom 1: out of memory */
static char **sm_list_lines(const char *path, uint32_t *n, int *oom)
{
    FILE *fp = fopen(path, "r");
    char **out = (char **)malloc(sizeof *out), *line = NULL, *nl;
    size_t cap = 0;
    *n = 0; *oom = 0;
    if (!fp || !out) { *oom = fp != NULL; if (fp) fclose(fp); free(out); return NULL; }
    while (getline(&line, &cap, fp) != -1) {
        char **grown = (char **)realloc(out, ((size_t)*n + 2) * sizeof *out);
        if (grown) out = grown;
        if ((nl = strchr(line, '\n')) != NULL) *nl = '\0';
        if (!grown || !(out[*n] = strdup(line))) { *oom = 1; break; }
        (*n)++;
    }
    free(line);
    fclose(fp);
    if (*oom) { sm_lines_free(out, *n); *n = 0; return NULL; }
    return out;
}

static int sm_decode_prev(const sm_union *r, uint32_t nr, const char *A, const char *B, const char *C, FILE *progress, FILE *err,
                          uint64_t *bases, sm_prev *pv)
{
    sk_ctx **uc = (sk_ctx **)malloc((size_t)nr * sizeof *uc);
    const char *list[3] = {A, B, C};
    uint32_t i, k, l, t, c_nline = 0;
    char **c_line = NULL;                            /* -C's lines, kept for the "skipping" lines: the list is read ONCE */
    int failed = 0;
    if (!uc) { fprintf(err, "kmer_scrub_count: out of memory\n"); return 1; }
    for (i = 0; i < nr; i++) uc[i] = sk_union_context(r[i].u);
    if (pv->timing) (void)sk_item_fold_timing_(uc[0], 1, NULL, NULL);
    for (l = 0; l < 3 && list[l] && !failed; l++) {
        sm_fold_job j;
        skh_prev_items walked = {NULL, 0};
        uint64_t **h_rec = (uint64_t **)calloc(nr, sizeof *h_rec);
        int rc = SK_OK, oom = 0;
        memset(&j, 0, sizeof j);
        j.r = r; j.nr = nr; j.col = l + 1; j.prev_col = pv->base + l; j.min = pv->min; j.is_c = l == 2; j.err = err;
        j.line = sm_list_lines(list[l], &j.nline, &oom);
        j.d_rec = (uint64_t **)calloc(nr, sizeof *j.d_rec);
        if (!h_rec || !j.d_rec || oom) rc = SK_E_NOMEM;
        for (i = 0; rc == SK_OK && j.line && i < nr; i++) {      /* the record cells, zeroed */
            const size_t bytes = ((size_t)j.nline * r[i].n + 1) * 2u * sizeof(uint64_t);
            if (!(h_rec[i] = (uint64_t *)calloc(1, bytes))) { rc = SK_E_NOMEM; break; }
            if ((rc = sk_dev_alloc(uc[i], (void **)&j.d_rec[i], bytes)) == SK_OK) rc = sk_dev_upload(uc[i], j.d_rec[i], h_rec[i], bytes);
        }
        if (rc != SK_OK) fprintf(err, "kmer_scrub_count: no room for the items' records (--prevalence): %s\n", sk_strerror(rc));
        else rc = skh_scan_list_many_prevalence(uc, nr, list[l], 0, pv->nslots, sm_item_fold_hook, &j, &walked, progress, err, bases);
        failed = rc != SK_OK;
        if (!failed) {                                           /* the walk's lines are the lines the masks and cells were made from */
            int same = walked.n == j.nline;
            for (t = 0; same && t < walked.n; t++) same = walked.item[t].line == t + 1 && !strcmp(walked.item[t].path, j.line[t]);
            if (!same) { fprintf(err, "kmer_scrub_count: %s changed while it was read\n", list[l]); failed = 1; }
        }
        for (i = 0; i < nr; i++) {                               /* where the list ends: ONE wait per union, then its cells come home */
            const size_t bytes = ((size_t)j.nline * r[i].n + 1) * 2u * sizeof(uint64_t);
            int src = sk_sync(uc[i]);
            if (src == SK_OK && !failed && j.d_rec && j.d_rec[i]) src = sk_dev_download(uc[i], h_rec[i], j.d_rec[i], bytes);
            if (src != SK_OK && !failed) {
                fprintf(err, "kmer_scrub_count: the items' records could not be fetched: %s (%s)\n", sk_strerror(src), sk_last_error(uc[i]));
                failed = 1;
            }
            if (j.d_rec && j.d_rec[i]) (void)sk_dev_free(uc[i], j.d_rec[i]);
        }
        for (i = 0; !failed && i < nr; i++)                      /* every member's items of this list */
            for (k = 0; k < r[i].n; k++) {
                skh_prev_items *o = &r[i].g[k]->pitems[l];
                o->item = (skh_prev_item *)calloc((size_t)walked.n + 1, sizeof *o->item);
                o->n = 0;
                if (!o->item) { fprintf(err, "kmer_scrub_count: out of memory\n"); failed = 1; break; }
                for (t = 0; t < walked.n; t++) {
                    const skh_prev_item *w = &walked.item[t];
                    const uint64_t *cell = h_rec[i] + ((size_t)(w->line - 1) * r[i].n + k) * 2u;
                    skh_prev_item *it = &o->item[o->n];
                    if (j.is_c && strcmp(r[i].g[k]->genome, w->path) == 0) continue;
                    it->line = w->line; it->path = strdup(w->path); it->bases = w->bases;
                    it->kmers_present = cell[0]; it->kmer_hits = cell[1];
                    o->n++;
                }
            }
        skh_prev_items_free(&walked);
        for (i = 0; i < nr; i++) if (h_rec) free(h_rec[i]);
        free(h_rec); free(j.d_rec);
        if (l == 2 && !failed) { c_line = j.line; c_nline = j.nline; }
        else sm_lines_free(j.line, j.nline);
    }
    if (pv->timing) {
        double ms = 0.0;
        uint64_t nf = 0;
        (void)sk_item_fold_timing_(uc[0], 0, &ms, &nf);
        pv->fold_ms += ms; pv->folds += nf;
    }
    free(uc);
    /* the lines a member would have skipped: said where and in the order one pass per union said them (sm_union_skips) */
    for (i = 0; !failed && i < nr; i++)
        for (t = 0; t < c_nline; t++)
            for (k = 0; k < r[i].n; k++) if (strcmp(r[i].g[k]->genome, c_line[t]) == 0) fprintf(err, "skipping %s (identical match)\n", c_line[t]);
    sm_lines_free(c_line, c_nline);
    return failed;
}

static int sm_is_gz(const char *p)
{
    const size_t l = strlen(p);
    return l >= 3 && strcmp(p + l - 3, ".gz") == 0;
}

static void sm_usage(FILE *err)
{
    fputs("Usage: kmer_scrub_count -S <strains file: genome TAB outfile per line> -A <file with multiple genome filenames> "
          "-B <file with multiple metagenome filenames> -C <(optional) file with multiple genome filenames of drug strains> "
          "-p [progress output file, optional]\n", err);
    fputs("  with --scrub <min_fraction> [--independent] --detect <strain_detect arguments: -B list | -b -c -t, --coverage-depth, "
          "--min-kmer-hits>: a line is genome TAB informative outfile TAB hits outfile [TAB -g list] (steps 1-3, 4)\n", err);
}

/* where strain_detect --coverage-depth puts a strain's table: its hit list's name, ".kmer_hits.gz" replaced by ".coverage_depth" */
static char *sm_cov_path(const char *hits)
{
    const size_t n = strlen(hits);
    char *c = (char *)malloc(n + 32);
    strcpy(c, hits);
    if (n >= 13 && !strcmp(c + n - 13, ".kmer_hits.gz")) c[n - 13] = 0;
    strcat(c, ".coverage_depth");
    return c;
}

/* the arguments behind --detect, checked before anything is opened: strain_detect's own letters, less the ones every strain's
 * line gives (-r -a -o -g) and -S; --coverage-depth without a file name (one name cannot serve many strains) */
static int sm_check_detect(int argc, char **argv, int *want_cov, int *want_sw, FILE *err)
{
    char **v = (char **)malloc(((size_t)argc + 1) * sizeof *v);
    int c, n = 0, bad = 0, saved = opterr, want_rg = 0, want_sp = 0, want_rc = 0, want_rp = 0, want_th = 0, want_su = 0, want_sq = 0;
    const char *th_list = NULL;
    if (!v) return 1;
    for (c = 0; c < argc; c++) {
        if (c > 0 && !strncmp(argv[c], "--coverage-background", 21) && (argv[c][21] == 0 || argv[c][21] == '=')) {
            fprintf(err, "kmer_scrub_count: --coverage-background does not go behind --detect: the resident tables are loaded without its count column; "
                         "run strain_detect on its own for it\n");
            free(v);
            return 1;
        }
        if (c > 0 && !strncmp(argv[c], "--coverage-depth", 16) && (argv[c][16] == 0 || argv[c][16] == '=')) {
            if (argv[c][16] == '=') {
                fprintf(err, "kmer_scrub_count: with -S, --coverage-depth takes no file name (each strain's table goes next to its hit list)\n");
                free(v);
                return 1;
            }
            *want_cov |= 1;
            continue;
        }
        if (c > 0 && !strncmp(argv[c], "--coverage-only", 15) && (argv[c][15] == 0 || argv[c][15] == '=')) {
            if (argv[c][15] == '=') {
                fprintf(err, "kmer_scrub_count: with -S, --coverage-only takes no file name (each strain's table goes where its hit list would name it)\n");
                free(v);
                return 1;
            }
            *want_cov |= 2;                          /* (no hit list is written: none is created up front either) */
            continue;
        }
        if (c > 0 && !strncmp(argv[c], "--coverage-regions", 18) && (argv[c][18] == 0 || argv[c][18] == '=')) {
            if (argv[c][18] == '=') {
                fprintf(err, "kmer_scrub_count: with -S, --coverage-regions takes no file name (each strain's table goes next to its coverage table)\n");
                free(v);
                return 1;
            }
            want_rg = 1;
            continue;
        }
        if (c > 0 && !strcmp(argv[c], "--region-window") && c + 1 < argc) { c++; continue; }
        if (c > 0 && !strncmp(argv[c], "--region-window=", 16)) continue;
        if (c > 0 && !strncmp(argv[c], "--coverage-spectrum", 19) && (argv[c][19] == 0 || argv[c][19] == '=')) {
            if (argv[c][19] == '=') {
                fprintf(err, "kmer_scrub_count: with -S, --coverage-spectrum takes no file name (each strain's table goes next to its coverage table)\n");
                free(v);
                return 1;
            }
            want_sp = 1;
            continue;
        }
        if (c > 0 && !strncmp(argv[c], "--coverage-recurrence", 21) && (argv[c][21] == 0 || argv[c][21] == '=')) {
            if (argv[c][21] == '=') {
                fprintf(err, "kmer_scrub_count: with -S, --coverage-recurrence takes no file name (each strain's table goes next to its coverage table)\n");
                free(v);
                return 1;
            }
            want_rc = 1;
            continue;
        }
        if (c > 0 && !strncmp(argv[c], "--recurrence-pairs", 18) && (argv[c][18] == 0 || argv[c][18] == '=')) {
            if (argv[c][18] == '=') {
                fprintf(err, "kmer_scrub_count: with -S, --recurrence-pairs takes no file name (each strain's table goes next to its coverage table)\n");
                free(v);
                return 1;
            }
            want_rp = 1;
            continue;
        }
        if (c > 0 && !strncmp(argv[c], "--coverage-thresholds", 21) && (argv[c][21] == 0 || argv[c][21] == '=')) {
            if (argv[c][21] == '=') {
                fprintf(err, "kmer_scrub_count: with -S, --coverage-thresholds takes no file name (each strain's table goes next to its coverage table)\n");
                free(v);
                return 1;
            }
            want_th = 1;
            continue;
        }
        if (c > 0 && !strncmp(argv[c], "--coverage-scrub-sweep", 22) && (argv[c][22] == 0 || argv[c][22] == '=')) {
            if (argv[c][22] == '=') {
                fprintf(err, "kmer_scrub_count: with -S, --coverage-scrub-sweep takes no file name (each strain's table goes next to its coverage table)\n");
                free(v);
                return 1;
            }
            *want_sw = 1;
            continue;
        }
        if (c > 0 && !strncmp(argv[c], "--scrub-classes", 15) && (argv[c][15] == 0 || argv[c][15] == '=')) {
            fprintf(err, "kmer_scrub_count: with -S, each strain's class file is the one --scrub f0,f1,... writes beside its informative list (no --scrub-classes)\n");
            free(v);
            return 1;
        }
        if (c > 0 && !strcmp(argv[c], "--threshold-list") && c + 1 < argc) { th_list = argv[++c]; continue; }
        if (c > 0 && !strncmp(argv[c], "--threshold-list=", 17)) { th_list = argv[c] + 17; continue; }
        if (c > 0 && !strcmp(argv[c], "--spectrum-max") && c + 1 < argc) { c++; continue; }
        if (c > 0 && !strncmp(argv[c], "--spectrum-max=", 15)) continue;
        if (c > 0 && !strncmp(argv[c], "--panel-share", 13) && (argv[c][13] == 0 || argv[c][13] == '=')) {
            if (argv[c][13] == 0 || argv[c][14] == 0) {      /* (the one table of the whole panel: here a file name is needed) */
                fprintf(err, "kmer_scrub_count: --panel-share=FILE needs a file name: the table is one file for the whole panel\n");
                free(v);
                return 1;
            }
            continue;
        }
        if (c > 0 && !strncmp(argv[c], "--coverage-support", 18) && (argv[c][18] == 0 || argv[c][18] == '=')) {
            if (argv[c][18] == '=') {
                fprintf(err, "kmer_scrub_count: with -S, --coverage-support takes no file name (each strain's table goes next to its coverage table)\n");
                free(v);
                return 1;
            }
            want_su = 1;
            continue;
        }
        if (c > 0 && !strncmp(argv[c], "--support-pairs", 15) && (argv[c][15] == 0 || argv[c][15] == '=')) {
            if (argv[c][15] == 0 || argv[c][16] == 0) {      /* (the one file of the whole panel: here a file name is needed) */
                fprintf(err, "kmer_scrub_count: --support-pairs=FILE needs a file name: the table is one file for the whole panel\n");
                free(v);
                return 1;
            }
            want_sq = 1;
            continue;
        }
        if (c > 0 && !strcmp(argv[c], "--min-kmer-hits") && c + 1 < argc) { c++; continue; }
        v[n++] = argv[c];
    }
    v[n] = NULL;
    if (*want_cov == 3) {
        fprintf(err, "kmer_scrub_count: --coverage-only and --coverage-depth exclude each other (the table is the same; only one writes the hit list)\n");
        free(v);
        return 1;
    }
    if (want_rg && !*want_cov) {
        fprintf(err, "kmer_scrub_count: --coverage-regions goes with --coverage-depth or --coverage-only: it folds their table's numbers by region\n");
        free(v);
        return 1;
    }
    if (want_sp && !*want_cov) {
        fprintf(err, "kmer_scrub_count: --coverage-spectrum goes with --coverage-depth or --coverage-only: it bins their table's hits by depth\n");
        free(v);
        return 1;
    }
    if (th_list && !want_th) {
        fprintf(err, "kmer_scrub_count: --threshold-list goes with --coverage-thresholds\n");
        free(v);
        return 1;
    }
    if (want_th && !*want_cov) {
        fprintf(err, "kmer_scrub_count: --coverage-thresholds goes with --coverage-depth or --coverage-only: it gives their table's two numbers at several --min-kmer-hits\n");
        free(v);
        return 1;
    }
    if (th_list) {                                   /* (the list is read before the lists are: strain_detect runs after the scrub) */
        int64_t t[SK_COVACC_THRESHOLDS_MAX];
        uint32_t nt = 0;
        char why[160];
        if (skc_parse_threshold_list(th_list, t, &nt, why, sizeof why)) {
            fprintf(err, "kmer_scrub_count: --threshold-list %s: %s\n", th_list, why);
            free(v);
            return 1;
        }
    }
    if (*want_sw && !*want_cov) {
        fprintf(err, "kmer_scrub_count: --coverage-scrub-sweep goes with --coverage-depth or --coverage-only: it gives their table's numbers at several min_fraction\n");
        free(v);
        return 1;
    }
    if (want_sq && !want_su) {
        fprintf(err, "kmer_scrub_count: --support-pairs goes with --coverage-support\n");
        free(v);
        return 1;
    }
    if (want_su && !*want_cov) {
        fprintf(err, "kmer_scrub_count: --coverage-support goes with --coverage-depth or --coverage-only: it counts the read pairs behind their table's numbers\n");
        free(v);
        return 1;
    }
    if (want_rp && !want_rc) {
        fprintf(err, "kmer_scrub_count: --recurrence-pairs goes with --coverage-recurrence\n");
        free(v);
        return 1;
    }
    if (want_rc && !*want_cov) {
        fprintf(err, "kmer_scrub_count: --coverage-recurrence goes with --coverage-depth or --coverage-only: it follows their table's k-mers over the samples\n");
        free(v);
        return 1;
    }
    opterr = 0;                                      /* (strain_detect itself reports unknown letters later) */
    optind = 1;
    while (!bad && (c = getopt(n, v, "g:r:a:A:b:c:B:S:M:o:t:Hhuspn")) != -1)
        if (c == 'r' || c == 'a' || c == 'o' || c == 'S' || c == 'g') {
            fprintf(err, "kmer_scrub_count: with -S, each strain's line gives strain_detect's -%c (not after --detect)\n", c);
            bad = 1;
        }
    opterr = saved;
    optind = 1;
    free(v);
    return bad;
}

static int sm_main(int argc, char **argv, FILE *out, FILE *err, int *pack_cache_word_out);

/* (--pack-cache DIR sets the process-wide default of the packed input cache: taken back when the call ends, however it ends) */
int skh_kmer_scrub_count_multi_main(int argc, char **argv, FILE *out, FILE *err)
{
    int word = 0;
    const int status = sm_main(argc, argv, out, err, &word);
    if (word) skh_pack_cache_set(NULL, NULL, NULL);
    return status;
}

static int sm_main(int argc, char **argv, FILE *out, FILE *err, int *pack_cache_word_out)
{
    const char *A = NULL, *B = NULL, *C = NULL, *P = NULL, *S = NULL, *env;
    const int world = sm_env_int("SK_WORLD_SIZE", "WORLD_SIZE", "OMPI_COMM_WORLD_SIZE", 1);
    const int rank = sm_env_int("SK_RANK", "RANK", "OMPI_COMM_WORLD_RANK", 0);
    int device = sm_env_int("SK_LOCAL_RANK", "LOCAL_RANK", "OMPI_COMM_WORLD_LOCAL_RANK", 0);
    uint32_t group = SK_UNION_MAX, ns = 0, k, nunion = 0, nsingle = 0, ndecode = 0, max_unions = UINT32_MAX;
    uint64_t hbm_mb = 0, list_bases = 0;
    sm_strain *st = NULL;
    FILE *progress = NULL;
    skzo_pool zpool;
    int zpool_on = 0, status = 1, c, j, any_gz = 0, want_cov = 0;
    double t0 = sm_now(), t1 = 0, t2 = 0, t3 = 0, t4 = 0, fold_ms = 0;
    double scrub_fraction = -1.0;                    /* >= 0: step 2 on the resident counts instead of the table */
    int independent = 0, detect_argc = 0, want_sw = 0;
    const char *scrub_list = NULL;                   /* --scrub f0,f1,...: the scrub sweep (scrub_fraction is f0) */
    char **detect_argv = NULL;                       /* --detect ...: strain_detect's arguments (step 3 for all the strains) */
    /* --prevalence=SUFFIX [--prevalence-items=SUFFIX] [--prevalence-min-count m] [--scrub-by prevalence]: each strain's prevalence
     * table (and item records) beside its outfile, from the same pass (the rule is in include/strainer_kmer.h at sk_item_fold) */
    const char *prev_sfx = NULL, *items_sfx = NULL, *prev_min_text = NULL, *scrub_by = NULL;
    uint32_t prev_min = 1;
    int scrub_by_prev = 0;
    sm_prev pvs, *pv = NULL;
    char **allname = NULL;                           /* ... every output name of every strain line, whichever rank writes it */
    uint32_t nall = 0;

    /* the words of the single-strain program's extensions (skh_kmer_scrub_count_main): everything behind --detect is
     * strain_detect's command line; --scrub and --independent are taken out of argv before getopt.  Without --detect, -S does
     * not take them: the informative lists alone are the single-strain program's */
    for (c = 1; c < argc; c++)
        if (!strcmp(argv[c], "--detect")) { detect_argv = argv + c; detect_argc = argc - c; argc = c; break; }
    /* the prevalence words (before anything is read, and before --scrub-by could pass for --scrub): under -S they take a SUFFIX --
     * each strain's table goes to <its outfile><SUFFIX> --, because one file name cannot serve many strains */
    for (c = 1, j = 1; c < argc; c++) {
        if (!strncmp(argv[c], "--prevalence-min-count", 22) && (argv[c][22] == 0 || argv[c][22] == '=')) {
            prev_min_text = argv[c][22] ? argv[c] + 23 : (c + 1 < argc ? argv[++c] : "");
            continue;
        }
        if (!strncmp(argv[c], "--prevalence-items", 18) && (argv[c][18] == 0 || argv[c][18] == '=')) {
            if (argv[c][18] == 0 || argv[c][19] == 0) {
                fprintf(err, "kmer_scrub_count: with -S, --prevalence-items takes a suffix: give --prevalence-items=SUFFIX (each strain's records go to <its outfile><SUFFIX>)\n");
                return 1;
            }
            items_sfx = argv[c] + 19;
            continue;
        }
        if (!strncmp(argv[c], "--prevalence", 12)) {
            if (argv[c][12] != '=' || argv[c][13] == 0) {
                fprintf(err, "kmer_scrub_count: --prevalence does not go with -S as it stands: one file name cannot serve many strains; "
                             "give --prevalence=SUFFIX (each strain's table goes to <its outfile><SUFFIX>)\n");
                return 1;
            }
            prev_sfx = argv[c] + 13;
            continue;
        }
        if (!strncmp(argv[c], "--scrub-by", 10) && (argv[c][10] == 0 || argv[c][10] == '=')) {
            scrub_by = argv[c][10] ? argv[c] + 11 : (c + 1 < argc ? argv[++c] : "");
            continue;
        }
        argv[j++] = argv[c];
    }
    argc = j;
    if (scrub_by && strcmp(scrub_by, "prevalence") && strcmp(scrub_by, "count")) {
        fprintf(err, "kmer_scrub_count: --scrub-by takes count or prevalence\n");
        return 1;
    }
    scrub_by_prev = scrub_by && !strcmp(scrub_by, "prevalence");
    if ((prev_min_text || items_sfx) && !prev_sfx) {
        fprintf(err, "kmer_scrub_count: --prevalence-min-count and --prevalence-items need --prevalence=SUFFIX\n");
        return 1;
    }
    if (scrub_by_prev && !prev_sfx) { fprintf(err, "kmer_scrub_count: --scrub-by prevalence needs --prevalence=SUFFIX\n"); return 1; }
    if (prev_min_text) {
        char *e;
        const unsigned long long m = strtoull(prev_min_text, &e, 10);
        if (e == prev_min_text || *e || prev_min_text[0] == '-' || prev_min_text[0] == '+' || m < 1 || m > 0xFFFFFFFFull) {
            fprintf(err, "kmer_scrub_count: --prevalence-min-count needs an integer of at least 1\n");
            return 1;
        }
        prev_min = (uint32_t)m;
    }
    if (scrub_by) {                                   /* (--scrub-by needs --scrub, whatever else the line holds) */
        int has_scrub = 0;
        for (c = 1; c < argc; c++) if (!strncmp(argv[c], "--scrub", 7) && (argv[c][7] == 0 || argv[c][7] == '=')) has_scrub = 1;
        if (!has_scrub) { fprintf(err, "kmer_scrub_count: --scrub-by needs --scrub <min_fraction>\n"); return 1; }
    }
    for (c = 1; !detect_argv && c < argc; c++)
        if (!strncmp(argv[c], "--scrub", 7) || !strcmp(argv[c], "--independent")) {
            fprintf(err, "kmer_scrub_count: -S does not go with --scrub/--detect (run the strains one by one for those)\n");
            return 1;
        }
    for (c = 1, j = 1; c < argc; c++) {
        if (!strcmp(argv[c], "--independent")) { independent = 1; continue; }
        if (!strncmp(argv[c], "--pack-cache", 12) && (argv[c][12] == 0 || argv[c][12] == '=')) {     /* the packed input cache's directory (SK_PACK_CACHE) */
            const char *m = getenv("SK_PACK_CACHE_MODE");
            const char *dir = argv[c][12] ? argv[c] + 13 : (c + 1 < argc ? argv[++c] : "");
            if (!dir[0]) { fprintf(err, "kmer_scrub_count: --pack-cache needs a directory\n"); return 1; }
            skh_pack_cache_set(NULL, dir, m && !strcmp(m, "ro") ? "ro" : "rw");
            *pack_cache_word_out = 1;
            continue;
        }
        if (!strncmp(argv[c], "--scrub-out", 11)) {
            fprintf(err, "kmer_scrub_count: with -S the strains file names each informative outfile (no --scrub-out)\n");
            return 1;
        }
        if (!strncmp(argv[c], "--scrub", 7) && (argv[c][7] == 0 || argv[c][7] == '=')) {
            const char *v = argv[c][7] ? argv[c] + 8 : (c + 1 < argc ? argv[++c] : "");
            char *e;
            if (strchr(v, ',')) {                    /* a list: the scrub sweep (include/strainer_kmer.h has the rule) */
                skw_list l;
                char why[160];
                if (skw_parse_list(v, &l, why, sizeof why)) { fprintf(err, "kmer_scrub_count: --scrub %s: %s\n", v, why); return 1; }
                scrub_list = v;
                scrub_fraction = l.f[0];
                continue;
            }
            scrub_fraction = strtod(v, &e);
            if (e == v || *e || scrub_fraction < 0.0 || scrub_fraction > 1.0) {
                fprintf(err, "kmer_scrub_count: --scrub needs a fraction between 0.0 and 1.0\n");
                return 1;
            }
            continue;
        }
        argv[j++] = argv[c];
    }
    argc = j;
    optind = 1;
    while ((c = getopt(argc, argv, "A:B:C:S:p:Hhud")) != -1) {
        switch (c) {
        case 'A': A = optarg; break;
        case 'B': B = optarg; break;
        case 'C': C = optarg; break;
        case 'S': S = optarg; break;
        case 'p': P = optarg; break;
        case 'd': break;
        default:
            sm_usage(err);
            break;
        }
    }
    if (!S || !A || !B) {
        sm_usage(err);
        return 1;
    }
    if (detect_argv && scrub_fraction < 0.0) {
        fprintf(err, "kmer_scrub_count: --detect needs --scrub <min_fraction> and a single process\n");
        return 1;
    }
    if (scrub_by_prev && scrub_list) {
        fprintf(err, "kmer_scrub_count: --scrub-by prevalence does not go with a list of fractions (the scrub sweep ranks by count)\n");
        return 1;
    }
    if (detect_argv && sm_check_detect(detect_argc, detect_argv, &want_cov, &want_sw, err)) return 1;
    if (scrub_list && !want_sw) {
        fprintf(err, "kmer_scrub_count: --scrub %s: a list of fractions goes with --detect ... --coverage-scrub-sweep\n", scrub_list);
        return 1;
    }
    if (want_sw && !scrub_list) {
        fprintf(err, "kmer_scrub_count: --coverage-scrub-sweep behind --detect goes with a list of fractions, --scrub f0,f1,...\n");
        return 1;
    }
    if (scrub_list && !skh_scrub_filter_resident_sweep) { fprintf(err, "kmer_scrub_count: this build has no scrub sweep\n"); return 1; }
    if (world < 1 || rank < 0 || rank >= world) { fprintf(err, "kmer_scrub_count: bad rank %d of %d\n", rank, world); return 1; }
    if (detect_argv && (env = getenv("SK_DEVICES")) != NULL && *env) {
        fprintf(err, "kmer_scrub_count: -S --detect keeps every strain on the device that counted it (SK_DEVICES is not for this run)\n");
        return 1;
    }
    if ((env = getenv("SK_DEVICE")) != NULL) device = atoi(env);
    if ((env = getenv("SK_SCRUB_GROUP")) != NULL && atoi(env) >= 1 && atoi(env) <= SK_UNION_MAX) group = (uint32_t)atoi(env);
    if ((env = getenv("SK_SCRUB_UNIONS")) != NULL && atol(env) >= 1) max_unions = atol(env) > UINT32_MAX ? UINT32_MAX : (uint32_t)atol(env);
    if ((env = getenv("SK_SCRUB_HBM_MB")) != NULL && atoll(env) >= 1) hbm_mb = (uint64_t)atoll(env);

    {   /* the strains file: <genome> TAB <outfile> (with --detect: <genome> TAB <informative> TAB <hits> [TAB <-g list>]);
         * this rank's lines (round-robin over the strain lines) */
        FILE *fp = fopen(S, "r");
        char *line = NULL, *nl;
        size_t cap = 0;
        unsigned lineno = 0;
        if (!fp) { fprintf(err, "kmer_scrub_count: could not read the strain list %s\n", S); return 1; }
        while (getline(&line, &cap, fp) != -1) {
            char *fr, *fo, *fh = NULL, *fg = NULL, *rest;
            if ((nl = strchr(line, '\n')) != NULL) *nl = '\0';
            if (line[0] == '#' || line[0] == '\0') continue;
            fr = strtok(line, "\t"); fo = strtok(NULL, "\t");
            if (detect_argv) { fh = strtok(NULL, "\t"); fg = strtok(NULL, "\t"); }
            rest = strtok(NULL, "\t");
            if (!fr || !fo || rest || (detect_argv && !fh)) {
                if (detect_argv)
                    fprintf(err, "kmer_scrub_count: %s: a line needs <reference genome> TAB <informative outfile> TAB <hits outfile> "
                                 "[TAB <-g list>]\n", S);
                else fprintf(err, "kmer_scrub_count: %s: a line needs <reference genome> TAB <outfile>\n", S);
                free(line); fclose(fp);
                goto done;
            }
            if (prev_sfx) {
                /* the names this line's strain will write, on whichever rank: compared below over ALL the lines, before the deal --
                 * the ranks write into the same directories */
                char **grown = (char **)realloc(allname, ((size_t)nall + 6) * sizeof *allname), *cat;
                const char *sfx[3];
                int q;
                if (!grown) { fprintf(err, "kmer_scrub_count: out of memory\n"); free(line); fclose(fp); goto done; }
                allname = grown;
                sfx[0] = prev_sfx; sfx[1] = items_sfx; sfx[2] = scrub_list ? ".classes" : NULL;
                allname[nall++] = strdup(fo);
                for (q = 0; q < 3; q++)
                    if (sfx[q] && (cat = (char *)malloc(strlen(fo) + strlen(sfx[q]) + 1)) != NULL) { strcpy(cat, fo); strcat(cat, sfx[q]); allname[nall++] = cat; }
                if (fh && !(want_cov & 2)) allname[nall++] = strdup(fh);
                if (fh && want_cov) allname[nall++] = sm_cov_path(fh);
            }
            if (world > 1 && (int)(lineno++ % (unsigned)world) != rank) continue;     /* strains are dealt to the ranks; no collective */
            st = (sm_strain *)realloc(st, ((size_t)ns + 1) * sizeof *st);
            memset(&st[ns], 0, sizeof st[ns]);
            st[ns].genome = strdup(fr);
            st[ns].outfile = strdup(fo);
            if (fh) st[ns].hits = strdup(fh);
            if (fg) st[ns].glist = strdup(fg);
            if (fh && want_cov) st[ns].cov = sm_cov_path(fh);
            ns++;
        }
        free(line);
        fclose(fp);
    }
    if (prev_sfx) {
        /* each strain's prevalence files: its outfile's name with the suffix behind it.  No two names of the run may coincide --
         * outfiles x and x.p with the suffix .p -- or one file would end up holding another's bytes */
        uint32_t a2, b2;
        for (a2 = 0; a2 < nall; a2++)
            for (b2 = a2 + 1; b2 <= nall; b2++) {
                const char *other = b2 < nall ? allname[b2] : P;
                if (allname[a2] && other && !strcmp(allname[a2], other)) {
                    fprintf(err, "kmer_scrub_count: two outputs of this run would be the one file %s (the suffixes of --prevalence / --prevalence-items go behind each outfile's name)\n", other);
                    goto done;
                }
            }
        for (k = 0; k < ns; k++) {
            st[k].prev_path = (char *)malloc(strlen(st[k].outfile) + strlen(prev_sfx) + 1);
            if (st[k].prev_path) { strcpy(st[k].prev_path, st[k].outfile); strcat(st[k].prev_path, prev_sfx); }
            if (items_sfx && (st[k].items_path = (char *)malloc(strlen(st[k].outfile) + strlen(items_sfx) + 1)) != NULL) {
                strcpy(st[k].items_path, st[k].outfile); strcat(st[k].items_path, items_sfx);
            }
            if (!st[k].prev_path || (items_sfx && !st[k].items_path)) { fprintf(err, "kmer_scrub_count: out of memory\n"); goto done; }
        }
        memset(&pvs, 0, sizeof pvs);
        pvs.base = detect_argv ? 6u : 4u; pvs.min = prev_min; pvs.timing = getenv("SK_TIMING") != NULL;
        pv = &pvs;
    }
    /* every outfile is created before anything is scanned: a run that cannot write its results does not start (the hit lists
     * and coverage tables are written by step 3, which opens them again) */
    for (k = 0; k < ns; k++) any_gz |= sm_is_gz(st[k].outfile);
    if (any_gz) { skzo_pool_start(&zpool, sm_threads()); zpool_on = 1; }
    for (k = 0; k < ns; k++) {
        const char *more[4];
        int m;
        if (sm_is_gz(st[k].outfile)) st[k].zo = skzo_open(&zpool, st[k].outfile);
        else st[k].fp = fopen(st[k].outfile, "w");
        if (!st[k].zo && !st[k].fp) { fprintf(err, "kmer_scrub_count: cannot write %s\n", st[k].outfile); goto done; }
        st[k].made |= 1u;
        more[0] = (want_cov & 2) ? NULL : st[k].hits; more[1] = st[k].cov; more[2] = st[k].prev_path; more[3] = st[k].items_path;
        for (m = 0; m < 4; m++) {
            FILE *f;
            if (!more[m]) continue;
            if (!(f = fopen(more[m], "w"))) { fprintf(err, "kmer_scrub_count: cannot write %s\n", more[m]); goto done; }
            fclose(f);
            st[k].made |= 2u << m;
        }
    }
    if (P && rank == 0) {
        progress = fopen(P, "w");
        if (!progress) { fprintf(err, "could not open progress file %s\n", P); goto done; }
        fputs("adding kmer counts for:\n", progress);
    }

    {   /* the strains are opened on worker threads; what went wrong is said here, in list order, up to the first failure */
        sm_job j;
        memset(&j, 0, sizeof j);
        j.st = st; j.n = ns; j.device = device; j.ncols = (detect_argv ? 6 : 4) + (pv ? 3 : 0);    /* (the prevalence columns lie behind the table's own) */
        sm_pool_run(&j, sm_threads(), sm_open_worker);
        for (k = 0; k < ns; k++) {
            sm_strain *s = &st[k];
            if (s->rc_keys == SK_E_OPEN) { fprintf(err, "could not read file %s GEN_hash_sequences_set_count_vec()\n", s->genome); goto done; }
            if (s->rc_keys != SK_OK) { fprintf(err, "kmer_scrub_count: %s\n", sk_strerror(s->rc_keys)); goto done; }
            if (s->ks.short_records && rank == 0)
                fprintf(err, "kmer_scrub_count: skipped %llu reference record(s) shorter than %d bases "
                             "(the original program crashes on these)\n", (unsigned long long)s->ks.short_records, SK_K - 1);
            if (s->rc_ctx != SK_OK) { fprintf(err, "kmer_scrub_count: cannot use HIP device %d: %s\n", device, sk_strerror(s->rc_ctx)); goto done; }
            if (s->rc_load != SK_OK) { fprintf(err, "kmer_scrub_count: table load failed: %s (%s)\n", sk_strerror(s->rc_load), sk_last_error(s->ctx)); goto done; }
        }
    }
    t1 = sm_now();

    {   /* the passes: unions of up to `group` strains, as many resident at once as fit (SK_SCRUB_UNIONS at most), every list
         * decoded ONCE for all of them; then every strain a union cannot hold on its own.  Only the first decode writes the progress
         * file (every decode walks the same lists). */
        sm_strain **uni = (sm_strain **)malloc(((size_t)ns + 1) * sizeof *uni), **solo = (sm_strain **)malloc(((size_t)ns + 1) * sizeof *solo);
        sm_union *res = (sm_union *)calloc((size_t)ns + 1, sizeof *res);
        uint32_t nu = 0, nsolo = 0, a = 0;
        const int no_union = getenv("SK_SCRUB_NO_UNION") != NULL && getenv("SK_SCRUB_NO_UNION")[0] == '1';
        uint64_t budget = 0;
        int rc = 0;
        if (!uni || !solo || !res) { fprintf(err, "kmer_scrub_count: out of memory\n"); free(uni); free(solo); free(res); goto done; }
        for (k = 0; k < ns; k++) {
            const skh_keyset *ks = &st[k].ks;
            /* what sk_union_create takes: packed keys only, the text stage, fewer rows than the hit log can name */
            const int fits = !no_union && ks->nrows && !ks->nwide && ks->text2 && ks->text_bases && !getenv("SK_NO_TEXT") &&
                             ks->nrows < (1u << SK_UNION_ROW_BITS) - 1u;
            if (fits) uni[nu++] = &st[k]; else solo[nsolo++] = &st[k];
        }
        if (nu) {   /* room for unions: free HBM (or SK_SCRUB_HBM_MB) less a reserve for scratch and staging */
            uint64_t fr = 0, tot = 0;
            if (hbm_mb) fr = hbm_mb << 20;
            else if (sk_device_memory(uni[0]->ctx, &fr, &tot) != SK_OK) fr = 0;
            budget = fr > (1ull << 30) + fr / 32 ? fr - (1ull << 30) - fr / 32 : 0;
        }
        while (rc == 0 && a < nu) {
            uint32_t nr = 0;
            uint64_t used = 0;
            while (a < nu && nr < max_unions) {                /* make this decode's unions */
                const uint32_t n = nu - a < group ? nu - a : group;
                uint32_t slots = pv ? (uint32_t)sm_threads() : 0;
                const uint64_t est = sm_union_bytes(uni + a, n, slots);
                if (nr && used + est > budget) break;
                rc = sm_union_make(uni + a, n, nr > 0, &res[nr].u, err, pv ? &slots : NULL);
                if (rc == SM_FALLBACK) {                       /* (nothing was scanned) */
                    for (k = 0; k < n; k++) solo[nsolo++] = uni[a + k];
                    a += n;
                    rc = 0;
                    continue;
                }
                if (rc == SM_LATER) { rc = 0; break; }         /* (made again for the next decode) */
                if (rc != 0) break;
                res[nr].g = uni + a; res[nr].n = n;
                if (pv) {                                      /* (every union of a decode is walked with the fewest slots any of them has) */
                    uint64_t rows = 0;
                    for (k = 0; k < n; k++) rows += uni[a + k]->ks.nrows;
                    if (!nr || slots < pv->nslots) pv->nslots = slots;
                    if (!nr) pv->slot_mb = 0.0;
                    pv->slot_mb += 1e-6 * (double)slots * 8.0 * (double)rows;
                }
                nr++; used += est; a += n;
            }
            if (rc == 0 && nr) {
                if (pv) {
                    const uint64_t f0 = pv->folds;
                    const double m0 = pv->fold_ms;
                    rc = sm_decode_prev(res, nr, A, B, C, progress, err, &list_bases, pv);
                    if (pv->timing)
                        fprintf(err, "kmer_scrub_count -S timing: prevalence: %u union(s) with %u item slot(s) each take %.1f MB of HBM; %llu union folds, "
                                     "%.3f ms on the device (%.1f us each)\n", nr, pv->nslots, pv->slot_mb, (unsigned long long)(pv->folds - f0),
                                pv->fold_ms - m0, pv->folds > f0 ? 1e3 * (pv->fold_ms - m0) / (double)(pv->folds - f0) : 0.0);
                } else
                rc = sm_decode(res, nr, A, B, C, progress, err, &fold_ms, &list_bases);
                ndecode++;
                if (rc == 0) nunion += nr;
                if (progress) { fclose(progress); progress = NULL; }
            }
            for (k = 0; k < nr; k++) { skh_pack_cache_set(sk_union_context(res[k].u), NULL, NULL); sk_union_destroy(res[k].u); res[k].u = NULL; }
        }
        for (k = 0; rc == 0 && k < nsolo; k++) {
            rc = sm_single_pass(solo[k], A, B, C, progress, err, &list_bases, pv);
            nsingle++;
            ndecode++;
            if (progress) { fclose(progress); progress = NULL; }
        }
        free(uni);
        free(solo);
        free(res);
        if (rc != 0) goto done;
    }
    t2 = sm_now();

    {   /* the tables, printed on worker threads (a 5 Mbp strain's table is ~250 MB of text), or with --scrub the informative
         * lists (sk_filter on each strain's device table); what the filters said is replayed here in list order */
        sm_job j;
        memset(&j, 0, sizeof j);
        j.st = st; j.n = ns; j.with_drug = C != NULL; j.scrub_fraction = scrub_fraction; j.scrub_list = scrub_list; j.independent = independent;
        j.prev = pv != NULL; j.scrub_by_prev = scrub_by_prev; j.prev_base = pv ? pv->base : 0; j.prev_min = prev_min;
        sm_pool_run(&j, sm_threads(), sm_print_worker);
        for (k = 0; k < ns; k++) {
            int wrc = st[k].print_rc;
            if (st[k].err_buf && st[k].err_len) fwrite(st[k].err_buf, 1, st[k].err_len, err);
            if (wrc == SM_FILTER_FAILED) goto done;
            if (wrc == SM_PREV_WRITE_FAILED || wrc == SM_ITEMS_WRITE_FAILED) {
                fprintf(err, "kmer_scrub_count: cannot write %s\n", wrc == SM_PREV_WRITE_FAILED ? st[k].prev_path : st[k].items_path);
                goto done;
            }
            if (st[k].zo) { if (skzo_close(st[k].zo) && wrc == SK_OK) wrc = SK_E_OPEN; st[k].zo = NULL; }
            if (st[k].fp) { if (fclose(st[k].fp) != 0 && wrc == SK_OK) wrc = SK_E_OPEN; st[k].fp = NULL; }
            if (wrc == SK_E_OPEN) { fprintf(err, "kmer_scrub_count: error writing %s\n", st[k].outfile); goto done; }
            if (wrc != SK_OK) { fprintf(err, "kmer_scrub_count: %s (%s)\n", sk_strerror(wrc), sk_last_error(st[k].ctx)); goto done; }
        }
    }
    t3 = sm_now();
    if (detect_argv && ns) {   /* step 3 (and 4) for all of this rank's strains, on the tables of step 1: taken over by the call */
        sk_ctx **ctxs = (sk_ctx **)calloc(ns, sizeof *ctxs);
        skh_keyset *kss = (skh_keyset *)calloc(ns, sizeof *kss);
        const char **inf = (const char **)calloc(ns, sizeof *inf), **hits = (const char **)calloc(ns, sizeof *hits);
        const char **gl = (const char **)calloc(ns, sizeof *gl), **gen = (const char **)calloc(ns, sizeof *gen);
        int rc;
        if (!ctxs || !kss || !inf || !hits || !gl || !gen) {
            fprintf(err, "kmer_scrub_count: out of memory\n");
            free(ctxs); free(kss); free(inf); free(hits); free(gl); free(gen);
            goto done;
        }
        for (k = 0; k < ns; k++) {
            ctxs[k] = st[k].ctx; kss[k] = st[k].ks;
            st[k].ctx = NULL; memset(&st[k].ks, 0, sizeof st[k].ks);
            inf[k] = st[k].outfile; hits[k] = st[k].hits; gl[k] = st[k].glist; gen[k] = st[k].genome;
        }
        if (skh_resident_genomes_) skh_resident_genomes_(gen, ns);     /* (--coverage-regions reads the records' names from them) */
        rc = skh_strain_detect_resident_many(ns, ctxs, kss, inf, hits, gl, detect_argc, detect_argv, out, err);
        free(ctxs); free(kss); free(inf); free(hits); free(gl); free(gen);
        if (rc != 0) goto done;
    }
    t4 = sm_now();
    status = 0;
done:
    if (getenv("SK_TIMING") && t3 > 0 && scrub_fraction < 0.0)
        fprintf(err, "kmer_scrub_count -S timing: %u strain(s) opened in %.2f s, %u union pass(es) + %u single pass(es) %.2f s "
                     "(folds %.1f ms), print %.2f s, lists decoded %u time(s) (%llu bases)\n", ns, t1 - t0, nunion, nsingle, t2 - t1,
                fold_ms, t3 - t2, ndecode, (unsigned long long)list_bases);
    if (getenv("SK_TIMING") && t3 > 0 && scrub_fraction >= 0.0)
        fprintf(err, "kmer_scrub_count -S timing: %u strain(s) opened in %.2f s, %u union pass(es) + %u single pass(es) %.2f s "
                     "(folds %.1f ms), filter %.2f s, detect %.2f s, lists decoded %u time(s) (%llu bases)\n", ns, t1 - t0, nunion, nsingle,
                t2 - t1, fold_ms, t3 - t2, t4 > 0 ? t4 - t3 : 0.0, ndecode, (unsigned long long)list_bases);
    for (k = 0; k < ns; k++) {
        if (st[k].zo) skzo_close(st[k].zo);
        if (st[k].fp) fclose(st[k].fp);
        if (status != 0) {                                              /* no outfile of a failed run looks complete */
            if (st[k].made & 1u) unlink(st[k].outfile);
            if (st[k].made & 2u) unlink(st[k].hits);
            if (st[k].made & 4u) unlink(st[k].cov);
            if (st[k].made & 8u) unlink(st[k].prev_path);
            if (st[k].made & 16u) unlink(st[k].items_path);
        }
        if (st[k].ctx) { skh_pack_cache_set(st[k].ctx, NULL, NULL); sk_ctx_destroy(st[k].ctx); }
        skh_keyset_free(&st[k].ks);
        free(st[k].genome);
        free(st[k].outfile);
        free(st[k].hits); free(st[k].glist); free(st[k].cov);
        free(st[k].err_buf);
        free(st[k].prev_path); free(st[k].items_path);
        for (c = 0; c < 3; c++) skh_prev_items_free(&st[k].pitems[c]);
    }
    free(st);
    for (k = 0; k < nall; k++) free(allname[k]);
    free(allname);
    if (progress) fclose(progress);
    if (zpool_on) skzo_pool_stop(&zpool);
    return status;
}
