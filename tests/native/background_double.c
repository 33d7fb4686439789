/* background_double.c -- strain_detect's host layer with --coverage-background (sk_host_sd.c: the seventh column, the count scans
 * beside the TALLY launches, the sweep where a target ends, PE2's unpaired tail; sk_host_background.c: the tables) over the CPU device
 * double, as a stand-alone program for tests/test_coverage_background_double.py.  It includes device_double.c and adds plain-C
 * stand-ins for the entry points that file leaves out: sk_scan_batch, sk_background_finish, sk_union_count_enable, sk_union_context,
 * sk_union_background_finish.  Every table that is loaded or built reports the number of columns it was given, one line per table,
 * to the file DOUBLE_NCOLS_LOG names: six without the flag, seven with it.
 * TEST CODE only -- the product's scans and sweeps are the HIP kernels. */
#define DOUBLE_NO_MAIN
#define sk_table_load_ex dd_table_load_ex
#define sk_table_build_from_text dd_table_build_from_text
#include "device_double.c"
#undef sk_table_load_ex
#undef sk_table_build_from_text
#include "../../strainer2_amd/csrc/sk_host_background.c"

static pthread_mutex_t log_mu = PTHREAD_MUTEX_INITIALIZER;
static void log_ncols(uint32_t ncols)
{
    const char *path = getenv("DOUBLE_NCOLS_LOG");
    FILE *f;
    if (!path) return;
    pthread_mutex_lock(&log_mu);
    if ((f = fopen(path, "a")) != NULL) { fprintf(f, "%u\n", ncols); fclose(f); }
    pthread_mutex_unlock(&log_mu);
}
int sk_table_load_ex(sk_ctx *c, const uint64_t *keys, uint32_t n, uint32_t ncols, const uint32_t *loc)
{
    log_ncols(ncols);
    return dd_table_load_ex(c, keys, n, ncols, loc);
}
int sk_table_build_from_text(sk_ctx *c, const uint32_t *text2, const uint32_t *ok, uint32_t nbases, uint32_t nstarts, uint32_t ncols, uint32_t col0, uint32_t *nrows)
{
    log_ncols(ncols);
    return dd_table_build_from_text(c, text2, ok, nbases, nstarts, ncols, col0, nrows);
}

/* a union's count column: here one array per member, behind a context of the union's own that holds no table */
#define BG_UNIONS 16
static struct { sk_union *u; sk_ctx *ctx; uint32_t *cnt[SK_UNION_MAX]; } bgu[BG_UNIONS];
static int bgu_of_union(const sk_union *u) { int k; for (k = 0; k < BG_UNIONS; k++) if (bgu[k].u == u) return k; return -1; }
static int bgu_of_ctx(const sk_ctx *c) { int k; for (k = 0; k < BG_UNIONS; k++) if (bgu[k].u && bgu[k].ctx == c) return k; return -1; }

int sk_union_count_enable(sk_union *u, uint32_t ncols)
{
    int k = bgu_of_union(u);
    uint32_t s;
    if (ncols != 1) return die("sk_union_count_enable: one column");
    if (k >= 0) return SK_OK;
    for (k = 0; k < BG_UNIONS && bgu[k].u; k++) ;
    if (k == BG_UNIONS) return die("sk_union_count_enable: too many unions");
    bgu[k].u = u;
    bgu[k].ctx = calloc(1, sizeof *bgu[k].ctx);
    for (s = 0; s < u->n; s++) bgu[k].cnt[s] = calloc((size_t)u->m[s]->n + 1, 4);
    return SK_OK;
}
sk_ctx *sk_union_context(sk_union *u) { const int k = bgu_of_union(u); return k < 0 ? NULL : bgu[k].ctx; }

static void count_into(const sk_ctx *c, const sk_batch *b, uint32_t *cnt)
{
    uint64_t f = 0, i;
    uint32_t run = 0;
    for (i = 0; i < b->nbytes; i++) {
        if (!sk_is_acgt(b->bytes[i])) { run = 0; continue; }
        f = ((f << 2) | sk_code(b->bytes[i])) & ((1ull << 62) - 1);
        if (++run >= 31) {
            const uint64_t rc = sk_revcomp62(f);
            const int64_t row = find(c, f > rc ? f : rc);
            if (row >= 0) cnt[row]++;
        }
    }
}

int sk_scan_batch(sk_ctx *c, const sk_batch *b, uint32_t col)
{
    const int k = bgu_of_ctx(c);
    uint32_t s;
    if (!b || !b->nrec) return SK_E_STATE;
    if (k >= 0) {
        if (col != 0) return die("sk_scan_batch: the union has one column");
        for (s = 0; s < bgu[k].u->n; s++) count_into(bgu[k].u->m[s], b, bgu[k].cnt[s]);
        return SK_OK;
    }
    if (col >= c->ncols) return die("sk_scan_batch: column out of range");
    count_into(c, b, c->cols + (size_t)col * c->n);
    return SK_OK;
}

static void block_of(uint32_t *cnt, const uint32_t *type, uint32_t inf_value, uint32_t n, uint32_t D, uint64_t *out)
{
    uint32_t r;
    memset(out, 0, (size_t)SK_BACKGROUND_WORDS(D) * sizeof *out);
    for (r = 0; r < n; r++) {
        uint64_t *o = out + (type[r] == inf_value ? 0u : SK_BACKGROUND_CLASS_WORDS(D));
        const uint32_t v = cnt[r];
        cnt[r] = 0;
        o[0]++; o[1] += v > 0; o[2] += v;
        if (v > D) { o[3]++; o[4] += v; } else o[SK_BACKGROUND_HEAD + v]++;
    }
}

int sk_background_finish(sk_ctx *c, uint32_t col, uint32_t type_col, uint32_t inf_value, uint32_t D, uint64_t *out)
{
    if (col >= c->ncols || type_col >= c->ncols || col == type_col || D > SK_BACKGROUND_MAX_DEPTH) return SK_E_ARG;
    block_of(c->cols + (size_t)col * c->n, c->cols + (size_t)type_col * c->n, inf_value, c->n, D, out);
    return SK_OK;
}

int sk_union_background_finish(sk_union *u, uint32_t ucol, uint32_t D, uint64_t *out)
{
    const int k = bgu_of_union(u);
    uint32_t s;
    if (k < 0) return SK_E_STATE;
    if (ucol != 0 || D > SK_BACKGROUND_MAX_DEPTH) return SK_E_ARG;
    for (s = 0; s < u->n; s++)
        block_of(bgu[k].cnt[s], u->m[s]->cols + (size_t)u->type_col * u->m[s]->n, u->inf_value, u->m[s]->n, D, out + (size_t)s * SK_BACKGROUND_WORDS(D));
    return SK_OK;
}

int main(int argc, char **argv) { return skh_strain_detect_main(argc, argv, stdout, stderr); }
