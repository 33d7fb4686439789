/* prevalence_double.c -- kmer_scrub_count's host layer with --prevalence (sk_host.c: the uncut plan, a slot per decode thread named
 * before every submit, the fold where an item ends, the records' merge, the two files) over the CPU device double, as a stand-alone
 * program for tests/test_prevalence_host.py.  It includes device_double.c and adds plain-C stand-ins for the entry points that file
 * leaves out: sk_item_slots, sk_item_slot, sk_item_fold and the device buffer calls the records travel through.  Every item-slot
 * call is appended to the file DOUBLE_ITEM_LOG names, one line per call: without the flag the file stays empty.
 * TEST CODE only -- the product's scans and folds are the HIP kernels. */
#define DOUBLE_NO_MAIN
#define sk_scan_stream dd_scan_stream
#define sk_scan_pinned dd_scan_pinned
#define sk_scan_pinned_packed dd_scan_pinned_packed
#include "device_double.c"
#undef sk_scan_stream
#undef sk_scan_pinned
#undef sk_scan_pinned_packed

static pthread_mutex_t item_mu = PTHREAD_MUTEX_INITIALIZER;
static void item_log(const char *what, long a)
{
    const char *path = getenv("DOUBLE_ITEM_LOG");
    FILE *f;
    if (!path) return;
    pthread_mutex_lock(&item_mu);
    if ((f = fopen(path, "a")) != NULL) { fprintf(f, "%s %ld\n", what, a); fclose(f); }
    pthread_mutex_unlock(&item_mu);
}

/* the slots of the one context a run has: per slot a whole counter matrix of its own, of which an item's scans fill one column */
static struct { sk_ctx *c; uint32_t nslots; int slot; uint32_t **mat; } pv = {NULL, 0, -1, NULL};

int sk_item_slots(sk_ctx *c, uint32_t nslots)
{
    uint32_t s;
    item_log("slots", (long)nslots);
    for (s = 0; s < pv.nslots; s++) free(pv.mat[s]);
    free(pv.mat);
    pv.mat = NULL; pv.nslots = 0; pv.slot = -1; pv.c = NULL;
    if (!nslots) return SK_OK;
    if (getenv("DOUBLE_ITEM_NOMEM")) return SK_E_NOMEM;                    /* (tests: the slots do not fit) */
    pv.mat = calloc(nslots, sizeof *pv.mat);
    for (s = 0; s < nslots; s++) pv.mat[s] = calloc((size_t)c->n * c->ncols + 1, 4);
    pv.nslots = nslots; pv.c = c;
    return SK_OK;
}
int sk_item_slot(sk_ctx *c, int slot)
{
    item_log("slot", (long)slot);
    if (slot < -1 || (slot >= 0 && ((uint32_t)slot >= pv.nslots || c != pv.c))) return die("sk_item_slot: no such slot");
    pv.slot = slot;
    return SK_OK;
}
int sk_item_fold(sk_ctx *c, uint32_t slot, uint32_t count_col, uint32_t prev_col, uint32_t min_count, uint64_t *rec)
{
    uint32_t r, *v, *cnt = c->cols + (size_t)count_col * c->n, *prev = c->cols + (size_t)prev_col * c->n;
    item_log("fold", (long)slot);
    if (c != pv.c || slot >= pv.nslots || count_col >= c->ncols || prev_col >= c->ncols || count_col == prev_col || min_count < 1) return die("sk_item_fold: bad argument");
    v = pv.mat[slot] + (size_t)count_col * c->n;
    for (r = 0; r < c->n; r++) {
        cnt[r] += v[r];
        if (v[r] >= min_count) { prev[r]++; rec[0]++; }
        rec[1] += v[r];
        v[r] = 0;
    }
    for (r = 0; r < c->n * c->ncols; r++) if (pv.mat[slot][r]) return die("sk_item_fold: an item's scans went into several columns");
    return SK_OK;
}
/* a scan goes into the slot that was named last (the callers name it under the lock that orders their submits) */
static int scan_in_slot(sk_ctx *c, int (*fn)(sk_ctx *, const void *, uint64_t, uint32_t, uint64_t *), const void *s, uint64_t n, uint32_t col, uint64_t *t)
{
    uint32_t *const own = c->cols;
    int rc;
    if (pv.slot >= 0 && c == pv.c) c->cols = pv.mat[pv.slot];
    rc = fn(c, s, n, col, t);
    c->cols = own;
    return rc;
}
static int as_stream(sk_ctx *c, const void *s, uint64_t n, uint32_t col, uint64_t *t) { (void)t; return dd_scan_stream(c, (const uint8_t *)s, n, col); }
static int as_pinned(sk_ctx *c, const void *s, uint64_t n, uint32_t col, uint64_t *t) { return dd_scan_pinned(c, (const uint8_t *)s, n, col, t); }
static int as_packed(sk_ctx *c, const void *s, uint64_t n, uint32_t col, uint64_t *t) { return dd_scan_pinned_packed(c, s, n, col, t); }
int sk_scan_stream(sk_ctx *c, const uint8_t *s, uint64_t n, uint32_t col) { return scan_in_slot(c, as_stream, s, n, col, NULL); }
int sk_scan_pinned(sk_ctx *c, const uint8_t *s, uint64_t n, uint32_t col, uint64_t *t) { return scan_in_slot(c, as_pinned, s, n, col, t); }
int sk_scan_pinned_packed(sk_ctx *c, const void *p, uint64_t n, uint32_t col, uint64_t *t) { return scan_in_slot(c, as_packed, p, n, col, t); }

int sk_dev_alloc(sk_ctx *c, void **dev, uint64_t n) { (void)c; *dev = calloc(n ? n : 16, 1); return *dev ? SK_OK : SK_E_NOMEM; }
int sk_dev_free(sk_ctx *c, void *dev) { (void)c; free(dev); return SK_OK; }
int sk_dev_upload(sk_ctx *c, void *dev, const void *host, uint64_t n) { (void)c; memcpy(dev, host, n); return SK_OK; }
int sk_dev_download(sk_ctx *c, void *host, const void *dev, uint64_t n) { (void)c; memcpy(host, dev, n); return SK_OK; }

#ifndef DOUBLE_MAIN
#define DOUBLE_MAIN skh_kmer_scrub_count_main
#endif
int main(int argc, char **argv) { return DOUBLE_MAIN(argc, argv, stdout, stderr); }
