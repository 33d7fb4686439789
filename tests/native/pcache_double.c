/* pcache_double.c -- tests/native/device_double.c plus the byte-string route, for the packed input cache's CPU tests
 * (tests/test_pack_cache_host.py): the golden cases `mixed`, `drug` and `iupac_strain` have IUPAC letters, U and CR in strain and
 * reads, which the double leaves out.  The double is included as it is, with its table-load-wide and its four count scans renamed
 * out of the way; the ones below walk every window the way the host's builder does (sk_host.c: builder_record, after
 * src/genome_compare.c:1000-1024): a window without N is keyed by its upper-cased text or that text's reverse complement under the
 * reference's complement map, whichever compares greater, and looked up among the packed keys when that key is all A/C/G/T, among
 * the byte-string keys otherwise.  TEST CODE only -- the product's lookups are the HIP kernels. */
#define sk_table_load_wide   dd_table_load_wide
#define sk_scan_stream       dd_scan_stream
#define sk_scan_pinned       dd_scan_pinned
#define sk_scan_pinned_packed dd_scan_pinned_packed
#define sk_scan_device_packed dd_scan_device_packed
#include "device_double.c"
#undef sk_table_load_wide
#undef sk_scan_stream
#undef sk_scan_pinned
#undef sk_scan_pinned_packed
#undef sk_scan_device_packed

static struct { const sk_ctx *c; char *keys; uint32_t *rows; uint32_t n; } pd_wide[16];
static uint32_t pd_nwide;

int sk_table_load_wide(sk_ctx *c, const char *keys31, const uint32_t *rows, uint32_t n)
{
    uint32_t i;
    for (i = 0; i < pd_nwide && pd_wide[i].c != c; i++) ;
    if (i == 16) return die("pcache_double: more than 16 contexts");
    if (i == pd_nwide) pd_nwide++;
    free(pd_wide[i].keys); free(pd_wide[i].rows);
    pd_wide[i].c = c; pd_wide[i].n = n;
    pd_wide[i].keys = malloc((size_t)n * 32 + 1); pd_wide[i].rows = malloc((size_t)n * 4 + 1);
    memcpy(pd_wide[i].keys, keys31, (size_t)n * 32); memcpy(pd_wide[i].rows, rows, (size_t)n * 4);
    return SK_OK;
}

int sk_scan_stream(sk_ctx *c, const uint8_t *s, uint64_t n, uint32_t col)
{
    static signed char comp[256];
    static int comp_ready;
    uint64_t f = 0, rc = 0, i;
    uint32_t run = 0, soft = 0, w, nw = 0, *cnt = c->cols + (size_t)col * c->n;
    const char *wk = NULL;
    const uint32_t *wr = NULL;
    pthread_mutex_lock(&scan_mu);
    if (!comp_ready) { sk_fill_complement(comp); comp_ready = 1; }
    for (w = 0; w < pd_nwide; w++) if (pd_wide[w].c == c) { wk = pd_wide[w].keys; wr = pd_wide[w].rows; nw = pd_wide[w].n; }
    for (i = 0; i < n; i++) {
        const uint32_t ch = s[i], code = sk_code(ch);
        f = ((f << 2) | code) & SK_KMASK62;
        rc = (rc >> 2) | ((uint64_t)(3u - code) << 60);
        run = sk_is_acgt(ch) ? run + 1 : 0;
        soft = sk_is_hard_break(ch) ? 0 : soft + 1;
        if (run >= 31) {
            const int64_t row = find(c, f > rc ? f : rc);
            if (row >= 0) cnt[row]++;
        } else if (soft >= 31) {
            char u[31], o[32];
            const uint8_t *win = s + i - 30;
            int j, sign = 0, pure = 1;
            for (j = 0; j < 31; j++) u[j] = (char)sk_upper(win[j]);
            for (j = 0; j < 31 && !sign; j++) {
                const signed char a = (signed char)u[j], b = comp[(uint8_t)u[30 - j]];
                sign = (a > b) - (b > a);
            }
            if (sign >= 0) memcpy(o, u, 31);
            else for (j = 0; j < 31; j++) o[30 - j] = (char)comp[(uint8_t)u[j]];
            o[31] = '\0';
            for (j = 0; j < 31; j++) pure &= (o[j] == 'A') | (o[j] == 'C') | (o[j] == 'G') | (o[j] == 'T');
            if (pure) {
                uint64_t key = 0;
                int64_t row;
                for (j = 0; j < 31; j++) key = (key << 2) | sk_code((uint8_t)o[j]);
                if ((row = find(c, key)) >= 0) cnt[row]++;
            } else {
                for (w = 0; w < nw; w++) if (memcmp(wk + (size_t)w * 32, o, 31) == 0) { cnt[wr[w]]++; break; }
            }
        }
    }
    pthread_mutex_unlock(&scan_mu);
    return SK_OK;
}

int sk_scan_pinned(sk_ctx *c, const uint8_t *s, uint64_t n, uint32_t col, uint64_t *t) { if (t) *t = 1; return sk_scan_stream(c, s, n, col); }

/* a packed batch: its bytes made again, as the double does (a separator for every byte that was no base) */
int sk_scan_pinned_packed(sk_ctx *c, const void *packed, uint64_t n, uint32_t col, uint64_t *t)
{
    const uint64_t nch = (n + 15u) >> 4;
    const uint32_t *codes = (const uint32_t *)packed;
    const uint16_t *inv = (const uint16_t *)((const uint8_t *)packed + nch * 4u);
    uint8_t *b = (uint8_t *)malloc(n ? n : 1);
    uint64_t i;
    int rc;
    for (i = 0; i < n; i++) {
        const uint64_t g = i >> 4;
        const unsigned k = (unsigned)(i & 15u);
        b[i] = (inv[g] >> k) & 1u ? (uint8_t)'\n' : (uint8_t)"ACGT"[(codes[g] >> (30u - 2u * k)) & 3u];
    }
    if (t) *t = 1;
    rc = sk_scan_stream(c, b, n, col);
    free(b);
    return rc;
}
int sk_scan_device_packed(sk_ctx *c, const void *p, uint64_t n, uint32_t col) { uint64_t t; return sk_scan_pinned_packed(c, p, n, col, &t); }
