/* sk_host.c -- host layer (plain C) of libstrainer_kmer.so.
 *
 * Keeps the reference's FILE semantics around the device layer:
 *   - FASTA/FASTQ(.gz) record grammar of the reference's parser (src/kseq.h:166-211), here as a
 *     push-style state machine over inflated blocks;
 *   - build phase (src/genome_compare.c:967-1030): oriented keys of the strain, first-occurrence
 *     order, column-0 multiplicity -- keys are 62-bit packed integers, wide (non-ACGT) keys are
 *     kept as bytes;
 *   - BIO_hash slot-order replay (src/BIO_hash.c:39-61,129-139,208-216) so that rows come out in
 *     exactly the reference's order;
 *   - file-list walk, progress log, skip rule, error texts (src/genome_compare.c:115-177);
 *   - TSV printing (src/kmer_scrub_count.c:134-156) and the program's argv contract (:29-131).
 *
 * No window is ever looked up on the CPU here: lookups happen in sk_scan_grid / sk_scan_wide.
 */
#define _GNU_SOURCE
#include <ctype.h>
#include <errno.h>
#include <pthread.h>
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include <unistd.h>
#include <zlib.h>

#include "../../include/strainer_kmer.h"
#include "sk_alloc.h"
#include "sk_common.h"

#include "sk_parser.h"
#include "sk_input.h"
#include "sk_pack.h"
#include "sk_pcache.h"
#include "sk_ctxjob.h"
#include "sk_gzpipe.h"
#include "sk_cpus.h"
#include "sk_rendezvous.h"
#include "sk_internal.h"
#include "sk_sweep.h"
#pragma weak skh_scrub_filter_resident_sweep

int sk_rendezvous_exchange(int rank, int world, const char *base_path, int my_status, unsigned char *payload128, double timeout_s)
{
    return skr_exchange(rank, world, base_path, my_status, payload128, timeout_s);
}

/* tables of tens of MB that are touched at random: 2 MiB-aligned and offered to transparent huge pages
 * (fewer page faults while they are filled, fewer TLB misses while they are probed) */
static void *big_alloc(size_t bytes)
{
    void *p = NULL;
    if (bytes < (8u << 20)) return malloc(bytes);
    if (posix_memalign(&p, 2u << 20, (bytes + (2u << 20) - 1) & ~(size_t)((2u << 20) - 1))) return malloc(bytes);
    madvise(p, bytes, MADV_HUGEPAGE);
    return p;
}

static double now_s(void) { struct timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec; }


/* run a whole (possibly gzipped) file through the parser */
/* decoded bytes of a gzip file straight into the record parser; stops the inflate once the parser has stopped */
static int parse_feed_sink(void *user, const unsigned char *data, size_t n)
{
    parser *ps = (parser *)user;
    parser_feed(ps, data, n);
    return ps->state == P_STOP;
}

/* ---- the host-side pre-pack (sk_pack.h) behind the C-ABI ---- */
uint64_t sk_packed_bytes(uint64_t nbytes) { return ((nbytes + 15u) >> 4) * 6u; }

int sk_pack_stream(const uint8_t *stream, uint64_t nbytes, void *packed, int *odd)
{
    static skp_pack_fn picked = NULL;
    skp_pack_fn fn = __atomic_load_n(&picked, __ATOMIC_RELAXED);
    const uint64_t nch = (nbytes + 15u) >> 4;
    int o = 0;
    if ((!stream && nbytes) || (!packed && nbytes) || !odd) return SK_E_ARG;
    if (!fn) { fn = skp_pack_pick(); __atomic_store_n(&picked, fn, __ATOMIC_RELAXED); }       /* (idempotent: two threads store the same pointer) */
    fn(stream, nbytes, (uint32_t *)packed, (uint16_t *)((uint8_t *)packed + nch * 4u), &o);
    *odd = o;
    return SK_OK;
}

/* pipe: inflate on a helper thread while this one parses (worth it when there are fewer files than cores);
 * pipe > 1: the helper inflates each gzip member with that many threads (sk_gzpar.h) */
/* how a plain file's bytes are got at (sk_input.h): SKI_POPULATE (default), or SKI_PREAD -- SK_LIST_INPUT=read, or latched by the first
 * thread that finds the kernel without the populate advice */
static int list_input_mode = SKI_POPULATE;
static int list_input_read(void)
{
    const char *e = getenv("SK_LIST_INPUT");
    return __atomic_load_n(&list_input_mode, __ATOMIC_RELAXED) == SKI_PREAD || (e && !strcmp(e, "read"));
}

/* this thread is parsing PLAIN text (set by parse_file / parse_range, read by the list scan's sink): only then are its chunks packed
 * before they go up -- a .gz item is bound by its inflate on these same CPUs, the link idles, and packing would cost it 7 % */
static __thread int tl_plain_text;

static int parse_file(const char *path, rec_fn fn, void *user, int64_t *nrecords, int *sink_rc, int pipe)
{
    enum { BLK = 1 << 20 };
    gzFile g;
    unsigned char *blk;
    parser ps;
    int got, zrc;
    parser_init(&ps, fn, user);
    tl_plain_text = 0;
    /* gzip files go through the library's own inflate (sk_gzfast.h, about twice zlib's rate); anything else
     * -- plain text, which gzread passes through, or SK_ZLIB=1 -- through zlib */
    if (getenv("SK_ZLIB")) zrc = SKZ_NOT_GZIP;
    else if (pipe) {
        skzp zp;
        zrc = skzp_open_threads(&zp, path, pipe);               /* pipe > 1: that many threads inflate the one file */
        if (zrc == SKZ_OK) {
            const unsigned char *data;
            size_t n;
            while (ps.state != P_STOP && (n = skzp_next(&zp, &data)) > 0) parser_feed(&ps, data, n);
            skzp_close(&zp);
        }
    } else zrc = skz_decode_file(path, parse_feed_sink, &ps);
    if (zrc == SKZ_OPEN) { parser_free(&ps); return SK_E_OPEN; }
    if (zrc == SKZ_NOT_GZIP && !getenv("SK_ZLIB")) {
        /* plain text in 4 MiB blocks, populated into a mapping of the file or copied (sk_input.h has the measurements).  zlib's
         * pass-through copies behind more layers and cuts the text every MiB (the parser's whole-record shortcuts want their records
         * inside ONE block).  What is not a regular file goes through gzread below, which hands the same bytes on */
        const int fd = open(path, O_RDONLY);
        struct stat sb;
        tl_plain_text = 1;
        if (fd >= 0 && fstat(fd, &sb) == 0 && S_ISREG(sb.st_mode)) {
            const size_t n = (size_t)sb.st_size, PBLK = (size_t)4 << 20, RBLK = ski_read_block(PBLK);
            const unsigned char *t = n > 0 && !list_input_read() ? (const unsigned char *)mmap(NULL, n, PROT_READ, MAP_PRIVATE, fd, 0) : NULL;
            ski_rbuf rb = { NULL, 0 };
            size_t at = 0;
            int fr = SKI_FED;
            if (t == MAP_FAILED) t = NULL;
            if (!t) (void)posix_fadvise(fd, 0, 0, POSIX_FADV_SEQUENTIAL);
            /* (mapped: up to the size it was mapped with; copied: up to wherever the reads end, as with gzread) */
            while (fr == SKI_FED && ps.state != P_STOP && (!t || at < n)) {
                const size_t take = !t ? RBLK : n - at < PBLK ? n - at : PBLK;
                fr = ski_feed_span(&ps, t, fd, at, take, &list_input_mode, &rb, RBLK, NULL);
                at += take;
            }
            if (t) munmap((void *)t, n);
            free(rb.buf);
            if (fr != SKI_NOMEM) zrc = SKZ_OK;
        }
        if (fd >= 0) close(fd);
    }
    if (zrc == SKZ_NOT_GZIP) {
        g = gzopen(path, "r");
        if (!g) { parser_free(&ps); return SK_E_OPEN; }
        gzbuffer(g, 1 << 18);
        blk = (unsigned char *)malloc(BLK);
        while (ps.state != P_STOP && (got = gzread(g, blk, BLK)) > 0) parser_feed(&ps, blk, (size_t)got);
        free(blk);
        gzclose(g);
    }
    if (ps.state != P_STOP) parser_eof(&ps);
    if (nrecords) *nrecords = ps.nrecords;
    if (sink_rc) *sink_rc = ps.sink_rc;
    parser_free(&ps);
    return SK_OK;
}

static int parse_memory(const char *text, size_t n, rec_fn fn, void *user)
{
    /* "stream" form: every '\n'-separated line is one decoded record */
    size_t pos = 0;
    char *tmp = NULL; size_t cap = 0;
    int rc = 0;
    while (pos <= n) {
        const char *nl = pos < n ? (const char *)memchr(text + pos, '\n', n - pos) : NULL;
        size_t len = nl ? (size_t)(nl - (text + pos)) : n - pos;
        if (!nl && len == 0 && pos > 0) break;          /* nothing after the final separator */
        grow(&tmp, &cap, len);
        memcpy(tmp, text + pos, len);
        tmp[len] = '\0';
        rc = fn(user, tmp, len);
        if (rc || !nl) break;
        pos += len + 1;
    }
    free(tmp);
    return rc;
}

/* =========================================================================================
 * record stream writer: packs decoded records into '\n'-separated chunks for the device
 * ======================================================================================= */

typedef struct {
    uint8_t    *buf;
    uint64_t    cap, len;
    skh_sink_fn sink;
    void       *user;
    uint8_t  *(*next_buf)(void *user);   /* optional: buffer to fill after a flush (double buffering) */
    uint64_t    bases;
    int         rc;
} stream_writer;

static int writer_flush(stream_writer *w)
{
    if (w->len && !w->rc) {
        w->rc = w->sink(w->user, w->buf, w->len);
        if (!w->rc && w->next_buf) w->buf = NULL;    /* the next buffer is asked for when a record needs it: not after the last flush */
    }
    w->len = 0;
    return w->rc;
}

static int writer_record(void *user, char *seq, size_t len)
{
    stream_writer *w = (stream_writer *)user;
    size_t off = 0;
    w->bases += len;
    if (len < SK_K) return 0;                        /* src/genome_compare.c:204: no window fits */
    if (w->rc) return w->rc;
    while (off < len) {
        uint64_t room, take;
        if (w->cap - w->len < 2 * SK_K + 2 && writer_flush(w)) return w->rc;
        if (!w->buf && (!w->next_buf || !(w->buf = w->next_buf(w->user)))) return w->rc = SK_E_NOMEM;
        room = w->cap - w->len - 1;
        take = len - off;
        if (take > room) take = room;
        memcpy(w->buf + w->len, seq + off, take);
        w->len += take;
        w->buf[w->len++] = '\n';
        off += take;
        if (off < len) off -= SK_OVERLAP;            /* cut record: next piece re-reads k-1 bytes */
    }
    return 0;
}

int64_t skh_decode_file(const char *path, uint64_t chunk_bytes, skh_sink_fn sink, void *user, uint64_t *bases)
{
    stream_writer w;
    int64_t nrec = 0;
    int rc;
    if (chunk_bytes < 4096) chunk_bytes = 4096;
    memset(&w, 0, sizeof w);
    w.buf = (uint8_t *)malloc(chunk_bytes);
    w.cap = chunk_bytes;
    w.sink = sink;
    w.user = user;
    rc = parse_file(path, writer_record, &w, &nrec, NULL, 0);
    if (rc == SK_OK) writer_flush(&w);
    if (bases) *bases += w.bases;
    free(w.buf);
    if (rc != SK_OK) return rc;
    if (w.rc) return w.rc;
    return nrec;
}

/* =========================================================================================
 * build phase: oriented keys in first-occurrence order
 * ======================================================================================= */

#define WIDE_FLAG 0x8000000000000000ull     /* order-list entry refers to wide key (index in low bits) */

#define SK_RING 16u
typedef struct {
    /* packed-key set: open addressing on u64 -> order index */
    uint64_t *pk; uint32_t *pv; uint64_t pmask; uint64_t pcount;
    /* wide-key set */
    char *wkeys; uint32_t *wv; uint32_t wn, wcap; uint32_t *windex; uint32_t wmask;
    /* insertion order */
    uint64_t *order; uint32_t *count; uint8_t *fwd_first; uint32_t *firstpos; uint32_t n, cap;
    uint32_t default_val, incr;
    /* the strain's text, 2 bits per base (16 per word, first base on top), records end to end: the scan's
     * seed-and-verify stage compares reads with it (sk_table_load_text) */
    uint32_t *text2; uint64_t text_n, text_cap_words;
    uint64_t short_records;
    signed char comp[256];
    /* packed keys wait here for SK_RING more windows while their table line is fetched: the distinct-key
     * set of a 5 Mbp strain (100+ MB) lives in DRAM and every insert is a cache miss otherwise */
    uint64_t ring_key[SK_RING]; uint8_t ring_fwd[SK_RING]; uint32_t ring_tpos[SK_RING]; uint32_t ring_n, ring_pos;
} builder;

#define NO_POS 0xFFFFFFFFu

/* hint_bases: about how many bases the strain has (0 = unknown): the distinct-key set starts at twice
 * that many slots instead of growing there by repeated rehashing */
static void builder_init(builder *b, uint32_t default_val, uint32_t incr, uint64_t hint_bases)
{
    memset(b, 0, sizeof *b);
    b->pmask = (1u << 16) - 1;
    while (b->pmask + 1 < 2 * hint_bases && b->pmask < (1ull << 30) - 1) b->pmask = b->pmask * 2 + 1;
    b->pk = (uint64_t *)big_alloc((b->pmask + 1) * sizeof(uint64_t));
    b->pv = (uint32_t *)big_alloc((b->pmask + 1) * sizeof(uint32_t));
    memset(b->pk, 0xFF, (b->pmask + 1) * sizeof(uint64_t));
    b->wmask = 63;
    b->windex = (uint32_t *)calloc(b->wmask + 1, sizeof(uint32_t));
    b->default_val = default_val;
    b->incr = incr;
    sk_fill_complement(b->comp);
}

static void builder_free(builder *b)
{
    free(b->pk); free(b->pv); free(b->wkeys); free(b->wv); free(b->windex);
    free(b->order); free(b->count); free(b->fwd_first); free(b->firstpos); free(b->text2);
}

static uint32_t builder_append(builder *b, uint64_t entry)
{
    if (b->n == b->cap) {
        b->cap = b->cap ? b->cap * 2 : 1 << 16;
        b->order = (uint64_t *)realloc(b->order, (size_t)b->cap * sizeof(uint64_t));
        b->count = (uint32_t *)realloc(b->count, (size_t)b->cap * sizeof(uint32_t));
        b->fwd_first = (uint8_t *)realloc(b->fwd_first, (size_t)b->cap);
        b->firstpos = (uint32_t *)realloc(b->firstpos, (size_t)b->cap * sizeof(uint32_t));
    }
    b->order[b->n] = entry;
    b->count[b->n] = b->default_val;
    b->fwd_first[b->n] = 0;
    b->firstpos[b->n] = NO_POS;
    return b->n++;
}

static void builder_grow_packed(builder *b)
{
    uint64_t oldn = b->pmask + 1, i, nm = oldn * 2 - 1;
    uint64_t *ok = b->pk; uint32_t *ov = b->pv;
    b->pk = (uint64_t *)big_alloc((nm + 1) * sizeof(uint64_t));
    b->pv = (uint32_t *)big_alloc((nm + 1) * sizeof(uint32_t));
    memset(b->pk, 0xFF, (nm + 1) * sizeof(uint64_t));
    for (i = 0; i < oldn; i++) {
        uint64_t s;
        if (ok[i] == SK_EMPTY64) continue;
        s = sk_hash62(ok[i]) & nm;
        while (b->pk[s] != SK_EMPTY64) s = (s + 1) & nm;
        b->pk[s] = ok[i]; b->pv[s] = ov[i];
    }
    b->pmask = nm;
    free(ok); free(ov);
}

/* is_fwd: the key is the strain's text itself at this occurrence (not its reverse complement);
 * tpos: text position of the window's first base when the window is all ACGT, else NO_POS */
static void builder_insert_packed(builder *b, uint64_t key, int is_fwd, uint32_t tpos)
{
    uint64_t s = sk_hash62(key) & b->pmask;
    while (b->pk[s] != SK_EMPTY64) {
        if (b->pk[s] == key) { b->count[b->pv[s]] += b->incr; return; }
        s = (s + 1) & b->pmask;
    }
    b->pk[s] = key;
    b->pv[s] = builder_append(b, key);
    b->fwd_first[b->pv[s]] = (uint8_t)is_fwd;
    b->firstpos[b->pv[s]] = tpos;
    if (++b->pcount * 2 > b->pmask) builder_grow_packed(b);
}

/* queue a packed key: prefetch its table line now, insert it SK_RING windows later (order is kept) */
static void builder_add_packed(builder *b, uint64_t key, int is_fwd, uint32_t tpos)
{
    uint32_t at;
    if (b->ring_n == SK_RING) {
        builder_insert_packed(b, b->ring_key[b->ring_pos], b->ring_fwd[b->ring_pos], b->ring_tpos[b->ring_pos]);
        b->ring_pos = (b->ring_pos + 1u) & (SK_RING - 1u);
        b->ring_n--;
    }
    at = (b->ring_pos + b->ring_n) & (SK_RING - 1u);
    {
        const uint64_t s0 = sk_hash62(key) & b->pmask;
        __builtin_prefetch(&b->pk[s0], 1);
        __builtin_prefetch(&b->pv[s0], 1);
    }
    b->ring_key[at] = key;
    b->ring_fwd[at] = (uint8_t)is_fwd;
    b->ring_tpos[at] = tpos;
    b->ring_n++;
}

static void builder_drain(builder *b)
{
    while (b->ring_n) {
        builder_insert_packed(b, b->ring_key[b->ring_pos], b->ring_fwd[b->ring_pos], b->ring_tpos[b->ring_pos]);
        b->ring_pos = (b->ring_pos + 1u) & (SK_RING - 1u);
        b->ring_n--;
    }
}

static void builder_add_wide(builder *b, const char *key31)
{
    builder_drain(b);                                 /* wide and packed entries share one insertion order */
    uint32_t s = sk_hash_wide(key31) & b->wmask, i;
    while (b->windex[s]) {
        uint32_t e = b->windex[s] - 1;
        if (memcmp(b->wkeys + (size_t)e * 32, key31, SK_K) == 0) { b->count[b->wv[e]] += b->incr; return; }
        s = (s + 1) & b->wmask;
    }
    if (b->wn == b->wcap) {
        b->wcap = b->wcap ? b->wcap * 2 : 64;
        b->wkeys = (char *)realloc(b->wkeys, (size_t)b->wcap * 32);
        b->wv = (uint32_t *)realloc(b->wv, (size_t)b->wcap * sizeof(uint32_t));
    }
    memcpy(b->wkeys + (size_t)b->wn * 32, key31, SK_K);
    b->wkeys[(size_t)b->wn * 32 + SK_K] = '\0';
    b->wv[b->wn] = builder_append(b, WIDE_FLAG | b->wn);
    b->windex[s] = ++b->wn;
    if (b->wn * 2 > b->wmask) {                      /* rebuild the small index */
        uint32_t nm = b->wmask * 2 + 1;
        free(b->windex);
        b->windex = (uint32_t *)calloc((size_t)nm + 1, sizeof(uint32_t));
        for (i = 0; i < b->wn; i++) {
            uint32_t t = sk_hash_wide(b->wkeys + (size_t)i * 32) & nm;
            while (b->windex[t]) t = (t + 1) & nm;
            b->windex[t] = i + 1;
        }
        b->wmask = nm;
    }
}

/* one strain record: every window, rolling 2-bit pack; windows with a non-ACGT byte that is
 * not a hard breaker take the byte-string route (src/genome_compare.c:1000-1024) */
static int builder_record(void *user, char *seq, size_t len)
{
    builder *b = (builder *)user;
    uint64_t fwd = 0, rc = 0;
    uint32_t run = 0, soft = 0;
    size_t i;
    if (len + 1 < SK_K) { b->short_records++; return 0; }   /* reference: size_t underflow, crash */
    /* room for this record in the 2-bit text (positions beyond 2^32 - 2 are not recorded: first_pos stays NO_POS) */
    if ((b->text_n + len + 64) / 16 + 1 > b->text_cap_words) {
        uint64_t want = b->text_cap_words ? b->text_cap_words * 2 : 1u << 16;
        while (want < (b->text_n + len + 64) / 16 + 1) want *= 2;
        b->text2 = (uint32_t *)realloc(b->text2, want * sizeof(uint32_t));
        memset(b->text2 + b->text_cap_words, 0, (want - b->text_cap_words) * sizeof(uint32_t));
        b->text_cap_words = want;
    }
    const uint64_t tbase = b->text_n;
    for (i = 0; i < len; i++) {
        uint32_t c = (uint8_t)seq[i], code = sk_code(c);
        b->text2[(tbase + i) >> 4] |= (code & 3u) << (2u * (15u - (uint32_t)((tbase + i) & 15u)));
        fwd = ((fwd << 2) | code) & SK_KMASK62;
        rc = (rc >> 2) | ((uint64_t)(3u - code) << 60);
        run = sk_is_acgt(c) ? run + 1 : 0;
        soft = sk_is_hard_break(c) ? 0 : soft + 1;
        if (run >= SK_K) {
            const uint64_t tp = tbase + i - (SK_K - 1);
            builder_add_packed(b, fwd > rc ? fwd : rc, fwd > rc, tp < 0x7FFFFF00u ? (uint32_t)tp : NO_POS);
        } else if (soft >= SK_K) {
            char u[SK_K], o[SK_K + 1];
            const char *w = seq + i - (SK_K - 1);
            int j, sign = 0, pure = 1;
            for (j = 0; j < SK_K; j++) u[j] = (char)sk_upper((uint8_t)w[j]);
            for (j = 0; j < SK_K && !sign; j++) {
                signed char f = (signed char)u[j], r = b->comp[(uint8_t)u[SK_K - 1 - j]];
                sign = (f > r) - (r > f);
            }
            if (sign >= 0) memcpy(o, u, SK_K);
            else for (j = 0; j < SK_K; j++) o[SK_K - 1 - j] = (char)b->comp[(uint8_t)u[j]];
            o[SK_K] = '\0';
            for (j = 0; j < SK_K; j++) pure &= (o[j] == 'A') | (o[j] == 'C') | (o[j] == 'G') | (o[j] == 'T');
            if (pure) {                              /* e.g. U in the strain whose revcomp wins */
                uint64_t key = 0;
                for (j = 0; j < SK_K; j++) key = (key << 2) | sk_code((uint8_t)o[j]);
                builder_add_packed(b, key, sign >= 0, NO_POS);
            } else {
                builder_add_wide(b, o);
            }
        }
    }
    b->text_n = tbase + len;
    return 0;
}

/* ---- BIO_hash order replay ------------------------------------------------------------- */

static void decode_key(uint64_t key, char out[32])
{
    int i;
    for (i = 0; i < SK_K; i++) out[i] = "ACGT"[(key >> (2 * (SK_K - 1 - i))) & 3];
    out[SK_K] = '\0';
}

static uint32_t djb2_bytes(const char *s)           /* src/BIO_hash.c:208-216, signed bytes */
{
    uint32_t h = 5381u;
    for (; *s; s++) h = h * 33u + (uint32_t)(int32_t)(signed char)*s;
    return h;
}

/* djb2 of the 31 letters of a packed key without the 31 dependent multiplies:
 * h = 5381 * 33^31 + sum_i letter_i * 33^(30-i)  (mod 2^32), four letters (one byte of codes) per table lookup */
static uint32_t djb2_tab[8][256], djb2_base;
static pthread_once_t djb2_once = PTHREAD_ONCE_INIT;
static void djb2_init(void)
{
    uint32_t pw[SK_K + 1], g, v, j;
    pw[0] = 1u;
    for (j = 1; j <= SK_K; j++) pw[j] = pw[j - 1] * 33u;
    djb2_base = 5381u * pw[SK_K];
    /* the key holds letter i (0 = first) at bits 61-2i..60-2i; byte group g covers bits 8g+7..8g, i.e.
     * letters 30-4g-3 .. 30-4g (group 7 only has the first 3 letters, bits 61..56) */
    for (g = 0; g < 8; g++)
        for (v = 0; v < 256; v++) {
            uint32_t sum = 0;
            for (j = 0; j < 4; j++) {
                const int letter = 30 - 4 * (int)g - (int)j;          /* letter held in bits 2j+1..2j of the byte */
                if (letter < 0) continue;
                sum += (uint32_t)"ACGT"[(v >> (2 * j)) & 3u] * pw[30 - letter];
            }
            djb2_tab[g][v] = sum;
        }
}
static inline uint32_t djb2_packed(uint64_t key)
{
    return djb2_base + djb2_tab[0][key & 255u] + djb2_tab[1][(key >> 8) & 255u] + djb2_tab[2][(key >> 16) & 255u] +
           djb2_tab[3][(key >> 24) & 255u] + djb2_tab[4][(key >> 32) & 255u] + djb2_tab[5][(key >> 40) & 255u] +
           djb2_tab[6][(key >> 48) & 255u] + djb2_tab[7][(key >> 56) & 63u];
}

/* Replays insert-with-doubling and returns entries in ascending slot order of the final table.
 * The slot array (64 MB for a 5 Mbp strain) is probed at random: the line of the insert 16 ahead is
 * prefetched while the current one is placed. */
static uint32_t *replay_slot_order(const builder *b, uint32_t initial_slots, uint32_t *final_slots)
{
    enum { AHEAD = 48 };
    uint32_t M = initial_slots, N = 0, e, i;
    uint32_t *h32 = (uint32_t *)malloc((size_t)(b->n ? b->n : 1) * sizeof(uint32_t));
    int32_t *slot;
    uint32_t *rows;
    if (M == 0) M = 1000; else if (M < 10) M = 10;       /* src/BIO_hash.c:18-21 */
    pthread_once(&djb2_once, djb2_init);
    for (e = 0; e < b->n; e++) {
        if (b->order[e] & WIDE_FLAG) h32[e] = djb2_bytes(b->wkeys + (size_t)(b->order[e] & 0xFFFFFFFFu) * 32);
        else h32[e] = djb2_packed(b->order[e]);
    }
    slot = (int32_t *)big_alloc((size_t)M * sizeof(int32_t));
    memset(slot, 0xFF, (size_t)M * sizeof(int32_t));
    for (e = 0; e < b->n; e++) {
        uint32_t s = h32[e] % M;
        if (e + AHEAD < b->n) __builtin_prefetch(&slot[h32[e + AHEAD] % M], 1);
        while (slot[s] >= 0) s = s + 1 == M ? 0 : s + 1;
        slot[s] = (int32_t)e;
        if (N++ >= M / 2) {                              /* post-increment test: src/BIO_hash.c:138 */
            uint32_t M2 = M + M;
            int32_t *ns = (int32_t *)big_alloc((size_t)M2 * sizeof(int32_t));
            memset(ns, 0xFF, (size_t)M2 * sizeof(int32_t));
            N = 0;
            for (i = 0; i < M; i++) {                    /* old slot order: src/BIO_hash.c:54-58 */
                uint32_t t;
                if (i + 160 < M && slot[i + 160] >= 0) __builtin_prefetch(&h32[slot[i + 160]]);
                if (i + 64 < M && slot[i + 64] >= 0) __builtin_prefetch(&ns[h32[slot[i + 64]] % M2], 1);
                if (slot[i] < 0) continue;
                t = h32[slot[i]] % M2;
                while (ns[t] >= 0) t = t + 1 == M2 ? 0 : t + 1;
                ns[t] = slot[i];
                N++;
            }
            free(slot);
            slot = ns;
            M = M2;
        }
    }
    rows = (uint32_t *)malloc(((size_t)b->n + 1) * sizeof(uint32_t));
    for (i = 0, e = 0; i < M; i++) { rows[e] = (uint32_t)slot[i]; e += (uint32_t)(slot[i] >= 0); }   /* (branch-free compaction) */
    free(slot);
    free(h32);
    *final_slots = M;
    return rows;
}

static int keyset_finish(skh_keyset *ks, builder *b, uint32_t initial_slots)
{
    uint32_t r, *rows;
    builder_drain(b);
    if (initial_slots == SK_ROWS_IN_STRAIN_ORDER) {      /* rows as they first occur along the strain: no replay of the reference's table */
        rows = (uint32_t *)malloc(((size_t)b->n + 1) * sizeof(uint32_t));
        for (r = 0; r < b->n; r++) rows[r] = r;
        ks->final_slots = 0;
    } else rows = replay_slot_order(b, initial_slots, &ks->final_slots);
    uint32_t *wide_newrow = (uint32_t *)calloc(b->wn ? b->wn : 1, sizeof(uint32_t));
    ks->nrows = b->n;
    ks->nwide = b->wn;
    ks->short_records = b->short_records;
    ks->packed = (uint64_t *)malloc((size_t)(b->n ? b->n : 1) * sizeof(uint64_t));
    ks->first_count = (uint32_t *)malloc((size_t)(b->n ? b->n : 1) * sizeof(uint32_t));
    ks->locality = (uint32_t *)malloc((size_t)(b->n ? b->n : 1) * sizeof(uint32_t));
    ks->wide_keys = (char *)malloc((size_t)(b->wn ? b->wn : 1) * 32);
    ks->wide_rows = (uint32_t *)malloc((size_t)(b->wn ? b->wn : 1) * sizeof(uint32_t));
    ks->first_pos = (uint32_t *)malloc((size_t)(b->n ? b->n : 1) * sizeof(uint32_t));
    /* locality order = the device's counter order: entries with a text position first, in text order (that is
     * their insertion order), then the others (wide keys, keys met only through a U) in insertion order --
     * the contract of sk_table_load_text */
    uint32_t *newloc = (uint32_t *)malloc((size_t)(b->n ? b->n : 1) * sizeof(uint32_t));
    {
        uint32_t e, m = 0;
        for (e = 0; e < b->n; e++) if (b->firstpos[e] != NO_POS) newloc[e] = m++;
        for (e = 0; e < b->n; e++) if (b->firstpos[e] == NO_POS) newloc[e] = m++;
    }
    ks->text_bases = b->text_n < 0x7FFFFF00u ? (uint32_t)b->text_n : 0u;       /* 0: too long (a table slot has 31 bits for a position): no text stage */
    ks->text2 = NULL;
    if (ks->text_bases) {
        const size_t words = (size_t)ks->text_bases / 16 + 4;
        ks->text2 = (uint32_t *)calloc(words, sizeof(uint32_t));
        memcpy(ks->text2, b->text2, ((size_t)ks->text_bases + 15) / 16 * sizeof(uint32_t));
    }
    for (r = 0; r < b->n; r++) {
        uint64_t ent;
        if (r + 32 < b->n) { __builtin_prefetch(&b->order[rows[r + 32]]); __builtin_prefetch(&b->count[rows[r + 32]]); __builtin_prefetch(&b->fwd_first[rows[r + 32]]); }
        ent = b->order[rows[r]];
        ks->first_count[r] = b->count[rows[r]];
        ks->locality[r] = newloc[rows[r]] | (b->fwd_first[rows[r]] ? SK_LOCALITY_FWD : 0u);
        ks->first_pos[r] = ks->text_bases ? b->firstpos[rows[r]] : NO_POS;
        if (ent & WIDE_FLAG) { ks->packed[r] = SK_KEY_NONE; wide_newrow[ent & 0xFFFFFFFFu] = r; }
        else ks->packed[r] = ent;
    }
    for (r = 0; r < b->wn; r++) {
        memcpy(ks->wide_keys + (size_t)r * 32, b->wkeys + (size_t)r * 32, 32);
        ks->wide_rows[r] = wide_newrow[r];
    }
    free(wide_newrow);
    free(rows);
    free(newloc);
    return SK_OK;
}

int skh_keyset_from_file(skh_keyset *ks, const char *path, uint32_t initial_slots, uint32_t default_val, uint32_t incr)
{
    builder b;
    int rc;
    if (!ks || !path) return SK_E_ARG;
    memset(ks, 0, sizeof *ks);
    {
        struct stat st;
        const size_t pl = strlen(path);
        uint64_t hint = 0;
        if (stat(path, &st) == 0 && S_ISREG(st.st_mode))
            hint = (uint64_t)st.st_size * (pl > 3 && !strcmp(path + pl - 3, ".gz") ? 4u : 1u);
        if (hint > (1ull << 28)) hint = 1ull << 28;
        builder_init(&b, default_val, incr, hint);
    }
    {
        const double t0 = now_s();
        double t1;
        rc = parse_file(path, builder_record, &b, NULL, NULL, 0);
        t1 = now_s();
        if (rc == SK_OK) rc = keyset_finish(ks, &b, initial_slots);
        if (getenv("SK_TIMING"))
            fprintf(stderr, "key set of %s: decode + distinct k-mers %.2f s, row order replay + layout %.2f s (%u keys)\n",
                    path, t1 - t0, now_s() - t1, b.n);
    }
    builder_free(&b);
    return rc;
}

int skh_keyset_from_stream(skh_keyset *ks, const char *stream, size_t nbytes, uint32_t initial_slots,
                           uint32_t default_val, uint32_t incr)
{
    builder b;
    int rc;
    if (!ks || (!stream && nbytes)) return SK_E_ARG;
    memset(ks, 0, sizeof *ks);
    builder_init(&b, default_val, incr, nbytes);
    parse_memory(stream, nbytes, builder_record, &b);
    rc = keyset_finish(ks, &b, initial_slots);
    builder_free(&b);
    return rc;
}

/* ---- the key set built on the DEVICE (strain_detect's opening, round 3) ----------------------------------------------------
 * The host's part shrinks to what needs the file: the reference's record grammar (src/kseq.h:166-211), the strain's bases packed
 * 2 bits each, records end to end, and one bit per position "a window of 31 A/C/G/T bases of ONE record starts here" -- the
 * windows src/genome_compare.c:1000-1019 turns into keys (N breaks a window, :1007; records shorter than k - 1 are skipped and
 * counted as the host builder does).  sk_table_build_from_text makes keys, first occurrences, row numbers, rank map, filters and
 * column 0 from that; the keys come back once, in row order, for the hit lines' k-mer text.  A strain with any other letter (U,
 * IUPAC: byte-string keys) is not for this path: SK_E_UNSUPPORTED, and the caller builds the key set on the host as before. */
typedef struct { uint32_t *text2, *ok; uint64_t n, cap_words, ok_words; uint64_t nstarts, short_records; int soft; } dk_state;

static int dk_record(void *user, char *seq, size_t len)
{
    dk_state *d = (dk_state *)user;
    uint32_t run = 0;
    size_t i;
    if (len + 1 < SK_K) { d->short_records++; return 0; }
    if ((d->n + len + 64) / 16 + 1 > d->cap_words) {
        uint64_t want = d->cap_words ? d->cap_words * 2 : 1u << 16;
        while (want < (d->n + len + 64) / 16 + 1) want *= 2;
        {   /* (one bit per base: 16 bases per text word); a failed realloc leaves the old block in place for the caller to free */
            uint32_t *t2 = (uint32_t *)realloc(d->text2, want * sizeof(uint32_t)), *okb;
            if (!t2) return SK_E_NOMEM;
            d->text2 = t2;
            okb = (uint32_t *)realloc(d->ok, (want / 2 + 2) * sizeof(uint32_t));
            if (!okb) return SK_E_NOMEM;
            d->ok = okb;
        }
        memset(d->text2 + d->cap_words, 0, (want - d->cap_words) * sizeof(uint32_t));
        memset(d->ok + d->ok_words, 0, (want / 2 + 2 - d->ok_words) * sizeof(uint32_t));
        d->cap_words = want;
        d->ok_words = want / 2 + 2;
    }
    for (i = 0; i < len; i++) {
        const uint32_t c = (uint8_t)seq[i];
        const uint64_t at = d->n + i;
        if (sk_is_acgt(c)) {
            d->text2[at >> 4] |= (sk_code(c) & 3u) << (2u * (15u - (uint32_t)(at & 15u)));
            if (++run >= SK_K) { const uint64_t p = at - (SK_K - 1); d->ok[p >> 5] |= 1u << (p & 31u); d->nstarts++; }
        } else {
            run = 0;
            if (!sk_is_hard_break(c)) d->soft = 1;          /* a letter the packed table cannot hold: the host's builder decides */
        }
    }
    d->n += len;
    return 0;
}

int skh_keyset_build_on_device(skh_keyset *ks, sk_ctx *ctx, const char *path, uint32_t ncols, uint32_t col0_value)
{
    dk_state d;
    uint32_t nrows = 0;
    int rc;
    if (!ks || !ctx || !path) return SK_E_ARG;
    memset(ks, 0, sizeof *ks);
    memset(&d, 0, sizeof d);
    rc = parse_file(path, dk_record, &d, NULL, NULL, 0);
    if (rc == SK_OK && (d.soft || d.nstarts == 0 || d.n >= 0x7FFFFF00u)) rc = SK_E_UNSUPPORTED;
    if (rc == SK_OK) rc = sk_table_build_from_text(ctx, d.text2, d.ok, (uint32_t)d.n, (uint32_t)d.nstarts, ncols, col0_value, &nrows);
    free(d.text2); free(d.ok);
    if (rc != SK_OK) return rc;
    ks->nrows = nrows;
    ks->short_records = d.short_records;
    /* the keys stay on the device; the host's list is filled in for the rows somebody asks about (skh_keyset_fetch_keys: the
     * informative rows, whose k-mers the hit lines print).  0 = not fetched: no canonical key is 0 (the reverse complement of
     * thirty-one A's is thirty-one T's, the larger of the two).  calloc: pages nobody touches cost nothing */
    ks->packed = (uint64_t *)calloc((size_t)(nrows ? nrows : 1), sizeof(uint64_t));
    return ks->packed ? SK_OK : SK_E_NOMEM;
}

int skh_keyset_fetch_keys(skh_keyset *ks, sk_ctx *ctx, const uint32_t *rows, uint32_t n)
{
    uint64_t *k;
    uint32_t i;
    int rc;
    if (!ks || !ctx || (n && !rows)) return SK_E_ARG;
    if (!n) return SK_OK;
    k = (uint64_t *)malloc((size_t)n * sizeof *k);
    if (!k) return SK_E_NOMEM;
    rc = sk_table_export_keys_of(ctx, rows, n, k);
    for (i = 0; i < n && rc == SK_OK; i++) ks->packed[rows[i]] = k[i];
    free(k);
    return rc;
}

void skh_keyset_free(skh_keyset *ks)
{
    if (!ks) return;
    free(ks->packed); free(ks->first_count); free(ks->locality); free(ks->wide_keys); free(ks->wide_rows);
    free(ks->text2); free(ks->first_pos);
    memset(ks, 0, sizeof *ks);
}

void skh_keyset_key(const skh_keyset *ks, uint32_t row, char out[32])
{
    uint32_t i;
    if (ks->packed[row] != SK_KEY_NONE) { decode_key(ks->packed[row], out); return; }
    for (i = 0; i < ks->nwide; i++)
        if (ks->wide_rows[i] == row) { memcpy(out, ks->wide_keys + (size_t)i * 32, 32); return; }
    out[0] = '\0';
}

int skh_keyset_load(sk_ctx *ctx, const skh_keyset *ks, uint32_t ncols)
{
    int rc = sk_table_load_ex(ctx, ks->packed, ks->nrows, ncols, ks->locality);
    if (rc) return rc;
    rc = sk_table_load_wide(ctx, ks->wide_keys, ks->wide_rows, ks->nwide);
    if (rc) return rc;
    if (ks->text2 && ks->text_bases && ks->nrows && !getenv("SK_NO_TEXT")) rc = sk_table_load_text(ctx, ks->text2, ks->text_bases, ks->first_pos);
    if (rc) return rc;
    if (ks->nrows) rc = sk_counts_set(ctx, 0, ks->first_count);
    return rc;
}

/* =========================================================================================
 * scan phase
 * ======================================================================================= */

/* ---- plain text parsed on the device (opt-in: option "device_parse" through sk_text_option, or SK_DEVICE_PARSE=1) -------------
 * A whole plain-text item is read in pieces into a page-locked buffer and every piece goes up as it lies in the file
 * (sk_scan_text_pinned[_many]: upload, device parse, scan); the next piece begins with text[consumed..) of the one before, so every
 * piece starts at a record boundary that the device VERIFIED.  A piece the device declines, or one that shows no whole record even
 * at the 256 MiB cap, hands the rest of the file -- from that piece's start, a true record boundary -- to the host parser below,
 * which also finds the record that ends the file for the reference (a quality string of the wrong length, src/kseq.h:205-209)
 * where the reference finds it.  The host-only test builds link this file without the device layer: the entry points are weak,
 * and without them the host path is taken. */
#pragma weak skh_resident_genomes_
#pragma weak sk_scan_text_pinned_many
#pragma weak sk_text_enabled

#define TEXT_NOT_TAKEN   (-100)
#define TEXT_WHOLE       UINT64_MAX
#define TEXT_PIECE_MAX   (256ull << 20)

static int text_wanted(sk_ctx *ctx, int timing)
{
    const char *e;
    static int said = 0;
    if (sk_text_enabled && sk_scan_text_pinned_many) return ctx ? sk_text_enabled(ctx) : 0;
    e = getenv("SK_DEVICE_PARSE");
    if (e && e[0] == '1' && timing && !__atomic_exchange_n(&said, 1, __ATOMIC_RELAXED))
        fprintf(stderr, "kmer_scrub_count timing: SK_DEVICE_PARSE=1, but this build has no device parser: the host parses\n");
    return 0;
}

static uint64_t text_piece_bytes(void)
{
    const char *e = getenv("SK_TEXT_PIECE_BYTES");
    const long long v = e ? atoll(e) : 0;
    return v >= 64 && (uint64_t)v <= TEXT_PIECE_MAX ? (uint64_t)v : 32ull << 20;
}

/* the rest of a plain-text file from byte `off`, a record boundary, through the host parser */
static int parse_from(const char *path, uint64_t off, rec_fn fn, void *user, int64_t *nrecords)
{
    enum { BLK = 4 << 20 };
    const int fd = open(path, O_RDONLY);
    unsigned char *rb;
    size_t n;
    parser ps;
    if (fd < 0) return SK_E_OPEN;
    if (!(rb = (unsigned char *)malloc(BLK))) { close(fd); return SK_E_NOMEM; }
    parser_init(&ps, fn, user);
    tl_plain_text = 0;                                   /* (an item that began on the device never packs) */
    while (ps.state != P_STOP && (n = ski_pread_exact(fd, rb, BLK, off)) > 0) {
        parser_feed(&ps, rb, n);
        off += n;
    }
    free(rb);
    close(fd);
    if (ps.state != P_STOP) parser_eof(&ps);
    if (nrecords) *nrecords += ps.nrecords;
    parser_free(&ps);
    return SK_OK;
}

/* SK_OK: *resume = TEXT_WHOLE (the whole file was counted on the device), or the offset from which the host goes on (everything
 * before it was counted); TEXT_NOT_TAKEN: not a plain regular file with text in it -- the ordinary way, which also reports a file
 * that cannot be opened; a negative SK_E_*: a device error.  `mu` (may be NULL) is held around every device call.  *tbuf / *tcap: the
 * caller's text buffer (NULL at first; made here, grown here when a piece must grow; the caller gives it back with sk_pinned_free when
 * its walk is over -- that call drains the context, so it is not made per file). */
static int text_scan(sk_ctx *const *ctxs, uint32_t nctx, pthread_mutex_t *mu, const char *path, uint32_t col, uint64_t *bases,
                     int64_t *nrecords, uint64_t *resume, uint8_t **tbuf, uint64_t *tcap, int slot /* the item's slot, named before every scan; -1: none */)
{
    sk_ctx *const ctx = ctxs[0];
    const int fd = open(path, O_RDONLY);
    struct stat st;
    uint8_t *buf = *tbuf;                                  /* the caller's page-locked text buffer, kept from file to file */
    uint64_t cap = *tbuf ? *tcap : text_piece_bytes(), off = 0, have = 0;
    int rc = SK_OK, eof = 0;
    *resume = TEXT_WHOLE;
    if (fd < 0) return TEXT_NOT_TAKEN;
    if (fstat(fd, &st) != 0 || !S_ISREG(st.st_mode) || st.st_size < 2) { close(fd); return TEXT_NOT_TAKEN; }
    {
        unsigned char magic[2];
        if (pread(fd, magic, 2, 0) != 2 || (magic[0] == 0x1f && magic[1] == 0x8b)) { close(fd); return TEXT_NOT_TAKEN; }
    }
    if (!buf) {
        if (sk_pinned_alloc(ctx, (void **)&buf, cap) != SK_OK) { close(fd); return TEXT_NOT_TAKEN; }
        *tbuf = buf; *tcap = cap;
    }
    for (;;) {
        sk_text_info info;
        if (!eof && have < cap) {
            have += ski_pread_exact(fd, buf + have, (size_t)(cap - have), off + have);
            if (have < cap) eof = 1;
        }
        if (off + have >= (uint64_t)st.st_size) eof = 1;
        if (!have) break;
        if (mu) pthread_mutex_lock(mu);
        if (slot >= 0) { uint32_t c; for (c = 0; c < nctx; c++) (void)sk_item_slot(ctxs[c], slot); }
        rc = sk_scan_text_pinned_many(ctxs, nctx, buf, have, eof, col, &info);
        if (mu) pthread_mutex_unlock(mu);
        if (rc != SK_OK) break;
        if (info.status != SK_TEXT_OK) { *resume = off; break; }
        *bases += info.bases;
        *nrecords += (int64_t)info.nrecords;
        if (eof) break;
        if (info.consumed == 0) {                            /* no whole record in the piece: a longer one, up to the cap */
            uint8_t *nb = NULL;
            const uint64_t ncap = cap * 2 > TEXT_PIECE_MAX ? TEXT_PIECE_MAX : cap * 2;
            if (cap >= TEXT_PIECE_MAX || sk_pinned_alloc(ctx, (void **)&nb, ncap) != SK_OK) { *resume = off; break; }
            memcpy(nb, buf, (size_t)have);
            if (mu) pthread_mutex_lock(mu);
            sk_pinned_free(ctx, buf);
            if (mu) pthread_mutex_unlock(mu);
            buf = nb; cap = ncap;
            *tbuf = buf; *tcap = cap;
        } else {
            memmove(buf, buf + info.consumed, (size_t)(have - info.consumed));
            off += info.consumed;
            have -= info.consumed;
        }
    }
    close(fd);
    return rc;
}

/* ---- the packed input cache (opt-in; sk_pcache.h has the file format, its writer and its reader) -----------------------------
 * Who wants it: a context that was told (skh_pack_cache_set), else the process-wide default (the programs' --pack-cache), else
 * SK_PACK_CACHE / SK_PACK_CACHE_MODE.  The contexts' settings and counters live here, by address: the context itself belongs to the
 * device layer, which this path leaves untouched. */
typedef struct { const sk_ctx *ctx; char *dir; int mode, set; uint64_t served, written, stale, not_cached; } pc_conf;
static pthread_mutex_t pc_mu = PTHREAD_MUTEX_INITIALIZER;
static pc_conf *pc_confs, pc_default;
static uint32_t pc_n, pc_cap;
static int pc_warned;

static pc_conf *pc_find(const sk_ctx *ctx, int create)          /* (under pc_mu) */
{
    uint32_t i;
    for (i = 0; i < pc_n; i++) if (pc_confs[i].ctx == ctx) return &pc_confs[i];
    if (!create) return NULL;
    if (pc_n == pc_cap) {
        pc_conf *nc = (pc_conf *)realloc(pc_confs, (size_t)(pc_cap ? pc_cap * 2 : 16) * sizeof *nc);
        if (!nc) return NULL;
        pc_confs = nc; pc_cap = pc_cap ? pc_cap * 2 : 16;
    }
    memset(&pc_confs[pc_n], 0, sizeof pc_confs[pc_n]);
    pc_confs[pc_n].ctx = ctx;
    return &pc_confs[pc_n++];
}

int skh_pack_cache_set(sk_ctx *ctx, const char *dir, const char *mode)
{
    pc_conf *c;
    int m = SKPC_RW, rc = SK_OK;
    if (mode && !strcmp(mode, "ro")) m = SKPC_RO;
    else if (mode && strcmp(mode, "rw") != 0) return SK_E_ARG;
    pthread_mutex_lock(&pc_mu);
    if (!dir && !mode) {                                 /* forget the context: its setting and its counters (NULL: the default) */
        if (!ctx) { free(pc_default.dir); memset(&pc_default, 0, sizeof pc_default); }
        else if ((c = pc_find(ctx, 0)) != NULL) { free(c->dir); *c = pc_confs[--pc_n]; }
    } else if ((c = ctx ? pc_find(ctx, 1) : &pc_default) == NULL) rc = SK_E_NOMEM;
    else {
        char *d = dir && dir[0] ? strdup(dir) : NULL;
        if (dir && dir[0] && !d) rc = SK_E_NOMEM;
        else { free(c->dir); c->dir = d; c->mode = m; c->set = 1; }
    }
    pthread_mutex_unlock(&pc_mu);
    return rc;
}

int skh_pack_cache_stats(sk_ctx *ctx, uint64_t *served, uint64_t *written, uint64_t *stale, uint64_t *not_cached, int reset)
{
    pc_conf *c;
    if (!ctx) return SK_E_ARG;
    pthread_mutex_lock(&pc_mu);
    c = pc_find(ctx, 0);
    if (served) *served = c ? c->served : 0;
    if (written) *written = c ? c->written : 0;
    if (stale) *stale = c ? c->stale : 0;
    if (not_cached) *not_cached = c ? c->not_cached : 0;
    if (c && reset) c->served = c->written = c->stale = c->not_cached = 0;
    pthread_mutex_unlock(&pc_mu);
    return SK_OK;
}

/* the directory that holds for ctx (malloc'd) and its mode, or NULL: no cache */
static char *pc_effective(const sk_ctx *ctx, int *mode)
{
    const pc_conf *c;
    char *dir = NULL;
    pthread_mutex_lock(&pc_mu);
    c = pc_find(ctx, 0);
    if (!c || !c->set) c = pc_default.set ? &pc_default : NULL;
    if (c) { dir = c->dir ? strdup(c->dir) : NULL; *mode = c->mode; }
    pthread_mutex_unlock(&pc_mu);
    if (!c) {
        const char *e = getenv("SK_PACK_CACHE"), *m = getenv("SK_PACK_CACHE_MODE");
        dir = e && e[0] ? strdup(e) : NULL;
        *mode = m && !strcmp(m, "ro") ? SKPC_RO : SKPC_RW;
    }
    return dir;
}

static void pc_count(const sk_ctx *ctx, uint64_t served, uint64_t written, uint64_t stale, uint64_t not_cached)
{
    pc_conf *c;
    pthread_mutex_lock(&pc_mu);
    if ((c = pc_find(ctx, 1)) != NULL) { c->served += served; c->written += written; c->stale += stale; c->not_cached += not_cached; }
    pthread_mutex_unlock(&pc_mu);
}

/* can the directory be used?  "rw" makes it when only its last component is missing.  One warning per process when it cannot. */
static int pc_dir_usable(const char *dir, int mode, FILE *err)
{
    struct stat st;
    int ok;
    if (mode == SKPC_RW && stat(dir, &st) != 0 && errno == ENOENT) (void)mkdir(dir, 0777);
    ok = stat(dir, &st) == 0 && (S_ISDIR(st.st_mode) || (errno = ENOTDIR, 0)) && access(dir, mode == SKPC_RW ? R_OK | W_OK | X_OK : R_OK | X_OK) == 0;
    if (!ok && !__atomic_exchange_n(&pc_warned, 1, __ATOMIC_RELAXED))
        fprintf(err ? err : stderr, "libstrainer_kmer: the pack cache directory %s cannot be used (%s): scanning without it\n", dir, strerror(errno));
    return ok;
}

/* Can the source be opened for reading, as the parser would open it?  A cache file never stands in for a source this process may not
 * read (mode 000, an ACL, a root-squashed mount): such an item takes the old path and fails where it failed before.  *st: the open
 * file's own stat. */
static int pc_source_readable(const char *path, struct stat *st)
{
    const int fd = open(path, O_RDONLY | O_CLOEXEC);
    int ok;
    if (fd < 0) return 0;
    ok = fstat(fd, st) == 0 && S_ISREG(st->st_mode);
    close(fd);
    return ok;
}

typedef struct { sk_ctx *ctx; uint32_t col; } scan_sink;

static int scan_sink_fn(void *user, const uint8_t *chunk, uint64_t nbytes)
{
    scan_sink *s = (scan_sink *)user;
    return sk_scan_stream(s->ctx, chunk, nbytes, s->col);
}

static int scan_file_cached(sk_ctx *ctx, const char *path, uint32_t col, uint64_t *bases, const char *dir, int mode, int *handled);

int skh_scan_file(sk_ctx *ctx, const char *path, uint32_t col, uint64_t *bases)
{
    scan_sink s;
    int64_t rc;
    s.ctx = ctx; s.col = col;
    if (ctx && path) {                                   /* the packed input cache (opt-in): the file served from it, or written to it */
        int mode = SKPC_RW, handled = 0;
        char *dir = pc_effective(ctx, &mode);
        if (dir) {
            const int crc = scan_file_cached(ctx, path, col, bases, dir, mode, &handled);
            free(dir);
            if (handled) return crc;
        }
    }
    if (ctx && text_wanted(ctx, getenv("SK_TIMING") != NULL)) {
        uint64_t resume = TEXT_WHOLE, b = 0, tcap = 0;
        uint8_t *tbuf = NULL;
        int64_t nrec = 0;
        int trc = text_scan(&ctx, 1, NULL, path, col, &b, &nrec, &resume, &tbuf, &tcap, -1);
        if (tbuf) sk_pinned_free(ctx, tbuf);
        if (trc != TEXT_NOT_TAKEN) {
            if (trc == SK_OK && resume != TEXT_WHOLE) {
                stream_writer w;
                memset(&w, 0, sizeof w);
                w.cap = 32u << 20;
                if (!(w.buf = (uint8_t *)malloc(w.cap))) return SK_E_NOMEM;
                w.sink = scan_sink_fn;
                w.user = &s;
                trc = parse_from(path, resume, writer_record, &w, &nrec);
                if (trc == SK_OK) writer_flush(&w);
                b += w.bases;
                free(w.buf);
                if (trc == SK_OK) trc = w.rc;
            }
            if (bases) *bases += b;
            return trc;
        }
    }
    rc = skh_decode_file(path, 32u << 20, scan_sink_fn, &s, bases);
    return rc < 0 ? (int)rc : SK_OK;
}

/* ---- list walk: files are decoded by a small pool of host threads (gz inflate + record parsing is
 * the slow part of the whole program), batches are submitted to the one device context under a lock.
 * SK_THREADS sets the pool size (default: min(16, usable CPUs, sk_cpus.h); 1 = the reference's strict sequence).
 *
 * Work items.  A list line is one item, or -- a big plain-text file -- several: pieces [a, b) of its bytes, each
 * starting at a record boundary (scan_item).  Items are dealt to the ranks by size (longest processing time first: the
 * biggest item to the least loaded rank), the same plan on every rank from the same list and file sizes; inside a
 * rank the decode threads take them from a queue.  The counters are sums (src/genome_compare.c:220-223), so neither
 * the dealing nor the cutting changes a count -- provided every piece really starts at a record boundary, which is
 * CHECKED, not assumed (parse_range). */
typedef struct {
    char *path; uint64_t a, b, size; uint32_t line; int ranged;
    /* the packed input cache: 0 not for this item, PC_SERVE a valid cache file was found when the list was planned, PC_FILL one is to
     * be written; cpath: the cache file; reg/mtime: the source is a regular file, its mtime in nanoseconds (with size: what the
     * cache file's header is compared with) */
    int cache, reg; char *cpath; int64_t mtime;
} scan_item;
#define PC_SERVE 1
#define PC_FILL  2

/* one line of the list as the reference reports it: "<line>\t<time>" in the progress file just before the file is opened
 * (src/genome_compare.c:133-136,167-170), "skipping ..." on stderr for the -C line that equals -r (:138-141) */
typedef struct { char *text; int skipped; long end; } list_line;

typedef struct {
    sk_ctx         *ctx;               /* the context whose staging ring, tickets and page-locked buffers the walk uses: ctxs[0] ... */
    sk_ctx *const  *ctxs;              /* ... and every context a chunk is scanned into (skh_scan_list_many: one upload, nctx scans) */
    uint32_t        nctx;
    uint32_t        col;
    int             pipe;              /* fewer files than cores: each file's inflate gets a helper thread (> 1: that many) */
    int             gpu_inflate;       /* SK_GPU_INFLATE=1: .gz items go through the device-side decoder first (experimental) */
    int             dev_workers, worker_ids;   /* ... on this many EXTRA threads (SK_GPU_INFLATE_WORKERS, default 4), which mostly wait for the device */
    pthread_mutex_t submit_mu;         /* sk_scan_stream is one-caller-at-a-time per context (per group of contexts: sk_scan_pinned_many) */
    pthread_mutex_t queue_mu;
    scan_item      *item;              /* work list of this call (what this rank scans), in list order */
    uint32_t        nitem, next;
    int             rc;                /* first failure ...                                         */
    uint32_t        rc_index;          /* ... and the item it belongs to                            */
    uint64_t        bases;
    FILE           *progress;          /* rank 0's progress file (or NULL) ...                      */
    list_line      *ll;                /* ... the list's lines ...                                  */
    uint32_t        nll, ll_next;      /* ... and the first one not yet written there               */
    int             timing;            /* SK_TIMING: where the decode threads' time goes (seconds summed over threads, under queue_mu) */
    double          t_item, t_submit_wait, t_submit, t_ticket, t_cpu, t_pack;
    uint64_t        nchunks, npacked;
    int             pack;              /* SK_LIST_PACK: 1 (default) = the chunks of plain-text items go up packed (6 bytes per 16 bases) once the scan has shown
                                        * itself bound by the link; 0 = never; 2 = always, .gz items' too (tests) */
    int             link_bound;        /* a decode thread has spent a tenth of its time waiting for uploads (atomic) */
    int             text;              /* whole plain-text items go up as text and are parsed on the device (option "device_parse", SK_DEVICE_PARSE=1) */
    FILE           *err;               /* where a damaged cache file is named */
    uint64_t        pc_served, pc_written, pc_stale, pc_not;       /* the packed input cache: items (under queue_mu) ... */
    double          pc_t_sum, pc_t_read, pc_t_write;               /* ... seconds summed over the threads: checksums, reading, writing */
    uint64_t        pc_bytes;                                      /* ... cache bytes read or written */
    int             pc_rw;                                         /* ... the directory may be written */
    /* prevalence (skh_scan_list_prevalence): every decode thread's index is its item slot, named under submit_mu before each submit
     * on EVERY context of the walk; an item's fold is enqueued when it ends, its record cell is that of its list line.  With a fold
     * hook (skh_scan_list_many_prevalence) the slots, the folds and the records are the caller's: the hook is called where
     * sk_item_fold would be, under submit_mu */
    int             prev;
    skh_item_fold_fn fold; void *fold_user;
    uint32_t        prev_col, prev_min;
    uint64_t       *d_rec;             /* device: {kmers_present, kmer_hits} per list line */
    uint64_t       *line_bases;        /* host: the bases of each list line's item (under queue_mu) */
} scan_pool;

/* The host-only test builds link this file against device doubles without item slots (a walk with prevalence is refused there) */
#pragma weak sk_item_slots
#pragma weak sk_item_slot
#pragma weak sk_item_fold
#pragma weak sk_dev_alloc
#pragma weak sk_dev_free
#pragma weak sk_dev_upload
#pragma weak sk_dev_download
#pragma weak skh_scrub_filter_resident_cols
#pragma weak sk_item_fold_timing_

/* under submit_mu, just before a submit: the scans that follow belong to this slot's item */
static inline void pool_slot(const scan_pool *p, int slot)
{
    uint32_t c;
    if (p->prev) for (c = 0; c < p->nctx; c++) (void)sk_item_slot(p->ctxs[c], slot);
}

/* The progress file gets a list line when a decode thread TAKES the line's (first) item, and every line before it that is
 * not there yet -- the reference writes the line, then opens the file.  Called under queue_mu (or from the one thread). */
static void progress_upto(scan_pool *p, uint32_t line)
{
    if (!p->progress) { if (line + 1 > p->ll_next) p->ll_next = line + 1; return; }
    for (; p->ll_next <= line && p->ll_next < p->nll; p->ll_next++) {
        time_t now = time(NULL);
        fprintf(p->progress, "%s\t%s", p->ll[p->ll_next].text, asctime(localtime(&now)));
        p->ll[p->ll_next].end = ftell(p->progress);
    }
}

/* one decode worker: two pinned chunk buffers filled in turn; a buffer is rewritten only after the
 * DMA that read it has finished (ticket) */
typedef struct {
    scan_pool *pool;
    uint8_t   *pinned[2];
    uint64_t   ticket[2];
    int        used[2], cur;
    sk_inflater *inf;                  /* SK_GPU_INFLATE=1: this worker's device-side gzip decoder ... */
    int          dev_ok;               /* ... which only the pool's first dev_workers threads use (the others inflate on the host) */
    uint8_t   *text; uint64_t text_cap;/* ... and the page-locked buffer its text lands in */
    double     t_submit_wait, t_submit, t_ticket, t_pack;      /* SK_TIMING */
    uint64_t   nchunks, npacked;
    uint8_t   *pk[2];                  /* the chunks' packed form (sk_pack_stream), two page-locked buffers taking turns ... */
    uint64_t   pk_ticket[2];           /* ... each rewritten only after the upload that read it */
    int        pk_used[2], pk_cur;
    double     t_begin, t_wait_all;    /* since this worker began: time spent waiting for its buffers' uploads */
    uint8_t   *tbuf; uint64_t tcap;    /* device_parse: the page-locked buffer its items' text is read into */
    /* the packed input cache: the file this worker's chunks are written to (NULL: none; the helpers of a split .gz item share their
     * item's), the item that wants one once the host parser takes it, and the chunk whose packed form the device is still sending home */
    skpc_writer *fill; const scan_item *fill_item;
    int        pk_kind[2];             /* pk_ticket[i] is sk_scan_pinned_pack_many's (1) or the context's (0) */
    uint32_t  *pkodd;                  /* page-locked: the device pack's odd flags, one per pk buffer */
    uint8_t   *fill_tmp;               /* the host's pack of a chunk that went up as bytes (builds without the device pack) */
    int        pend, pend_i; const uint8_t *pend_chunk; uint64_t pend_n;
    double     t_pc_sum, t_pc_read; uint64_t pc_bytes;
    int        slot;                   /* prevalence: this thread's item slot (a split .gz item's helpers: their parent's) */
} scan_worker;

/* size of a worker's chunk buffer: SK_CHUNK_BYTES (4096 .. 63 MiB; tests use small ones: many flushes per file), default 32 MiB */
static uint64_t pool_chunk_bytes(void)
{
    const char *e = getenv("SK_CHUNK_BYTES");
    const long long v = e ? atoll(e) : 0;
    return v >= 4096 && v <= (63ll << 20) ? (uint64_t)v : 32ull << 20;
}
#define POOL_CHUNK pool_chunk_bytes()

/* The host-only test builds link this file against device doubles that have no many-context scans; in the library they are
 * always there (sk_device.hip), and a walk into several contexts is refused without them (skh_scan_list_many). */
#pragma weak sk_scan_pinned_many
#pragma weak sk_scan_pinned_packed_many
/* ... nor the device-side pack (sk_packdev.hip): without it a chunk that went up as bytes is packed for the cache file by
 * sk_pack_stream on the decode thread */
#pragma weak sk_scan_pinned_pack_many
#pragma weak sk_pack_ticket_wait
#pragma weak sk_pack_release

/* a chunk to every context of the walk, under submit_mu: with several, it goes up once and is scanned into each of them */
static int pool_submit(scan_pool *p, const void *buf, uint64_t nbytes, int packed, uint64_t *ticket)
{
    if (p->nctx > 1)
        return packed ? sk_scan_pinned_packed_many(p->ctxs, p->nctx, buf, nbytes, p->col, ticket)
                      : sk_scan_pinned_many(p->ctxs, p->nctx, (const uint8_t *)buf, nbytes, p->col, ticket);
    return packed ? sk_scan_pinned_packed(p->ctx, buf, nbytes, p->col, ticket) : sk_scan_pinned(p->ctx, (const uint8_t *)buf, nbytes, p->col, ticket);
}

/* a pk buffer is free again once the transfer that used it last is over: the upload of a packed chunk, or the device pack's copy home */
static int worker_pk_wait(scan_worker *w, int i)
{
    int rc = SK_OK;
    if (w->pk_used[i]) rc = w->pk_kind[i] ? sk_pack_ticket_wait(w->pool->ctx, w->pk_ticket[i]) : sk_ticket_wait(w->pool->ctx, w->pk_ticket[i]);
    w->pk_used[i] = 0;
    return rc;
}

/* the chunk before this one went through the device pack: its packed form (or, odd, its bytes -- the writer has not been given that
 * buffer again) goes into the cache file now */
static int worker_fill_flush(scan_worker *w)
{
    int rc;
    if (!w->pend) return SK_OK;
    w->pend = 0;
    if ((rc = worker_pk_wait(w, w->pend_i)) != SK_OK) return rc;
    if (w->pkodd[w->pend_i]) skpc_append(w->fill, SKPC_BYTES, w->pend_n, w->pend_chunk);
    else skpc_append(w->fill, SKPC_PACKED, w->pend_n, w->pk[w->pend_i]);
    return SK_OK;
}

static int worker_sink(void *user, const uint8_t *chunk, uint64_t nbytes)
{
    scan_worker *w = (scan_worker *)user;
    int rc, known_odd = 0;
    double t0 = w->pool->timing ? now_s() : 0.0;
    double t1;
    if (w->fill && (rc = worker_fill_flush(w)) != SK_OK) return rc;
    if (w->pool->pack > 1 || (w->pool->pack && tl_plain_text && __atomic_load_n(&w->pool->link_bound, __ATOMIC_RELAXED))) {
        /* The chunk goes up PACKED: what the scan kernel's first phase would make of its bytes is made here (sk_pack.h), 6 bytes per
         * 16 bases over the link instead of 16 -- the list scan of plain text was bound by the link, not by these threads.  A chunk
         * with a byte for the byte-string kernel (IUPAC, U, CR ...) goes up as bytes, below. */
        const int i = w->pk_cur ^= 1;
        if (!w->pk[i] && sk_pinned_alloc(w->pool->ctx, (void **)&w->pk[i], sk_packed_bytes(POOL_CHUNK)) != SK_OK) w->pk[i] = NULL;
        if (w->pk[i]) {
            int odd = 0;
            worker_pk_wait(w, i);
            if (w->pool->timing) { t1 = now_s(); w->t_ticket += t1 - t0; t0 = t1; }
            sk_pack_stream(chunk, nbytes, w->pk[i], &odd);
            known_odd = odd;
            if (w->pool->timing) { t1 = now_s(); w->t_pack += t1 - t0; t0 = t1; }
            if (!odd) {
                pthread_mutex_lock(&w->pool->submit_mu);
                t1 = w->pool->timing ? now_s() : 0.0;
                pool_slot(w->pool, w->slot);
                rc = pool_submit(w->pool, w->pk[i], nbytes, 1, &w->pk_ticket[i]);
                pthread_mutex_unlock(&w->pool->submit_mu);
                if (w->pool->timing) { w->t_submit_wait += t1 - t0; w->t_submit += now_s() - t1; w->nchunks++; w->npacked++; }
                w->pk_used[i] = rc == SK_OK;
                w->pk_kind[i] = 0;
                w->used[w->cur] = 0;                    /* (the bytes were read by this thread alone: their buffer is free at once) */
                if (w->fill && rc == SK_OK) skpc_append(w->fill, SKPC_PACKED, nbytes, w->pk[i]);     /* (it lies packed in page-locked memory: written out) */
                return rc;
            }
        }
    }
    if (w->fill && !known_odd && sk_scan_pinned_pack_many && sk_pack_ticket_wait) {
        /* A chunk that goes up as bytes, for a cache file: the device packs it beside its scan (sk_packdev.hip) -- a .gz item's decode
         * thread has no cycles for that -- and sends the packed form home; it is written when the next chunk comes (worker_fill_flush). */
        const int i = w->pk_cur ^= 1;
        if (!w->pk[i] && sk_pinned_alloc(w->pool->ctx, (void **)&w->pk[i], sk_packed_bytes(POOL_CHUNK)) != SK_OK) w->pk[i] = NULL;
        if (!w->pkodd && sk_pinned_alloc(w->pool->ctx, (void **)&w->pkodd, 4096) != SK_OK) w->pkodd = NULL;
        if (w->pk[i] && w->pkodd) {
            if ((rc = worker_pk_wait(w, i)) != SK_OK) return rc;
            if (w->pool->timing) { t1 = now_s(); w->t_ticket += t1 - t0; t0 = t1; }
            pthread_mutex_lock(&w->pool->submit_mu);
            t1 = w->pool->timing ? now_s() : 0.0;
            pool_slot(w->pool, w->slot);
            rc = sk_scan_pinned_pack_many(w->pool->ctxs, w->pool->nctx, chunk, nbytes, w->pool->col, w->pk[i], &w->pkodd[i], &w->pk_ticket[i]);
            pthread_mutex_unlock(&w->pool->submit_mu);
            if (w->pool->timing) { w->t_submit_wait += t1 - t0; w->t_submit += now_s() - t1; w->nchunks++; }
            w->pk_used[i] = rc == SK_OK;
            w->pk_kind[i] = 1;
            w->used[w->cur] = 0;                        /* (on return the bytes have been read) */
            if (rc == SK_OK) { w->pend = 1; w->pend_i = i; w->pend_chunk = chunk; w->pend_n = nbytes; }
            return rc;
        }
    }
    pthread_mutex_lock(&w->pool->submit_mu);
    t1 = w->pool->timing ? now_s() : 0.0;
    pool_slot(w->pool, w->slot);
    rc = pool_submit(w->pool, chunk, nbytes, 0, &w->ticket[w->cur]);
    pthread_mutex_unlock(&w->pool->submit_mu);
    if (w->pool->timing) { w->t_submit_wait += t1 - t0; w->t_submit += now_s() - t1; w->nchunks++; }
    w->used[w->cur] = 1;
    if (w->fill && rc == SK_OK) {
        int odd = known_odd;
        if (!odd && !w->fill_tmp) w->fill_tmp = (uint8_t *)malloc((size_t)sk_packed_bytes(POOL_CHUNK) + 8u);
        if (!odd && w->fill_tmp) sk_pack_stream(chunk, nbytes, w->fill_tmp, &odd);
        if (odd || !w->fill_tmp) skpc_append(w->fill, SKPC_BYTES, nbytes, chunk);
        else skpc_append(w->fill, SKPC_PACKED, nbytes, w->fill_tmp);
    }
    return rc;
}

/* the buffers come from the context's store of page-locked memory (kept from call to call) when they are first
 * needed: a worker that finds the queue empty takes none, an item that fits one buffer never takes the second */
static uint8_t *worker_buf(scan_worker *w, int i)
{
    if (!w->pinned[i] && sk_pinned_alloc(w->pool->ctx, (void **)&w->pinned[i], POOL_CHUNK) != SK_OK) w->pinned[i] = NULL;
    return w->pinned[i];
}

static uint8_t *worker_next_buf(void *user)
{
    scan_worker *w = (scan_worker *)user;
    w->cur ^= 1;
    if (w->used[w->cur]) {
        const double t0 = now_s();
        double dt;
        sk_ticket_wait(w->pool->ctx, w->ticket[w->cur]);
        dt = now_s() - t0;
        if (w->pool->timing) w->t_ticket += dt;
        /* Is this list scan bound by the link?  A thread that has spent a tenth of its time waiting for its own buffers' uploads says
         * so for all: from then on the chunks of plain-text items go up packed (worker_sink).  A scan that is short of CPUs instead
         * -- few threads per card, .gz items -- never waits here and keeps its cycles for the decode. */
        w->t_wait_all += dt;
        if (!__atomic_load_n(&w->pool->link_bound, __ATOMIC_RELAXED) && w->t_wait_all > 0.002 && w->t_wait_all > 0.1 * (now_s() - w->t_begin))
            __atomic_store_n(&w->pool->link_bound, 1, __ATOMIC_RELAXED);
    }
    return worker_buf(w, w->cur);
}

static int worker_init(scan_worker *w, scan_pool *p)
{
    memset(w, 0, sizeof *w);
    w->pool = p;
    w->t_begin = now_s();
    return SK_OK;
}

static void worker_done(scan_worker *w)
{
    int i;
    for (i = 0; i < 2; i++) if (w->pk_used[i] && w->pk_kind[i]) worker_pk_wait(w, i);     /* (a device pack still on its way home after a failure) */
#ifdef SK_EXPERIMENTS
    if (w->inf) sk_inflater_destroy(w->inf);
#endif
    if (w->text) sk_pinned_free(w->pool->ctx, w->text);
    pthread_mutex_lock(&w->pool->submit_mu);
    if (w->pinned[0]) sk_pinned_free(w->pool->ctx, w->pinned[0]);      /* (synchronises the stream first) */
    if (w->pinned[1]) sk_pinned_free(w->pool->ctx, w->pinned[1]);
    if (w->pk[0]) sk_pinned_free(w->pool->ctx, w->pk[0]);
    if (w->pk[1]) sk_pinned_free(w->pool->ctx, w->pk[1]);
    if (w->tbuf) sk_pinned_free(w->pool->ctx, w->tbuf);
    if (w->pkodd) sk_pinned_free(w->pool->ctx, w->pkodd);
    pthread_mutex_unlock(&w->pool->submit_mu);
    free(w->fill_tmp);
}

/* One piece [a, b) of a plain-text file: the records that START in it.  The piece's own start s(a) and end s(b) come from
 * guess_record_start; its bytes are parsed as a file of their own, and afterwards the parser must stand between two records
 * (P_SEEK after a FASTQ record, P_LINE_START after a FASTA line) with a header character next -- then s(b) is a true record
 * boundary GIVEN that s(a) was one.  Piece 0 starts at 0, which is one; every later piece's start is the previous piece's
 * checked end.  So if every piece passes, the pieces' records are exactly the file's records; if any piece fails, the
 * caller fails the run (SK_E_SPLIT) instead of counting something else. */
static int parse_range(const scan_item *it, rec_fn fn, void *user, int64_t *nrecords)
{
    enum { BLK = 4 << 20 };
    int fd = open(it->path, O_RDONLY);
    struct stat st;
    const unsigned char *t;
    uint64_t sa, sb, i;
    parser ps;
    int ok = 1;
    if (fd < 0) return SK_E_OPEN;
    if (fstat(fd, &st) != 0 || (uint64_t)st.st_size != it->size) { close(fd); return SK_E_SPLIT; }     /* (changed since the plan) */
    t = (const unsigned char *)mmap(NULL, (size_t)it->size, PROT_READ, MAP_PRIVATE, fd, 0);
    if (t == MAP_FAILED) { close(fd); return SK_E_OPEN; }
    /* the mapping serves the two guesses and the look at the byte behind the piece (a few pages); the piece's text goes to the
     * parser block by block, populated or copied (sk_input.h) */
    sa = parser_guess_start(t, it->size, it->a, 1);
    sb = it->b >= it->size ? it->size : parser_guess_start(t, it->size, it->b, 1);
    parser_init(&ps, fn, user);
    tl_plain_text = 1;
    {
        int copy = SKI_PREAD;
        int *const mode = list_input_read() ? &copy : &list_input_mode;
        ski_rbuf rb = { NULL, 0 };
        for (i = sa; i < sb && ps.state != P_STOP; ) {
            const size_t want = (size_t)(sb - i < BLK ? sb - i : BLK);
            (void)ski_feed_span(&ps, t, fd, i, want, mode, &rb, BLK, NULL);      /* (never short: there is a mapping) */
            i += want;
        }
        free(rb.buf);
    }
    close(fd);
    if (ps.state != P_STOP && sb < it->size && sb > sa)
        ok = parser_between_records(&ps) && (t[sb] == 0x3e || t[sb] == 0x40);
    /* a FASTQ record whose quality does not match its sequence ends the FILE for the reference (src/kseq.h:205-209 returns -2,
     * src/genome_compare.c:203 stops reading): the pieces behind this one must not count, and some may have been counted
     * already -- so the run fails rather than report more than the reference would */
    if (ps.state == P_STOP && !ps.sink_rc && ps.end_kind == SKP_END_TRUNC && sb < it->size) ok = 0;
    if (ps.state != P_STOP) parser_eof(&ps);
    if (nrecords) *nrecords = ps.nrecords;
    {
        const int sink_rc = ps.sink_rc;
        parser_free(&ps);
        munmap((void *)t, (size_t)it->size);
        if (sink_rc) return sink_rc;
    }
    return ok ? SK_OK : SK_E_SPLIT;
}

/* ---- one .gz item inflated by several threads (pipe > 1): its text comes faster than one thread parses it (16 inflating
 * threads: 9.5 GB/s; the parser: 5-7 GB/s).  The item's thread only CUTS the text into segments of about a chunk's worth, each
 * ending at a line start that looks like a record start (parser_guess_start); a few helper threads parse the segments as files
 * of their own into their own page-locked buffers and CHECK that they end between two records (parser_between_records) -- the
 * first segment starts at the file's start, every other at the checked end of the one before, so if all checks hold the
 * segments' records are the file's records (src/kseq.h:171-211 reads from the top; nothing here changes what a record is).
 * Counters are sums: the order in which segments reach the device does not matter.  A failed check, or a record that ends the
 * file for the reference (FASTQ quality of the wrong length, :205-209) in a segment that is not the last, fails the scan
 * (SK_E_SPLIT) -- later segments may have been counted already; SK_NO_SPLIT=1 parses on one thread.
 * MEASURED (tools/one_gz_bench.py, profiles/r02_one_gz.txt; one 3 Gbase .gz, 16 inflating threads): it LOSES -- FASTA.gz
 * 7.4 Gbase/s with the one parser, 5.1 with four helpers; FASTQ.gz 5.0 against 2.6-4.8.  Gathering the text into segments is
 * one more copy of every byte on the cutting thread, which is about what parsing it costs, and FASTQ is bound by the inflate
 * (9.5 GB/s of text = 4.6 Gbase/s) either way.  So it runs only when SK_PARSE_THREADS asks for it (tests do). */
typedef struct gz_seg { unsigned char *buf; size_t n; int is_last; struct gz_seg *next; } gz_seg;
typedef struct {
    scan_pool *pool;
    pthread_mutex_t mu; pthread_cond_t cv;
    gz_seg *head, *tail;
    int nq, done, stop, rc;
    uint64_t bases; int64_t nrec;
    skpc_writer *fill;                 /* the item's cache file being written (or NULL): every helper's chunks go there */
    int slot;                          /* the item's slot (prevalence): the helpers' chunks are their parent's item's */
} gz_split;

static void *gz_split_worker(void *arg)
{
    gz_split *g = (gz_split *)arg;
    scan_worker w;
    worker_init(&w, g->pool);
    w.fill = g->fill;
    w.slot = g->slot;
    for (;;) {
        gz_seg *sg;
        int stop;
        pthread_mutex_lock(&g->mu);
        while (!g->head && !g->done) pthread_cond_wait(&g->cv, &g->mu);
        sg = g->head;
        if (!sg) { pthread_mutex_unlock(&g->mu); break; }
        g->head = sg->next;
        if (!g->head) g->tail = NULL;
        g->nq--;
        stop = g->stop;
        pthread_cond_broadcast(&g->cv);
        pthread_mutex_unlock(&g->mu);
        if (!stop) {
            stream_writer sw;
            parser ps;
            int ok = 1;
            memset(&sw, 0, sizeof sw);
            sw.cap = POOL_CHUNK; sw.sink = worker_sink; sw.user = &w; sw.next_buf = worker_next_buf;
            parser_init(&ps, writer_record, &sw);
            parser_feed(&ps, sg->buf, sg->n);
            if (!sg->is_last) {
                if (ps.state == P_STOP) ok = ps.sink_rc != 0 || ps.end_kind != SKP_END_TRUNC;   /* (a sink error is reported as itself) */
                else ok = parser_between_records(&ps);
            }
            if (ps.state != P_STOP) parser_eof(&ps);
            writer_flush(&sw);
            if (w.fill && !sw.rc) sw.rc = worker_fill_flush(&w);
            pthread_mutex_lock(&g->mu);
            g->bases += sw.bases;
            g->nrec += ps.nrecords;
            if (sw.rc && !g->rc) g->rc = sw.rc;
            if (!ok && !g->rc) g->rc = SK_E_SPLIT;
            if (!ok || sw.rc) g->stop = 1;
            pthread_mutex_unlock(&g->mu);
            parser_free(&ps);
        }
        free(sg->buf);
        free(sg);
    }
    worker_done(&w);
    return NULL;
}

/* a segment of the cutter's (sk_input.h) into the helpers' queue; they free it */
static void gz_split_push(gz_split *g, unsigned char *buf, size_t n, int is_last, int limit)
{
    gz_seg *sg = (gz_seg *)calloc(1, sizeof *sg);
    sg->buf = buf; sg->n = n; sg->is_last = is_last;
    pthread_mutex_lock(&g->mu);
    while (g->nq >= limit && !g->stop) pthread_cond_wait(&g->cv, &g->mu);
    if (g->tail) g->tail->next = sg; else g->head = sg;
    g->tail = sg;
    g->nq++;
    pthread_cond_broadcast(&g->cv);
    pthread_mutex_unlock(&g->mu);
}

/* records (or a negative SK_E_*); -100: not a gzip file / no helper could be started -- the caller parses it the ordinary way */
static int64_t parse_gz_split(scan_worker *w, const scan_item *it, uint64_t *bases)
{
    skzp zp;
    gz_split g;
    pthread_t th[8];
    const char *e = getenv("SK_PARSE_THREADS");
    int npar = e ? atoi(e) : 0, nth = 0, i;          /* off unless asked for: measured, it loses -- see the comment above */
    ski_cutter cut;
    unsigned char *seg; size_t seg_n;
    if (npar < 2) return -100;
    if (npar > 8) npar = 8;
    if (skzp_open_threads(&zp, it->path, w->pool->pipe) != SKZ_OK) return -100;
    memset(&g, 0, sizeof g);
    g.pool = w->pool;
    g.fill = w->fill;
    g.slot = w->slot;
    pthread_mutex_init(&g.mu, NULL);
    pthread_cond_init(&g.cv, NULL);
    for (i = 0; i < npar; i++) if (pthread_create(&th[nth], NULL, gz_split_worker, &g) == 0) nth++;
    if (nth == 0) { skzp_close(&zp); pthread_mutex_destroy(&g.mu); pthread_cond_destroy(&g.cv); return -100; }
    ski_cutter_init(&cut, POOL_CHUNK / 2 < (1u << 20) ? POOL_CHUNK : POOL_CHUNK / 2);
    for (;;) {
        const unsigned char *data = NULL;
        size_t n;
        int stop;
        pthread_mutex_lock(&g.mu);
        stop = g.stop;
        pthread_mutex_unlock(&g.mu);
        if (stop) break;
        n = skzp_next(&zp, &data);
        if (n == 0) break;
        ski_cutter_add(&cut, data, n);
        while (ski_cutter_take(&cut, &seg, &seg_n)) gz_split_push(&g, seg, seg_n, 0, nth + 2);      /* (a delivery may hold several segments' worth) */
    }
    ski_cutter_rest(&cut, &seg, &seg_n);
    gz_split_push(&g, seg, seg_n, 1, nth + 2);
    pthread_mutex_lock(&g.mu);
    g.done = 1;
    pthread_cond_broadcast(&g.cv);
    pthread_mutex_unlock(&g.mu);
    for (i = 0; i < nth; i++) pthread_join(th[i], NULL);
    skzp_close(&zp);
    pthread_mutex_destroy(&g.mu);
    pthread_cond_destroy(&g.cv);
    *bases += g.bases;
    return g.rc ? (int64_t)g.rc : g.nrec;
}

#ifdef SK_EXPERIMENTS        /* (make EXPERIMENTS=1; the library that ships has no device-side inflate: DESIGN.md section 7) */
/* SK_GPU_INFLATE=1 (experimental): a .gz item of one member and dynamic blocks only is inflated ON THE DEVICE (sk_inflate.hip: the speculative
 * scheme of sk_gzpar.h, a lane per 16 KiB segment; every guess checked, the chain checked here in the library, the CRC-32 here) and its text
 * parsed by this thread.  -100: not such a file, or a check failed -- the caller decodes it on the host as before, so the bytes are zlib's
 * either way. */
static int64_t parse_gz_on_device(scan_worker *w, const scan_item *it, uint64_t *bases)
{
    int fd;
    struct stat st;
    const unsigned char *m;
    uint64_t want, len = 0;
    uint32_t crc = 0;
    int rc;
    if (!w->pool->gpu_inflate || !w->dev_ok) return -100;
    fd = open(it->path, O_RDONLY);
    if (fd < 0) return -100;                              /* (the ordinary path reports it) */
    if (fstat(fd, &st) != 0 || !S_ISREG(st.st_mode) || st.st_size < 32) { close(fd); return -100; }
    m = (const unsigned char *)mmap(NULL, (size_t)st.st_size, PROT_READ, MAP_PRIVATE, fd, 0);
    close(fd);
    if (m == MAP_FAILED) return -100;
    want = sk_inflate_gz_size(m, (uint64_t)st.st_size);
    if (!want) {
        if (w->pool->gpu_inflate > 1 && m[0] == 0x1f && m[1] == 0x8b) fprintf(stderr, "%s: left to the host decoder (not one member of a size the device path takes)\n", it->path);
        munmap((void *)m, (size_t)st.st_size);
        return -100;
    }
    if (!w->inf && sk_inflater_create(sk_ctx_device_(w->pool->ctx), &w->inf) != SK_OK) { w->inf = NULL; munmap((void *)m, (size_t)st.st_size); return -100; }
    if (want > w->text_cap) {
        const uint64_t cap = (want + (64u << 20)) & ~(uint64_t)((64u << 20) - 1);      /* (few distinct sizes: the context keeps what is given back) */
        if (w->text) sk_pinned_free(w->pool->ctx, w->text);
        w->text = NULL; w->text_cap = 0;
        if (sk_pinned_alloc(w->pool->ctx, (void **)&w->text, cap) != SK_OK) { w->text = NULL; munmap((void *)m, (size_t)st.st_size); return -100; }
        w->text_cap = cap;
    }
    {
        const double t0 = now_s();
        double t1;
        rc = sk_inflate_gz(w->inf, m, (uint64_t)st.st_size, w->text, w->text_cap, &len, &crc);
        munmap((void *)m, (size_t)st.st_size);
        t1 = now_s();
        if (rc == SK_OK) { pthread_once(&skz_crc_once, skz_crc_init); if (skz_crc32(0, w->text, (size_t)len) != crc) rc = SK_E_UNSUPPORTED; }
        if (w->pool->gpu_inflate > 1)                      /* (SK_GPU_INFLATE=2: say which way every file went) */
            fprintf(stderr, rc == SK_OK ? "%s: inflated on the device (%llu bytes of text; %.0f ms, CRC-32 %.0f ms)\n"
                                        : "%s: left to the host decoder (a check of the device path did not hold)\n",
                    it->path, (unsigned long long)len, (t1 - t0) * 1e3, (now_s() - t1) * 1e3);
    }
    if (rc != SK_OK) return -100;                         /* (unsupported, or a device hiccup: the host path decides what the file is) */
    {
        stream_writer sw;
        parser ps;
        int64_t nrec;
        uint64_t at;
        memset(&sw, 0, sizeof sw);
        sw.cap = POOL_CHUNK; sw.sink = worker_sink; sw.user = w; sw.next_buf = worker_next_buf;
        parser_init(&ps, writer_record, &sw);
        for (at = 0; at < len && ps.state != P_STOP; at += 4u << 20) parser_feed(&ps, w->text + at, (size_t)(len - at < (4u << 20) ? len - at : (4u << 20)));
        if (ps.state != P_STOP) parser_eof(&ps);
        writer_flush(&sw);
        *bases += sw.bases;
        nrec = ps.nrecords;
        parser_free(&ps);
        return sw.rc ? (int64_t)sw.rc : nrec;
    }
}

#endif

/* the item's cache file is begun: from here on worker_sink writes every chunk to it as well */
static void worker_fill_begin(scan_worker *w, const scan_item *it)
{
    struct stat src;
    memset(&src, 0, sizeof src);
    src.st_size = (off_t)it->size;
    src.st_mtim.tv_sec = (time_t)(it->mtime / 1000000000ll);
    src.st_mtim.tv_nsec = (long)(it->mtime % 1000000000ll);
    w->fill = skpc_begin(it->cpath, &src, POOL_CHUNK);
}

/* decode one item into the worker's pinned buffers; returns records or a negative SK_E_* */
static int64_t worker_item_parse(scan_worker *w, const scan_item *it, uint64_t *bases)
{
    stream_writer sw;
    int64_t nrec = 0;
    int rc;
#ifdef SK_EXPERIMENTS
    if (!it->ranged) {
        const int64_t r = parse_gz_on_device(w, it, bases);
        if (r != -100) return r;
    }
#endif
    if (!it->ranged && w->pool->text) {
        uint64_t resume = TEXT_WHOLE;
        rc = text_scan(w->pool->ctxs, w->pool->nctx, &w->pool->submit_mu, it->path, w->pool->col, bases, &nrec, &resume, &w->tbuf, &w->tcap, w->pool->prev ? w->slot : -1);
        if (rc != TEXT_NOT_TAKEN) {
            if (rc != SK_OK) return rc;
            if (resume == TEXT_WHOLE) return nrec;
            memset(&sw, 0, sizeof sw);
            sw.cap = POOL_CHUNK; sw.sink = worker_sink; sw.user = w; sw.next_buf = worker_next_buf;
            rc = parse_from(it->path, resume, writer_record, &sw, &nrec);
            if (rc == SK_OK) writer_flush(&sw);
            *bases += sw.bases;
            if (rc != SK_OK) return rc;
            return sw.rc ? (int64_t)sw.rc : nrec;
        }
    }
    if (w->fill_item == it) worker_fill_begin(w, it);       /* (the host parser has the whole item) */
    if (!it->ranged && w->pool->pipe > 1 && !getenv("SK_NO_SPLIT") && !getenv("SK_ZLIB")) {
        const int64_t r = parse_gz_split(w, it, bases);
        if (r != -100) return r;
    }
    memset(&sw, 0, sizeof sw);
    sw.buf = NULL;                                   /* (taken through next_buf by the first record: the other buffer may still be read) */
    sw.cap = POOL_CHUNK;
    sw.sink = worker_sink;
    sw.user = w;
    sw.next_buf = worker_next_buf;
    rc = it->ranged ? parse_range(it, writer_record, &sw, &nrec) : parse_file(it->path, writer_record, &sw, &nrec, NULL, w->pool->pipe);
    if (rc == SK_OK || (rc == SK_E_SPLIT && !sw.rc)) writer_flush(&sw);
    *bases += sw.bases;
    if (rc != SK_OK) return rc;
    if (sw.rc) return sw.rc;
    return nrec;
}

/* A cached item: every segment of its file read into this worker's page-locked buffers and submitted as the chunk it was when a decode
 * thread first made it; the stored bases and records are the item's.  -100: the source or the file changed since the list was planned
 * and nothing was counted yet -- the caller parses the source as if there were no cache.  A segment that fails its checksum may come
 * after others were counted: the run fails (SK_E_CACHE) and says which file. */
static int64_t worker_serve(scan_worker *w, const scan_item *it, uint64_t *bases)
{
    scan_pool *const p = w->pool;
    skpc_reader rd;
    skpc_seg sg;
    struct stat st;
    int r, rc = SK_OK;
    const char *why = NULL;
    if (!pc_source_readable(it->path, &st) || skpc_open(&rd, it->cpath, &st, POOL_CHUNK) != SKPC_OK) return -100;
    while (rc == SK_OK && (r = skpc_next(&rd, &sg)) == SKPC_OK) {
        const double t0 = p->timing ? now_s() : 0.0;
        double t1, tsum = 0.0;
        if (sg.kind == SKPC_PACKED) {
            const int i = w->pk_cur ^= 1;
            if (!w->pk[i] && sk_pinned_alloc(p->ctx, (void **)&w->pk[i], sk_packed_bytes(POOL_CHUNK)) != SK_OK) { w->pk[i] = NULL; rc = SK_E_NOMEM; break; }
            if ((rc = worker_pk_wait(w, i)) != SK_OK) break;
            t1 = p->timing ? now_s() : 0.0;
            if ((r = skpc_payload(&rd, &sg, w->pk[i], p->timing ? &tsum : NULL)) != SKPC_OK) break;
            w->pc_bytes += sg.payload_len;
            if (p->timing) { w->t_pc_read += now_s() - t1 - tsum; w->t_pc_sum += tsum; w->t_ticket += t1 - t0; t1 = now_s(); }
            pthread_mutex_lock(&p->submit_mu);
            {
                const double t2 = p->timing ? now_s() : 0.0;
                pool_slot(p, w->slot);
                rc = pool_submit(p, w->pk[i], sg.stream_len, 1, &w->pk_ticket[i]);
                pthread_mutex_unlock(&p->submit_mu);
                if (p->timing) { w->t_submit_wait += t2 - t1; w->t_submit += now_s() - t2; w->nchunks++; w->npacked++; }
            }
            w->pk_used[i] = rc == SK_OK;
            w->pk_kind[i] = 0;
        } else {
            uint8_t *buf = worker_next_buf(w);
            if (!buf) { rc = SK_E_NOMEM; break; }
            t1 = p->timing ? now_s() : 0.0;
            if ((r = skpc_payload(&rd, &sg, buf, p->timing ? &tsum : NULL)) != SKPC_OK) break;
            w->pc_bytes += sg.payload_len;
            if (p->timing) { w->t_pc_read += now_s() - t1 - tsum; w->t_pc_sum += tsum; t1 = now_s(); }
            pthread_mutex_lock(&p->submit_mu);
            {
                const double t2 = p->timing ? now_s() : 0.0;
                pool_slot(p, w->slot);
                rc = pool_submit(p, buf, sg.stream_len, 0, &w->ticket[w->cur]);
                pthread_mutex_unlock(&p->submit_mu);
                if (p->timing) { w->t_submit_wait += t2 - t1; w->t_submit += now_s() - t2; w->nchunks++; }
            }
            w->used[w->cur] = rc == SK_OK;
        }
    }
    if (rc == SK_OK && r != SKPC_MISS) why = r == SKPC_IO ? "it cannot be read" : "a segment does not match its checksum";
    if (why) {
        fprintf(p->err ? p->err : stderr, "libstrainer_kmer: the pack cache file %s is damaged (%s) and part of it may have been counted: "
                                          "nothing is reported; remove the file and run again\n", it->cpath, why);
        rc = SK_E_CACHE;
    }
    if (rc == SK_OK) *bases += rd.h.bases;
    r = rc == SK_OK;
    {
        const int64_t nrec = (int64_t)rd.h.records;
        skpc_close(&rd);
        return r ? nrec : (int64_t)rc;
    }
}

/* one item: served from its cache file, or parsed -- and then, where the plan says so, written to one */
static int64_t worker_item(scan_worker *w, const scan_item *it, uint64_t *bases)
{
    scan_pool *const p = w->pool;
    uint64_t served = 0, written = 0, stale = 0, not_cached = 0;
    const uint64_t b0 = *bases;
    double tsum = 0.0, twrite = 0.0;
    int64_t r = -100;
    if (it->cache == PC_SERVE && (r = worker_serve(w, it, bases)) != -100) served = r >= 0;
    else {
        if (it->cache == PC_SERVE) stale = 1;              /* (changed since the plan: parsed, and in rw mode written anew) */
        w->fill_item = it->cache == PC_FILL || (it->cache == PC_SERVE && p->pc_rw) ? it : NULL;
        r = worker_item_parse(w, it, bases);
        w->fill_item = NULL;
        if (w->fill) {
            const int frc = worker_fill_flush(w);
            tsum = w->fill->t_sum; twrite = w->fill->t_write;
            w->pc_bytes += w->fill->h.payload_bytes;
            written = (uint64_t)skpc_end(w->fill, r >= 0 && frc == SK_OK, r >= 0 ? (uint64_t)r : 0, *bases - b0);
            w->fill = NULL;
            w->pend = 0;
            if (r >= 0 && frc != SK_OK) r = frc;
            not_cached = !written && r >= 0;
        } else if (it->cache && r >= 0) not_cached = 1;     /* (the device text parser took it, ro mode, or the file could not be begun) */
    }
    if (it->cache) {
        pthread_mutex_lock(&p->queue_mu);
        p->pc_served += served; p->pc_written += written; p->pc_stale += stale; p->pc_not += not_cached;
        p->pc_t_sum += tsum + w->t_pc_sum; p->pc_t_read += w->t_pc_read; p->pc_t_write += twrite; p->pc_bytes += w->pc_bytes;
        pthread_mutex_unlock(&p->queue_mu);
        w->t_pc_sum = w->t_pc_read = 0.0; w->pc_bytes = 0;
    }
    return r;
}

/* skh_scan_file with the cache on: the file as a list of one item (the list walk's worker serves or fills it).  *handled = 0: not a
 * regular file, no usable directory, nothing to serve and nothing to write -- the caller scans it as before. */
static int scan_file_cached(sk_ctx *ctx, const char *path, uint32_t col, uint64_t *bases, const char *dir, int mode, int *handled)
{
    scan_pool pool;
    scan_worker w;
    scan_item it;
    skpc_reader rd;
    struct stat st;
    sk_ctx *one = ctx;
    uint64_t b = 0, stale = 0;
    int64_t r;
    int o;
    const char *e = getenv("SK_LIST_PACK");
    *handled = 0;
    if (!pc_source_readable(path, &st) || !pc_dir_usable(dir, mode, stderr)) return SK_OK;     /* (missing, unreadable: as without the cache) */
    memset(&it, 0, sizeof it);
    if (!(it.cpath = skpc_path(dir, path))) return SK_OK;
    o = skpc_open(&rd, it.cpath, &st, POOL_CHUNK);
    if (o == SKPC_OK) { skpc_close(&rd); it.cache = PC_SERVE; }
    else {
        stale = o == SKPC_INVALID;
        if (mode == SKPC_RW && !text_wanted(ctx, 0)) it.cache = PC_FILL;
    }
    if (!it.cache) { pc_count(ctx, 0, 0, stale, 1); free(it.cpath); return SK_OK; }
    it.path = (char *)(uintptr_t)path; it.size = (uint64_t)st.st_size; it.mtime = skpc_mtime_ns(&st); it.reg = 1;
    memset(&pool, 0, sizeof pool);
    pool.ctx = ctx; pool.ctxs = &one; pool.nctx = 1; pool.col = col;
    pool.pack = e && e[0] == '0' ? 0 : e && e[0] == '2' ? 2 : 1;
    pool.err = stderr;
    pool.pc_rw = mode == SKPC_RW;
    pthread_mutex_init(&pool.submit_mu, NULL);
    pthread_mutex_init(&pool.queue_mu, NULL);
    worker_init(&w, &pool);
    r = worker_item(&w, &it, &b);
    worker_done(&w);
    pc_count(ctx, pool.pc_served, pool.pc_written, pool.pc_stale + stale, pool.pc_not);
    pthread_mutex_destroy(&pool.submit_mu);
    pthread_mutex_destroy(&pool.queue_mu);
    free(it.cpath);
    if (bases) *bases += b;
    *handled = 1;
    return r < 0 ? (int)r : SK_OK;
}

/* prevalence: where an item ends -- served, parsed or failed part-way -- its slot is folded into the two columns and its record
 * cell; what was scanned does not stay in the slot.  Returns the item's status (a fold that fails makes a good item fail). */
static int64_t worker_item_end(scan_worker *w, const scan_item *it, int64_t rc)
{
    scan_pool *const p = w->pool;
    int frc;
    if (!p->prev) return rc;
    pthread_mutex_lock(&p->submit_mu);
    frc = p->fold ? p->fold(p->fold_user, (uint32_t)w->slot, it->line)
                  : sk_item_fold(p->ctx, (uint32_t)w->slot, p->col, p->prev_col, p->prev_min, p->d_rec + 2u * (size_t)it->line);
    pthread_mutex_unlock(&p->submit_mu);
    return rc >= 0 && frc != SK_OK ? (int64_t)frc : rc;
}

static void *pool_worker(void *arg)
{
    scan_pool *p = (scan_pool *)arg;
    scan_worker w;
    int wrc = worker_init(&w, p);
    pthread_setname_np(pthread_self(), "sk-decode");
    pthread_mutex_lock(&p->queue_mu);
    w.slot = p->worker_ids;
    w.dev_ok = p->worker_ids++ < p->dev_workers;
    pthread_mutex_unlock(&p->queue_mu);
    for (;;) {
        uint32_t i;
        uint64_t bases = 0;
        int64_t rc;
        pthread_mutex_lock(&p->queue_mu);
        i = p->next;
        if (i >= p->nitem || p->rc != SK_OK) { pthread_mutex_unlock(&p->queue_mu); break; }
        p->next++;
        progress_upto(p, p->item[i].line);
        pthread_mutex_unlock(&p->queue_mu);
        {
            const double t0 = p->timing ? now_s() : 0.0;
            rc = wrc != SK_OK ? wrc : worker_item(&w, &p->item[i], &bases);
            rc = worker_item_end(&w, &p->item[i], rc);
            pthread_mutex_lock(&p->queue_mu);
            if (p->prev) p->line_bases[p->item[i].line] = bases;
            if (p->timing) p->t_item += now_s() - t0;
        }
        p->bases += bases;
        if (rc < 0 && (p->rc == SK_OK || i < p->rc_index)) { p->rc = (int)rc; p->rc_index = i; }
        pthread_mutex_unlock(&p->queue_mu);
    }
    if (p->timing) {
        struct timespec ts;
        pthread_mutex_lock(&p->queue_mu);
        p->t_submit_wait += w.t_submit_wait; p->t_submit += w.t_submit; p->t_ticket += w.t_ticket; p->nchunks += w.nchunks;
        p->t_pack += w.t_pack; p->npacked += w.npacked;
        if (clock_gettime(CLOCK_THREAD_CPUTIME_ID, &ts) == 0) p->t_cpu += (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec;
        pthread_mutex_unlock(&p->queue_mu);
    }
    worker_done(&w);
    return NULL;
}

/* the plan: items of the whole list (every rank computes the same), then who takes which */
typedef struct { uint64_t est; uint32_t idx; } plan_key;
static int plan_cmp(const void *a, const void *b)
{
    const plan_key *x = (const plan_key *)a, *y = (const plan_key *)b;
    if (x->est != y->est) return x->est > y->est ? -1 : 1;
    return x->idx < y->idx ? -1 : x->idx > y->idx;
}

/* items[0..n): all items in list order; owner[i] = the rank that scans item i */
static void plan_owners(const scan_item *items, const uint64_t *est, uint32_t n, uint32_t world, uint32_t *owner)
{
    plan_key *k = (plan_key *)malloc(((size_t)n + 1) * sizeof *k);
    uint64_t *load = (uint64_t *)calloc(world, sizeof *load);
    uint32_t i, r;
    (void)items;
    for (i = 0; i < n; i++) { k[i].est = est[i]; k[i].idx = i; }
    qsort(k, n, sizeof *k, plan_cmp);
    for (i = 0; i < n; i++) {
        uint32_t best = 0;
        for (r = 1; r < world; r++) if (load[r] < load[best]) best = r;
        owner[k[i].idx] = best;
        load[best] += k[i].est ? k[i].est : 1;
    }
    free(k); free(load);
}

/* FNV-1a over everything the ranks must agree on: the items (path, byte range, size as seen by stat) and their owners */
static uint64_t fnv_bytes(uint64_t h, const void *p, size_t n)
{
    const unsigned char *b = (const unsigned char *)p;
    while (n--) { h ^= *b++; h *= 0x100000001B3ull; }
    return h;
}
static uint64_t plan_digest(const scan_item *items, const uint32_t *owner, uint32_t n, uint32_t world)
{
    uint64_t h = 0xCBF29CE484222325ull;
    uint32_t i;
    h = fnv_bytes(h, &n, sizeof n);
    h = fnv_bytes(h, &world, sizeof world);
    for (i = 0; i < n; i++) {
        const uint32_t rg = (uint32_t)items[i].ranged;
        h = fnv_bytes(h, items[i].path, strlen(items[i].path) + 1);
        h = fnv_bytes(h, &items[i].a, sizeof items[i].a);
        h = fnv_bytes(h, &items[i].b, sizeof items[i].b);
        h = fnv_bytes(h, &items[i].size, sizeof items[i].size);
        h = fnv_bytes(h, &items[i].line, sizeof items[i].line);
        h = fnv_bytes(h, &rg, sizeof rg);
        h = fnv_bytes(h, &owner[i], sizeof owner[i]);
    }
    return h;
}

#define SK_PLAN_LANES 16u     /* decode lanes per rank the multi-rank plan is laid out for (the programs' thread cap) */

typedef struct { uint64_t *hash; uint32_t *owner; uint32_t cap, *nlines; } plan_report;

/* What a cut that does not hold costs: nothing but time.  Before a list with pieces is scanned the column is copied; if a
 * piece fails its check (SK_E_SPLIT: a record that ends the FILE for the reference in the middle of it, a layout the guess
 * misjudges) the column and the progress file are put back and the list is scanned again UNCUT -- the reference's strict
 * record sequence per file, which reports what the reference reports (src/kseq.h:205-209, src/genome_compare.c:203).
 * The cut is an optimisation that is checked, not a new way to fail.  With several ranks in the library's communicator
 * the same holds (round 4): the plan is global, so EVERY rank copies its column when the plan has pieces, the ranks learn of
 * a failed check through the agreement that closes every list scan, and all of them put their columns back and scan their
 * share of the whole-file plan.  Only a caller that runs ranks WITHOUT the library's communicator still gets SK_E_SPLIT
 * (its other ranks cannot be told from here): it coordinates the same steps itself (strainer2_amd/dist.py:
 * scan_list_sharded) with skh_scan_list_uncut.
 *
 * Collectives: whatever happens to a rank locally -- a list it cannot open, a file only it owns that is
 * missing, a cut that fails -- every rank issues the same sequence: per list scan ONE agreement before (plan hash, "my
 * set-up for this list failed") and ONE after (first unreadable line, "a cut failed", "a device error"), each a max
 * all-reduce of a few words (sk_comm_max_u64), and every rank returns the SAME status, so the callers' decisions
 * (skip the remaining lists, go to the big all-reduce) are the same everywhere. */
typedef struct { uint32_t **snap; uint32_t nsnap; long prog_at; int armed; } split_guard;     /* snap[i]: ctxs[i]'s column */

#define LIST_FAIL_OPEN  1u    /* agreement before the scan: this rank could not read the list itself */
#define LIST_FAIL_GUARD 2u    /*                            ... could not copy its column (no memory, device error) */

/* prevalence (skh_scan_list_prevalence): the second column, the threshold, and where the items' records go.  With `fold`
 * (skh_scan_list_many_prevalence) the walk makes no slots, no folds and no records of its own: every context has `nslots` item slots
 * already, at most that many decode threads run -- a thread owns a slot, so the others' items wait for one --, the hook is called
 * where an item ends, and the items handed out carry their bases alone */
typedef struct { uint32_t prev_col, min_count; skh_prev_items *items; skh_item_fold_fn fold; void *fold_user; uint32_t nslots; } prev_opts;

static int scan_list_once(sk_ctx *const *ctxs, uint32_t nctx, const char *list_path, const char *skip, uint32_t col, FILE *progress,
                          FILE *err, uint32_t rank, uint32_t world, uint64_t *bases, int plan_only, const plan_report *report,
                          int no_split, split_guard *guard, const prev_opts *pv)
{
    sk_ctx *const ctx = ctxs ? ctxs[0] : NULL;       /* (plan only: no context) */
    FILE *fp = fopen(list_path, "r");
    char *line = NULL, *nl;
    size_t cap = 0;
    uint32_t nline = 0, nall = 0, acap = 0, lcap = 0, i;
    int nthreads = 1;
    const char *env = getenv("SK_THREADS");
    scan_pool pool;
    scan_item *all = NULL;
    uint64_t *est = NULL, total = 0, plan_hash = 0;
    uint32_t *owner = NULL;
    uint64_t local_fail = 0;
    uint32_t open_line = UINT32_MAX;            /* the first list line whose file some rank could not open */
    int any_ranged = 0, coordinated, by_other = 0;
    char *pc_dir = NULL;                        /* the packed input cache's directory for this scan (NULL: none) */
    int pc_mode = SKPC_RW, pc_asked = 0;
    int prev_failed = 0;                        /* prevalence: the slots or the record array could not be made */
    if (world == 0) world = 1;
    /* several ranks act together only when all of them are in the library's communicator */
    coordinated = world <= 1 || (ctx && (uint32_t)sk_comm_world(ctx) == world);
    if (!fp) {
        if (err) fprintf(err, "could not read file %s in GEN_all_kmer_counts()\n", list_path);
        if (!ctx || plan_only || world <= 1 || !coordinated) return SK_E_OPEN;
        local_fail |= LIST_FAIL_OPEN;                       /* (the other ranks are waiting in the agreement below) */
    }
    if (no_split == 2) local_fail |= LIST_FAIL_GUARD;       /* (second scan after a failed cut: this rank could not put its column back) */
    memset(&pool, 0, sizeof pool);
    pool.timing = getenv("SK_TIMING") != NULL;
    { const char *e = getenv("SK_LIST_PACK"); pool.pack = e && e[0] == '0' ? 0 : e && e[0] == '2' ? 2 : 1; }      /* (0: never, 2: always -- tests --, default: plain-text items' chunks once the scan is bound by the link) */
    pool.ctx = ctx;
    pool.ctxs = ctxs;
    pool.nctx = ctxs ? nctx : 0;
    pool.col = col;
    pool.err = err;
    pool.text = ctx && !plan_only ? text_wanted(ctx, pool.timing) : (getenv("SK_DEVICE_PARSE") && getenv("SK_DEVICE_PARSE")[0] == '1' && sk_scan_text_pinned_many != NULL);
    pthread_mutex_init(&pool.submit_mu, NULL);
    pthread_mutex_init(&pool.queue_mu, NULL);
    if (env) nthreads = atoi(env);
    else { long n = sk_cpu_budget(); nthreads = n > 16 ? 16 : (int)n; }
    if (nthreads < 1) nthreads = 1;

    /* the list's lines; what the reference says about each of them (progress line, skip message) is said in list
     * order: the progress line when a decode thread takes the line's file, the skip messages behind the scans */
    while (fp && getline(&line, &cap, fp) != -1) {
        struct stat st;
        if ((nl = strchr(line, '\n')) != NULL) *nl = '\0';
        if (nline == lcap) { lcap = lcap ? lcap * 2 : 64; pool.ll = (list_line *)realloc(pool.ll, lcap * sizeof *pool.ll); }
        memset(&pool.ll[nline], 0, sizeof pool.ll[nline]);
        pool.ll[nline].text = strdup(line);
        if (skip && strcmp(skip, line) == 0) {
            pool.ll[nline++].skipped = 1;
            continue;
        }
        if (nall == acap) { acap = acap ? acap * 2 : 64; all = (scan_item *)realloc(all, acap * sizeof *all); }
        memset(&all[nall], 0, sizeof all[nall]);
        all[nall].path = strdup(line);
        all[nall].line = nline++;
        all[nall].reg = stat(line, &st) == 0 && S_ISREG(st.st_mode);
        all[nall].size = all[nall].reg ? (uint64_t)st.st_size : 0;
        all[nall].mtime = all[nall].reg ? skpc_mtime_ns(&st) : 0;
        nall++;
    }
    free(line);
    if (fp) fclose(fp);
    pool.nll = nline;
    pool.progress = rank == 0 ? progress : NULL;

    /* The packed input cache (opt-in).  Which items a cache file serves is decided HERE, with the plan: the source must be a regular
     * file whose size and mtime are the header's, the file of this version and k and exactly as long as its header implies.  Such an
     * item stays whole -- never cut into ranges, never sent to the device text parser.  A source that is missing is none of the
     * cache's business: it fails where it failed before.  With several ranks the option is ignored (the items count as not cached). */
    if (ctx && !plan_only && (pc_dir = pc_effective(ctx, &pc_mode)) != NULL) {
        pc_asked = 1;
        if (world > 1 || !pc_dir_usable(pc_dir, pc_mode, err)) { free(pc_dir); pc_dir = NULL; }
        pool.pc_rw = pc_dir && pc_mode == SKPC_RW;
    }
    for (i = 0; pc_dir && i < nall; i++) {
        skpc_reader rd;
        struct stat st;
        int o;
        if (!all[i].reg || !(all[i].cpath = skpc_path(pc_dir, all[i].path))) continue;
        memset(&st, 0, sizeof st);
        st.st_size = (off_t)all[i].size;
        st.st_mtim.tv_sec = (time_t)(all[i].mtime / 1000000000ll); st.st_mtim.tv_nsec = (long)(all[i].mtime % 1000000000ll);
        o = skpc_open(&rd, all[i].cpath, &st, POOL_CHUNK);
        if (o == SKPC_OK) {
            struct stat now;
            skpc_close(&rd);
            /* a source that cannot be opened is not served: it goes the old way and fails there, as it does without the cache */
            if (pc_source_readable(all[i].path, &now)) all[i].cache = PC_SERVE;
            else { free(all[i].cpath); all[i].cpath = NULL; }
        } else {
            pool.pc_stale += o == SKPC_INVALID;
            if (pc_mode == SKPC_RW) all[i].cache = PC_FILL; else pool.pc_not++;
        }
    }

    /* cut big plain-text files into pieces (never with one thread and one rank: that is the reference's strict sequence).
     * With several ranks the plan must be the SAME on every rank, so it is a function of the list, the files' sizes and
     * the world size only: a fixed number of decode lanes per rank stands in for the local thread count (which follows
     * SK_THREADS, the cgroup quota, LOCAL_WORLD_SIZE ... and may differ from rank to rank) -- and the ranks compare a
     * hash of their plans before any of them scans (below). */
    {
        const uint64_t lanes = world > 1 ? (uint64_t)world * SK_PLAN_LANES : (uint64_t)(nthreads > 1 ? nthreads : 1);
        uint64_t target, floor_bytes = 32u << 20;
        uint32_t n0 = nall, out = 0;
        scan_item *cut;
        uint64_t *gz = (uint64_t *)calloc((size_t)nall + 1, sizeof *gz);
        for (i = 0; i < nall; i++) {
            unsigned char magic[2] = {0, 0};
            FILE *f = all[i].size ? fopen(all[i].path, "rb") : NULL;
            if (f) { if (fread(magic, 1, 2, f) != 2) magic[0] = 0; fclose(f); }
            gz[i] = magic[0] == 0x1f && magic[1] == 0x8b;
            total += gz[i] ? all[i].size * 4 : all[i].size;           /* (a .gz FASTQ inflates about fourfold) */
        }
        target = total / (4 * lanes);
        if ((env = getenv("SK_SPLIT_FLOOR_BYTES")) != NULL && atoll(env) > 0) floor_bytes = (uint64_t)atoll(env);   /* (tests) */
        if (target < floor_bytes) target = floor_bytes;
        if ((env = getenv("SK_SPLIT_BYTES")) != NULL && atoll(env) > 0) target = (uint64_t)atoll(env);     /* (tests) */
        {   /* how many items there will be */
            size_t total_items = 0;
            for (i = 0; i < n0; i++) {
                uint64_t np = 1;
                if (lanes > 1 && !gz[i] && !no_split && !(pool.text && world <= 1) && !getenv("SK_NO_SPLIT") && all[i].size >= 2 * target && all[i].cache != PC_SERVE) np = (all[i].size + target - 1) / target;
                total_items += np > 256 ? 256 : (size_t)np;
            }
            cut = (scan_item *)malloc((total_items + 1) * sizeof *cut);
            est = (uint64_t *)malloc((total_items + 1) * sizeof *est);
        }
        for (i = 0; i < n0; i++) {
            uint32_t np = 1, k;
            if (lanes > 1 && !gz[i] && !no_split && !(pool.text && world <= 1) && !getenv("SK_NO_SPLIT") && all[i].size >= 2 * target && all[i].cache != PC_SERVE) {
                np = (uint32_t)((all[i].size + target - 1) / target > 256 ? 256 : (all[i].size + target - 1) / target);
            }
            if (np > 1 && all[i].cache) { all[i].cache = 0; pool.pc_not++; }      /* (an item in byte ranges is not written in this version) */
            if (np > 1) { free(all[i].cpath); all[i].cpath = NULL; }
            for (k = 0; k < np; k++) {
                cut[out] = all[i];
                if (k) cut[out].path = strdup(all[i].path);
                cut[out].ranged = np > 1;
                cut[out].a = all[i].size / np * k;
                cut[out].b = k + 1 == np ? all[i].size : all[i].size / np * (k + 1);
                est[out] = np > 1 ? cut[out].b - cut[out].a : (gz[i] ? all[i].size * 4 : all[i].size);
                out++;
            }
        }
        free(all); free(gz);
        all = cut; nall = out;
    }
    owner = (uint32_t *)malloc(((size_t)nall + 1) * sizeof *owner);
    plan_owners(all, est, nall, world, owner);
    plan_hash = plan_digest(all, owner, nall, world);
    if (pv) {                                             /* the uncut plan with prevalence is another plan than the uncut plan */
        const uint32_t w[4] = {0x76657270u, pv->prev_col, pv->min_count, nline};
        plan_hash = fnv_bytes(plan_hash, w, sizeof w);
    }
    if (report && report->hash) *report->hash = plan_hash;
    if (report && report->nlines) *report->nlines = nline;
    if (report && report->owner) {                        /* who scans which list line (SKH_PLAN_SKIPPED / SKH_PLAN_SHARED) */
        for (i = 0; i < nline && i < report->cap; i++) report->owner[i] = SKH_PLAN_SKIPPED;
        for (i = 0; i < nall; i++)
            if (all[i].line < report->cap) {
                uint32_t *o = &report->owner[all[i].line];
                *o = *o == SKH_PLAN_SKIPPED || *o == owner[i] ? owner[i] : SKH_PLAN_SHARED;
            }
    }
    for (i = 0; i < nall; i++) any_ranged |= all[i].ranged;
    {
        uint32_t rows_any = 0, c;
        for (c = 0; ctx && c < nctx; c++) rows_any |= sk_table_rows(ctxs[c]);
        if (guard && ctx && !plan_only && !no_split && coordinated && any_ranged && rows_any) {
            /* pieces ahead (somewhere in the plan: on every rank, then): keep what a failed cut would spoil -- the column of
             * every context the chunks go to */
            int ok = (guard->snap = (uint32_t **)calloc(nctx, sizeof *guard->snap)) != NULL;
            if (ok) guard->nsnap = nctx;
            for (c = 0; ok && c < nctx; c++) {
                if (!sk_table_rows(ctxs[c])) continue;
                guard->snap[c] = (uint32_t *)malloc((size_t)sk_table_rows(ctxs[c]) * sizeof(uint32_t));
                ok = guard->snap[c] && sk_counts_fetch(ctxs[c], col, guard->snap[c]) == SK_OK;
            }
            if (ok) {
                guard->prog_at = progress ? (fflush(progress), ftell(progress)) : -1;
                guard->armed = 1;
            } else local_fail |= LIST_FAIL_GUARD;
        }
    }
    if (ctx && !plan_only) {                            /* (a world of one with a communicator -- SK_FORCE_COMM -- takes the same road: tests) */
        /* The agreement before the scan.  Local settings that change the plan (SK_SPLIT_BYTES, SK_NO_SPLIT) or a file whose
         * size another rank sees differently would have byte ranges scanned twice or never and the summed table silently
         * wrong: every rank leaves instead (SK_E_PLAN) -- and so does every rank when ONE of them could not read the list or
         * copy its column.  (Without an in-library communicator -- a caller that reduces the counters itself -- the caller
         * compares skh_list_plan_hash() through its own collective.) */
        uint64_t v[3];
        int arc;
        v[0] = plan_hash; v[1] = ~plan_hash; v[2] = local_fail;
        arc = sk_comm_max_u64(ctx, v, 3);
        if (arc != SK_OK) {
            if (err) fprintf(err, "kmer_scrub_count: %s (%s)\n", sk_strerror(arc), sk_last_error(ctx));
            pool.rc = arc; plan_only = 1;
        } else if (v[2] & LIST_FAIL_OPEN) {
            if (err && !(local_fail & LIST_FAIL_OPEN)) fprintf(err, "kmer_scrub_count: another rank could not read %s; nothing is reported\n", list_path);
            pool.rc = SK_E_OPEN; plan_only = 1;
        } else if (v[2] & LIST_FAIL_GUARD) {
            if (err) fprintf(err, "kmer_scrub_count: %s could not keep a copy of its counters before cutting the files of %s\n",
                             (local_fail & LIST_FAIL_GUARD) ? "this rank" : "another rank", list_path);
            pool.rc = SK_E_NOMEM; plan_only = 1;
        } else if (v[0] != plan_hash || v[1] != ~plan_hash) {
            if (err) fprintf(err, "kmer_scrub_count: the ranks computed different work plans for %s (rank %u: %016llx) -- check "
                                  "SK_SPLIT_BYTES / SK_NO_SPLIT and that every rank sees the same files; nothing is reported\n",
                             list_path, rank, (unsigned long long)plan_hash);
            pool.rc = SK_E_PLAN; plan_only = 1;           /* (fall through to the clean-up) */
        }
    }
    pool.item = (scan_item *)malloc(((size_t)nall + 1) * sizeof *pool.item);
    for (i = 0; i < nall; i++) {
        if (owner[i] == rank) pool.item[pool.nitem++] = all[i];
        else { free(all[i].path); free(all[i].cpath); }
    }
    if (pc_asked && world > 1 && !plan_only) pool.pc_not += pool.nitem;
    free(all); free(est); free(owner);

    {   /* with fewer files than half the cores, a file's inflate and its record parsing take a core each; with
         * fewer still, the threads left over inflate inside the files (a speculative segment costs about twice a
         * serial one, so it takes three threads per file to be worth it).  SK_GZ_THREADS sets the number per file. */
        const long ncpu = sk_cpu_budget();
        const char *gzt = getenv("SK_GZ_THREADS");
        pool.pipe = nthreads > 1 && (long)pool.nitem * 2 <= ncpu;
        if (pool.pipe && pool.nitem && nthreads / (int)pool.nitem >= 3) pool.pipe = nthreads / (int)pool.nitem;
        if (gzt && nthreads > 1) pool.pipe = atoi(gzt) < 1 ? 1 : atoi(gzt);
        if (pool.pipe > 16) pool.pipe = 16;
#ifdef SK_EXPERIMENTS
        pool.gpu_inflate = getenv("SK_GPU_INFLATE") ? atoi(getenv("SK_GPU_INFLATE")) : 0;
        if (pool.gpu_inflate && nthreads > 1) {               /* the device's decoder is fed by threads of its own, beside the host's decode threads */
            pool.dev_workers = getenv("SK_GPU_INFLATE_WORKERS") ? atoi(getenv("SK_GPU_INFLATE_WORKERS")) : 4;
            if (pool.dev_workers < 0) pool.dev_workers = 0;
            if (pool.dev_workers > 16) pool.dev_workers = 16;
            nthreads += pool.dev_workers;
        }
#endif
    }
    if (pv && pv->fold && !plan_only && pool.nitem) {       /* the caller's slots and folds: a decode thread per slot at the most */
        if ((uint32_t)nthreads > pv->nslots) { nthreads = (int)pv->nslots; if (nthreads == 1) pool.pipe = 0; }
        pool.line_bases = (uint64_t *)calloc((size_t)nline + 1, sizeof *pool.line_bases);
        if (!pool.line_bases) { pool.rc = SK_E_NOMEM; pool.rc_index = 0; prev_failed = 1; }
        else { pool.prev = 1; pool.fold = pv->fold; pool.fold_user = pv->fold_user; }
    } else
    if (pv && !plan_only && pool.nitem) {
        /* a slot per decode thread, a record cell per list line (the cells of lines this rank does not own stay zero) */
        const uint32_t nslots = nthreads == 1 ? 1u : (uint32_t)nthreads > pool.nitem ? pool.nitem : (uint32_t)nthreads;
        const size_t rbytes = (size_t)nline * 2u * sizeof(uint64_t);
        int prc;
        pool.prev_col = pv->prev_col; pool.prev_min = pv->min_count;
        pool.line_bases = (uint64_t *)calloc((size_t)nline + 1, sizeof *pool.line_bases);
        prc = pool.line_bases ? sk_item_slots(ctx, nslots) : SK_E_NOMEM;
        if (prc == SK_OK) prc = sk_dev_alloc(ctx, (void **)&pool.d_rec, rbytes);
        if (prc == SK_OK) {
            uint64_t *z = (uint64_t *)calloc((size_t)nline * 2u + 1, sizeof *z);
            prc = z ? sk_dev_upload(ctx, pool.d_rec, z, rbytes) : SK_E_NOMEM;
            free(z);
        }
        if (prc != SK_OK) {
            if (err) fprintf(err, "kmer_scrub_count: no room for %u item slots (--prevalence): %s (%s)\n", nslots, sk_strerror(prc), sk_last_error(ctx));
            pool.rc = prc; pool.rc_index = 0; prev_failed = 1;
        } else {
            pool.prev = 1;
            if (pool.timing && sk_item_fold_timing_) (void)sk_item_fold_timing_(ctx, 1, NULL, NULL);
            if (pool.timing && err)
                fprintf(err, "kmer_scrub_count timing: prevalence: %s: %u item slots take %.1f MB of HBM\n", list_path, nslots,
                        1e-6 * (double)nslots * (2.0 * (double)sk_table_rows(ctx) + 8.0) * 4.0);
        }
    }
    if (plan_only || prev_failed) {
        /* nothing is scanned */
    } else if (nthreads == 1) {                               /* strict sequence, as the reference */
        scan_worker seq;
        int seq_rc = SK_OK;
        if (pool.nitem) seq_rc = worker_init(&seq, &pool);
        for (i = 0; i < pool.nitem; i++) {
            uint64_t b = 0;
            int64_t rc;
            progress_upto(&pool, pool.item[i].line);
            rc = seq_rc != SK_OK ? seq_rc : worker_item(&seq, &pool.item[i], &b);
            if (seq_rc == SK_OK) rc = worker_item_end(&seq, &pool.item[i], rc);
            if (pool.prev) pool.line_bases[pool.item[i].line] = b;
            pool.bases += b;
            if (rc < 0) { pool.rc = (int)rc; pool.rc_index = i; break; }
        }
        if (pool.nitem) worker_done(&seq);
    } else if (pool.nitem) {
        pthread_t *th;
        if ((uint32_t)nthreads > pool.nitem) nthreads = (int)pool.nitem;
        th = (pthread_t *)malloc((size_t)nthreads * sizeof *th);
        for (i = 0; i < (uint32_t)nthreads; i++) pthread_create(&th[i], NULL, pool_worker, &pool);
        for (i = 0; i < (uint32_t)nthreads; i++) pthread_join(th[i], NULL);
        free(th);
        if (pool.timing && err)
            fprintf(err, "kmer_scrub_count timing: %s: %d decode threads, %u items, %llu chunks; summed over the threads: in items %.2f s, "
                         "of it on a core %.2f s, waiting for the submit lock %.2f s, inside the submit %.2f s, waiting for a buffer's copy %.2f s, "
                         "packing %.2f s (%llu chunks went up packed)\n",
                    list_path, nthreads, pool.nitem, (unsigned long long)pool.nchunks, pool.t_item, pool.t_cpu, pool.t_submit_wait,
                    pool.t_submit, pool.t_ticket, pool.t_pack, (unsigned long long)pool.npacked);
    }
    if (!plan_only && ctx) {
        /* The agreement after the scan: what went wrong, anywhere.  The first list line whose file could not be opened (the
         * reference stops there: the earliest line wins), "a cut did not hold", "a device error" -- one max all-reduce, and
         * from here on every rank holds the same status. */
        uint64_t v[3] = {0, 0, 0};
        int arc;
        if (pool.rc == SK_E_OPEN) v[0] = (uint64_t)UINT32_MAX - pool.item[pool.rc_index].line + 1;       /* (larger = earlier) */
        else if (pool.rc == SK_E_SPLIT) v[1] = 1;
        else if (pool.rc != SK_OK) v[2] = (uint64_t)(uint32_t)(-pool.rc);
        arc = sk_comm_max_u64(ctx, v, 3);
        if (arc != SK_OK) {
            if (err) fprintf(err, "kmer_scrub_count: %s (%s)\n", sk_strerror(arc), sk_last_error(ctx));
            pool.rc = arc; by_other = 1;
        } else if (v[2]) {
            if (pool.rc == SK_OK || pool.rc == SK_E_OPEN || pool.rc == SK_E_SPLIT) {
                pool.rc = -(int)(uint32_t)v[2]; by_other = 1;
                if (err) fprintf(err, "kmer_scrub_count: another rank reported an error while scanning %s: %s\n", list_path, sk_strerror(pool.rc));
            }
        } else if (v[0]) {
            open_line = (uint32_t)((uint64_t)UINT32_MAX - (v[0] - 1));
            if (!(pool.rc == SK_E_OPEN && pool.item[pool.rc_index].line == open_line)) by_other = 1;   /* (the line's owner says which file) */
            pool.rc = SK_E_OPEN;
        } else if (v[1]) {
            if (pool.rc != SK_E_SPLIT) by_other = 1;
            pool.rc = SK_E_SPLIT;
        }
    }
    if (pv && !plan_only && ctx && nline) {
        /* The items' records: every rank hands in its own lines' cells {kmers_present, kmer_hits, bases}, one max all-reduce makes them
         * everybody's -- issued here by every rank whatever failed where (a rank that scanned nothing hands in zeros). */
        uint64_t *v = (uint64_t *)calloc((size_t)nline * 3u + 1, sizeof *v), *r2 = (uint64_t *)calloc((size_t)nline * 2u + 1, sizeof *r2);
        int rrc = v && r2 ? SK_OK : SK_E_NOMEM, arc;
        if (pool.prev && pool.fold) {
            uint32_t c;
            for (c = 0; c < nctx; c++) (void)sk_item_slot(ctxs[c], -1);
            for (i = 0; rrc == SK_OK && i < nline; i++) v[3u * i + 2] = pool.line_bases[i];
        } else
        if (pool.prev) {
            (void)sk_item_slot(ctx, -1);
            if (rrc == SK_OK) rrc = sk_dev_download(ctx, r2, pool.d_rec, (size_t)nline * 2u * sizeof(uint64_t));      /* (waits for the folds) */
            if (pool.timing && sk_item_fold_timing_) {
                double fms = 0.0;
                uint64_t nf = 0;
                (void)sk_item_fold_timing_(ctx, 0, &fms, &nf);
                if (err) fprintf(err, "kmer_scrub_count timing: prevalence: %s: %llu item folds, %.3f ms on the device (%.1f us each)\n", list_path,
                                 (unsigned long long)nf, fms, nf ? 1e3 * fms / (double)nf : 0.0);
            }
            for (i = 0; rrc == SK_OK && i < nline; i++) { v[3u * i] = r2[2u * i]; v[3u * i + 1] = r2[2u * i + 1]; v[3u * i + 2] = pool.line_bases[i]; }
        }
        arc = v ? sk_comm_max_u64(ctx, v, nline * 3u) : SK_OK;
        if (rrc == SK_OK && arc != SK_OK) rrc = arc;
        if (rrc != SK_OK && pool.rc == SK_OK) {
            if (err) fprintf(err, "kmer_scrub_count: the items' records could not be fetched: %s (%s)\n", sk_strerror(rrc), sk_last_error(ctx));
            pool.rc = rrc; by_other = 1;
        }
        if (pool.rc == SK_OK && pv->items) {                  /* one record per item: per list line that was not skipped */
            skh_prev_items *const o = pv->items;
            o->item = (skh_prev_item *)calloc((size_t)nline + 1, sizeof *o->item);
            o->n = 0;
            for (i = 0; o->item && i < nline; i++) {
                skh_prev_item *const t = &o->item[o->n];
                if (pool.ll[i].skipped) continue;
                t->line = i + 1; t->path = strdup(pool.ll[i].text);
                t->kmers_present = v[3u * i]; t->kmer_hits = v[3u * i + 1]; t->bases = v[3u * i + 2];
                o->n++;
            }
            if (!o->item) pool.rc = SK_E_NOMEM;
        }
        free(v); free(r2);
    }
    if (pv && ctx && !plan_only) {
        if (pool.d_rec) (void)sk_dev_free(ctx, pool.d_rec);
        if (!pv->fold && (pool.prev || prev_failed)) (void)sk_item_slots(ctx, 0);
        free(pool.line_bases);
    }
    if (!plan_only) {
        /* What the reference has said by now.  All went well: every progress line, every skip message.  A file could not be
         * opened: it stopped right there (src/genome_compare.c:195-198) -- the progress file ends with that file's line
         * (lines of later files that other decode threads had taken meanwhile are cut off again) and no skip message of a
         * later line was printed.  (With several ranks only rank 0 writes; it knows the first failing line of ANY rank from
         * the agreement above.) */
        uint32_t upto = pool.nll;
        if (pool.rc == SK_E_OPEN) upto = (open_line != UINT32_MAX ? open_line : pool.item[pool.rc_index].line) + 1;
        if (pool.rc == SK_OK || pool.rc == SK_E_OPEN) {
            if (upto) progress_upto(&pool, upto - 1);
            if (pool.progress && upto < pool.ll_next && upto > 0 && fflush(pool.progress) == 0 &&
                ftruncate(fileno(pool.progress), (off_t)pool.ll[upto - 1].end) == 0)
                fseek(pool.progress, pool.ll[upto - 1].end, SEEK_SET);
        }
        if (err && rank == 0 && (pool.rc == SK_OK || pool.rc == SK_E_OPEN))
            for (i = 0; i < upto; i++)
                if (pool.ll[i].skipped) fprintf(err, "skipping %s (identical match)\n", pool.ll[i].text);
    }
    if (plan_only || by_other) {
        /* (said above or by the rank it happened to, or nothing to say) */
    } else if (pool.rc == SK_E_OPEN) {
        if (err) fprintf(err, "could not read file %s in GEN_calculate_kmer_count()\n", pool.item[pool.rc_index].path);
    } else if (pool.rc == SK_E_CACHE) {
        /* (the worker that found the damaged cache file has named it) */
    } else if (pool.rc == SK_E_SPLIT && guard && guard->armed) {
        /* (said nothing: the caller scans the list again, uncut) */
    } else if (pool.rc == SK_E_SPLIT) {
        if (err) fprintf(err, "kmer_scrub_count: %s could not be cut at record boundaries (bytes %llu-%llu): nothing is reported; "
                              "run again with SK_NO_SPLIT=1\n", pool.item[pool.rc_index].path,
                         (unsigned long long)pool.item[pool.rc_index].a, (unsigned long long)pool.item[pool.rc_index].b);
    } else if (pool.rc != SK_OK) {
        if (err) fprintf(err, "kmer_scrub_count: device error while scanning %s: %s (%s)\n", pool.item[pool.rc_index].path,
                         sk_strerror(pool.rc), sk_last_error(ctx));
    }
    if (pc_asked && ctx) {
        pc_count(ctx, pool.pc_served, pool.pc_written, pool.pc_stale, pool.pc_not);
        if (pool.timing && err && pc_dir)
            fprintf(err, "kmer_scrub_count timing: pack cache: %s: %llu items served, %llu written, %llu stale, %llu not cached; %.1f MB of cache files; "
                         "summed over the threads: checksums %.3f s, reading %.3f s, writing %.3f s\n", list_path, (unsigned long long)pool.pc_served,
                    (unsigned long long)pool.pc_written, (unsigned long long)pool.pc_stale, (unsigned long long)pool.pc_not, 1e-6 * (double)pool.pc_bytes,
                    pool.pc_t_sum, pool.pc_t_read, pool.pc_t_write);
    }
    free(pc_dir);
    for (i = 0; i < pool.nitem; i++) { free(pool.item[i].path); free(pool.item[i].cpath); }
    free(pool.item);
    for (i = 0; i < pool.nll; i++) free(pool.ll[i].text);
    free(pool.ll);
    pthread_mutex_destroy(&pool.submit_mu);
    pthread_mutex_destroy(&pool.queue_mu);
    if (bases && !(pool.rc == SK_E_SPLIT && guard && guard->armed)) *bases += pool.bases;
    return pool.rc;
}

static int scan_list_impl(sk_ctx *const *ctxs, uint32_t nctx, const char *list_path, const char *skip, uint32_t col, FILE *progress,
                          FILE *err, uint32_t rank, uint32_t world, uint64_t *bases, int plan_only, const plan_report *report, int no_split,
                          const prev_opts *pv)
{
    split_guard guard = {NULL, 0, -1, 0};
    uint32_t c;
    int rc = scan_list_once(ctxs, nctx, list_path, skip, col, progress, err, rank, world, bases, plan_only, report, no_split, &guard, pv);
    if (rc == SK_E_SPLIT && guard.armed) {               /* (armed on every rank of a coordinated run, or on none) */
        rc = SK_OK;
        for (c = 0; rc == SK_OK && c < guard.nsnap; c++)  /* every context's column back */
            if (guard.snap[c] && (rc = sk_counts_set(ctxs[c], col, guard.snap[c])) != SK_OK && err)
                fprintf(err, "kmer_scrub_count: could not put the counters back: %s (%s)\n", sk_strerror(rc), sk_last_error(ctxs[c]));
        if (rc == SK_OK && progress && guard.prog_at >= 0 && fflush(progress) == 0 && ftruncate(fileno(progress), (off_t)guard.prog_at) == 0)
            fseek(progress, guard.prog_at, SEEK_SET);
        if (getenv("SK_TIMING") && err && rc == SK_OK) fprintf(err, "kmer_scrub_count timing: a cut of %s did not hold; the list is scanned again uncut\n", list_path);
        /* the second scan opens with an agreement too: a rank whose restore failed says so there and everybody leaves */
        rc = scan_list_once(ctxs, nctx, list_path, skip, col, progress, err, rank, world, bases, plan_only, report, rc == SK_OK ? 1 : 2, NULL, pv);
    }
    for (c = 0; c < guard.nsnap; c++) free(guard.snap[c]);
    free(guard.snap);
    return rc;
}

int skh_scan_list(sk_ctx *ctx, const char *list_path, const char *skip, uint32_t col, FILE *progress,
                  FILE *err, uint32_t rank, uint32_t world, uint64_t *bases)
{
    return scan_list_impl(&ctx, 1, list_path, skip, col, progress, err, rank, world, bases, 0, NULL, 0, NULL);
}

int skh_scan_list_many(sk_ctx *const *ctx, uint32_t n, const char *list_path, const char *skip, uint32_t col, FILE *progress,
                       FILE *err, uint32_t rank, uint32_t world, uint64_t *bases)
{
    if (!ctx || n < 1) return SK_E_ARG;
    if (n > 1 && (!sk_scan_pinned_many || !sk_scan_pinned_packed_many)) return SK_E_STATE;
    return scan_list_impl(ctx, n, list_path, skip, col, progress, err, rank, world, bases, 0, NULL, 0, NULL);
}

int skh_scan_list_uncut(sk_ctx *ctx, const char *list_path, const char *skip, uint32_t col, FILE *progress,
                        FILE *err, uint32_t rank, uint32_t world, uint64_t *bases)
{
    return scan_list_impl(&ctx, 1, list_path, skip, col, progress, err, rank, world, bases, 0, NULL, 1, NULL);
}

int skh_scan_list_prevalence(sk_ctx *ctx, const char *list_path, const char *skip, uint32_t col, uint32_t prev_col, uint32_t min_count,
                             skh_prev_items *items_out, FILE *progress, FILE *err, uint32_t rank, uint32_t world, uint64_t *bases)
{
    prev_opts pv;
    if (!ctx || !list_path || !items_out || min_count < 1 || col == prev_col) return SK_E_ARG;
    if (!sk_item_slots || !sk_item_slot || !sk_item_fold || !sk_dev_alloc || !sk_dev_free || !sk_dev_upload || !sk_dev_download) return SK_E_STATE;
    items_out->item = NULL; items_out->n = 0;
    memset(&pv, 0, sizeof pv);
    pv.prev_col = prev_col; pv.min_count = min_count; pv.items = items_out;
    return scan_list_impl(&ctx, 1, list_path, skip, col, progress, err, rank, world, bases, 0, NULL, 1, &pv);
}

int skh_scan_list_many_prevalence(sk_ctx *const *ctx, uint32_t n, const char *list_path, uint32_t col, uint32_t nslots,
                                  skh_item_fold_fn fold, void *user, skh_prev_items *items_out, FILE *progress, FILE *err, uint64_t *bases)
{
    prev_opts pv;
    if (!ctx || n < 1 || !list_path || !items_out || !fold || nslots < 1) return SK_E_ARG;
    if (!sk_item_slot || (n > 1 && (!sk_scan_pinned_many || !sk_scan_pinned_packed_many))) return SK_E_STATE;
    items_out->item = NULL; items_out->n = 0;
    memset(&pv, 0, sizeof pv);
    pv.items = items_out; pv.fold = fold; pv.fold_user = user; pv.nslots = nslots;
    return scan_list_impl(ctx, n, list_path, NULL, col, progress, err, 0, 1, bases, 0, NULL, 1, &pv);
}

void skh_prev_items_free(skh_prev_items *items)
{
    uint32_t i;
    if (!items) return;
    for (i = 0; items->item && i < items->n; i++) free(items->item[i].path);
    free(items->item);
    items->item = NULL; items->n = 0;
}

int skh_list_plan_hash(const char *list_path, const char *skip, uint32_t world, uint64_t *hash)
{
    plan_report rp = {hash, NULL, 0, NULL};
    if (!list_path || !hash) return SK_E_ARG;
    return scan_list_impl(NULL, 0, list_path, skip, 0, NULL, NULL, 0, world ? world : 1, NULL, 1, &rp, 0, NULL);
}

int skh_list_plan_owners(const char *list_path, const char *skip, uint32_t world, uint32_t *owner, uint32_t cap, uint32_t *nlines)
{
    plan_report rp = {NULL, owner, cap, nlines};
    if (!list_path || !nlines || (cap && !owner)) return SK_E_ARG;
    return scan_list_impl(NULL, 0, list_path, skip, 0, NULL, NULL, 0, world ? world : 1, NULL, 1, &rp, 0, NULL);
}

/* =========================================================================================
 * output
 * ======================================================================================= */

static char *put_i32(char *p, int32_t v)             /* "%d" of an unsigned counter */
{
    char tmp[12];
    int n = 0;
    uint32_t u = v < 0 ? 0u - (uint32_t)v : (uint32_t)v;
    if (v < 0) *p++ = '-';
    do { tmp[n++] = (char)('0' + u % 10); u /= 10; } while (u);
    while (n) *p++ = tmp[--n];
    return p;
}

static int cmp_u64(const void *a, const void *b) { const uint64_t x = *(const uint64_t *)a, y = *(const uint64_t *)b; return x < y ? -1 : x > y; }

/* the table from any four columns of the counters (from[c]: the column printed as field c + 1), `extra` behind the header line */
static int print_table(sk_ctx *ctx, const skh_keyset *ks, FILE *out, int with_drug_column, const uint32_t from[4], const char *extra)
{
    const uint32_t ncols = with_drug_column ? 4 : 3, n = ks->nrows;
    uint32_t *cols[4] = {NULL, NULL, NULL, NULL};
    uint32_t c, r, w = 0, *worder;
    char *buf, *p;
    int rc = SK_OK;
    const size_t BUF = 1 << 20;
    if (sk_table_rows(ctx) != n) return SK_E_STATE;
    for (c = 0; c < ncols; c++) if (sk_table_cols(ctx) <= from[c]) return SK_E_STATE;
    for (c = 0; c < ncols && rc == SK_OK; c++) {
        cols[c] = (uint32_t *)malloc((size_t)(n ? n : 1) * sizeof(uint32_t));
        rc = sk_counts_fetch(ctx, from[c], cols[c]);
    }
    /* wide keys in ascending row order (an IUPAC-riddled strain has hundreds of thousands: sort, not insert) */
    worder = (uint32_t *)malloc((size_t)(ks->nwide ? ks->nwide : 1) * sizeof(uint32_t));
    {
        uint64_t *pair = (uint64_t *)malloc((size_t)(ks->nwide ? ks->nwide : 1) * sizeof(uint64_t));
        for (c = 0; c < ks->nwide; c++) pair[c] = ((uint64_t)ks->wide_rows[c] << 32) | c;
        qsort(pair, ks->nwide, sizeof *pair, cmp_u64);
        for (c = 0; c < ks->nwide; c++) worder[c] = (uint32_t)pair[c];
        free(pair);
    }
    if (rc == SK_OK) {
        buf = (char *)malloc(BUF + 256);
        p = buf;
        fputs("#kmer\treference_count\tpangenome_count\tmetagenome_count\tdrug_count\n", out);
        if (extra) fputs(extra, out);
        for (r = 0; r < n; r++) {
            if (ks->packed[r] != SK_KEY_NONE) { decode_key(ks->packed[r], p); p += SK_K; }
            else {
                const char *wk = ks->wide_keys + (size_t)worder[w++] * 32;
                size_t l = strlen(wk);
                memcpy(p, wk, l);
                p += l;
            }
            for (c = 0; c < ncols; c++) { *p++ = '\t'; p = put_i32(p, (int32_t)cols[c][r]); }
            *p++ = '\n';
            if ((size_t)(p - buf) >= BUF) { fwrite(buf, 1, (size_t)(p - buf), out); p = buf; }
        }
        fwrite(buf, 1, (size_t)(p - buf), out);
        free(buf);
    }
    for (c = 0; c < 4; c++) free(cols[c]);
    free(worder);
    return rc;
}

/* the count table's shape from any four columns, with comment lines behind the header (kmer_scrub_count -S writes each strain's
 * prevalence table with it) */
int skh_print_table_cols_(sk_ctx *ctx, const skh_keyset *ks, FILE *out, int with_drug_column, const uint32_t from[4], const char *extra)
{
    return print_table(ctx, ks, out, with_drug_column, from, extra);
}

int skh_print_counts(sk_ctx *ctx, const skh_keyset *ks, FILE *out, int with_drug_column)
{
    static const uint32_t from[4] = {0, 1, 2, 3};
    return print_table(ctx, ks, out, with_drug_column, from, NULL);
}

/* =========================================================================================
 * the program
 * ======================================================================================= */

static void usage(FILE *err)
{
    fputs("Usage: kmer_scrub_count -r <reference genome>  -A <file with multiple genome filenames> "
          "-B <file with multiple metagenome filenames> -C <(optional) file with multiple genome "
          "filenames of drug strains> -p [progress output file, optional]\n", err);
}

static int env_int(const char *a, const char *b, const char *c3, int dflt)
{
    const char *v = getenv(a);
    if (!v && b) v = getenv(b);
    if (!v && c3) v = getenv(c3);
    return v ? atoi(v) : dflt;
}

/* Multi-GPU use (new; one process per GPU, any launcher that sets the usual variables):
 *   SK_WORLD_SIZE | WORLD_SIZE | OMPI_COMM_WORLD_SIZE,  SK_RANK | RANK | OMPI_COMM_WORLD_RANK,
 *   SK_LOCAL_RANK | LOCAL_RANK | OMPI_COMM_WORLD_LOCAL_RANK (HIP device; SK_DEVICE overrides),
 *   SK_RCCL_ID_FILE (rendezvous file for the RCCL unique id; default /tmp/sk_rccl_id.<MASTER_PORT|uid>).
 * List items (files, byte ranges of big plain-text files) are dealt to the ranks by size -- the same plan on every rank,
 * compared before anyone scans (SK_E_PLAN) --, every rank's counters are summed with one RCCL all-reduce, rank 0 alone
 * writes stdout, the progress file and the skip/progress messages.  The sequence of collectives is the same on every rank
 * whatever fails where: set-up (in the rendezvous), table load (one sum), per list scan two agreements, one sum, the all-reduce. */
static int ksc_main(int argc, char **argv, FILE *out, FILE *err, int *pack_cache_word_out);

/* (--pack-cache DIR sets the process-wide default of the packed input cache: taken back when the call ends, however it ends) */
int skh_kmer_scrub_count_main(int argc, char **argv, FILE *out, FILE *err)
{
    int word = 0;
    const int status = ksc_main(argc, argv, out, err, &word);
    if (word) skh_pack_cache_set(NULL, NULL, NULL);
    return status;
}

static int ksc_main(int argc, char **argv, FILE *out, FILE *err, int *pack_cache_word_out)
{
    const char *A = NULL, *B = NULL, *C = NULL, *R = NULL, *P = NULL, *env;
    FILE *progress = NULL;
    skh_keyset ks;
    sk_ctx *ctx = NULL;
    int c, rc, status = 1, failed = 0;
    const int world = env_int("SK_WORLD_SIZE", "WORLD_SIZE", "OMPI_COMM_WORLD_SIZE", 1);
    const int rank = env_int("SK_RANK", "RANK", "OMPI_COMM_WORLD_RANK", 0);
    int device = env_int("SK_LOCAL_RANK", "LOCAL_RANK", "OMPI_COMM_WORLD_LOCAL_RANK", 0);
    const int use_comm = world > 1 || getenv("SK_FORCE_COMM") != NULL;
    uint32_t nfailed = 0;
    sk_ctxjob cj;
    int crc;
    double t0 = 0, t1 = 0, t2 = 0, t3 = 0, t4 = 0, t5 = 0;
    double scrub_fraction = -1.0;                    /* >= 0: print the scrub filter's result instead of the table */
    const char *scrub_list = NULL;                   /* --scrub f0,f1,...: the scrub sweep (scrub_fraction is f0) */
    skw_list scrub_sw;
    int scrub_independent = 0, j;
    const char *scrub_out = NULL;                    /* --scrub-out FILE: the filter's result goes there instead of stdout */
    int detect_argc = 0;                             /* --detect ...: strain_detect's arguments, run on the resident table */
    char **detect_argv = NULL;
    /* --prevalence[=FILE] [--prevalence-min-count m] [--prevalence-items=FILE] [--scrub-by prevalence] (extension; the rule is in
     * include/strainer_kmer.h at sk_item_fold): three more columns behind the table's own, a second table of the count table's shape */
    int prevalence = 0, scrub_by_prev = 0;
    const char *prev_file = NULL, *prev_items_file = NULL, *prev_min_text = NULL, *scrub_by = NULL;
    uint32_t prev_min = 1, prev_base = 4;
    skh_prev_items prev_items[3];
    char prev_path[4200] = "";

    /* Extension (not in the reference): "--scrub <min_fraction>" [--independent] runs step 2 of the
     * workflow (scripts/kmer_scrub_filter.py -s <table> -m <min_fraction> [-i]) on the counters while
     * they are still on the device and prints ITS output; the 38-bytes-per-k-mer table is never written.
     * The words are taken out of argv before getopt, which only knows the reference's letters. */
    /* "--detect <strain_detect arguments>" (extension; needs --scrub): after steps 1 and 2 the same process goes on into
     * step 3 on the SAME resident table (key set, row order, device table, filters and strain text built once; SURVEY
     * 8(f3)): -r is this run's, -a is the list --scrub just produced; everything behind --detect is strain_detect's
     * command line (-B/-b/-c/-t/-g/-o, --coverage-depth ...).  "--scrub-out FILE" keeps the informative list. */
    for (c = 1; c < argc; c++)
        if (!strcmp(argv[c], "--detect")) {
            detect_argv = argv + c;                  /* argv[0] of the second command line: ignored there */
            detect_argc = argc - c;
            argc = c;
            break;
        }
    for (c = 1, j = 1; c < argc; c++) {
        if (!strcmp(argv[c], "--independent")) { scrub_independent = 1; continue; }
        if (!strcmp(argv[c], "--scrub-out") && c + 1 < argc) { scrub_out = argv[++c]; continue; }
        if (!strncmp(argv[c], "--pack-cache", 12) && (argv[c][12] == 0 || argv[c][12] == '=')) {     /* the packed input cache's directory (SK_PACK_CACHE) */
            const char *m = getenv("SK_PACK_CACHE_MODE");
            const char *dir = argv[c][12] ? argv[c] + 13 : (c + 1 < argc ? argv[++c] : "");
            if (!dir[0]) { fprintf(err, "kmer_scrub_count: --pack-cache needs a directory\n"); return 1; }
            skh_pack_cache_set(NULL, dir, m && !strcmp(m, "ro") ? "ro" : "rw");
            *pack_cache_word_out = 1;
            continue;
        }
        if (!strncmp(argv[c], "--prevalence-min-count", 22) && (argv[c][22] == 0 || argv[c][22] == '=')) {
            prev_min_text = argv[c][22] ? argv[c] + 23 : (c + 1 < argc ? argv[++c] : "");
            continue;
        }
        if (!strncmp(argv[c], "--prevalence-items", 18) && (argv[c][18] == 0 || argv[c][18] == '=')) {
            prev_items_file = argv[c][18] ? argv[c] + 19 : (c + 1 < argc ? argv[++c] : "");
            continue;
        }
        if (!strncmp(argv[c], "--prevalence", 12) && (argv[c][12] == 0 || argv[c][12] == '=')) {
            prevalence = 1;
            if (argv[c][12]) prev_file = argv[c] + 13;
            continue;
        }
        if (!strncmp(argv[c], "--scrub-by", 10) && (argv[c][10] == 0 || argv[c][10] == '=')) {
            scrub_by = argv[c][10] ? argv[c] + 11 : (c + 1 < argc ? argv[++c] : "");
            continue;
        }
        if (!strncmp(argv[c], "--scrub", 7) && (argv[c][7] == 0 || argv[c][7] == '=')) {
            const char *v = argv[c][7] ? argv[c] + 8 : (c + 1 < argc ? argv[++c] : "");
            char *e;
            if (strchr(v, ',')) {                    /* a list: the scrub sweep (include/strainer_kmer.h has the rule) */
                char why[160];
                if (skw_parse_list(v, &scrub_sw, why, sizeof why)) { fprintf(err, "kmer_scrub_count: --scrub %s: %s\n", v, why); return 1; }
                scrub_list = v;
                scrub_fraction = scrub_sw.f[0];
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
    for (c = 1; c < detect_argc; c++)                 /* (before anything is read: the resident table has no column for it) */
        if (!strncmp(detect_argv[c], "--coverage-background", 21) && (detect_argv[c][21] == 0 || detect_argv[c][21] == '=')) {
            fprintf(err, "kmer_scrub_count: --coverage-background does not go behind --detect: the resident table is loaded without its count column; "
                         "run strain_detect on its own for it\n");
            return 1;
        }
    {   /* a list of fractions and --coverage-scrub-sweep behind --detect go together: step 3 reads the class file step 2 writes */
        int want_sw = 0;
        for (c = 1; c < detect_argc; c++)
            if (!strncmp(detect_argv[c], "--coverage-scrub-sweep", 22) && (detect_argv[c][22] == 0 || detect_argv[c][22] == '=')) want_sw = 1;
            else if (!strncmp(detect_argv[c], "--scrub-classes", 15) && (detect_argv[c][15] == 0 || detect_argv[c][15] == '=')) {
                fprintf(err, "kmer_scrub_count: behind --detect the class file is the one --scrub f0,f1,... writes (no --scrub-classes)\n");
                return 1;
            }
        if (scrub_list && !want_sw) {
            fprintf(err, "kmer_scrub_count: --scrub %s: a list of fractions goes with --detect ... --coverage-scrub-sweep\n", scrub_list);
            return 1;
        }
        if (want_sw && !scrub_list) {
            fprintf(err, "kmer_scrub_count: --coverage-scrub-sweep behind --detect goes with a list of fractions, --scrub f0,f1,...\n");
            return 1;
        }
        if (scrub_list && !skh_scrub_filter_resident_sweep) { fprintf(err, "kmer_scrub_count: this build has no scrub sweep\n"); return 1; }
    }

    memset(prev_items, 0, sizeof prev_items);
    {   /* the prevalence words, before anything is read */
        if (scrub_by && strcmp(scrub_by, "prevalence") && strcmp(scrub_by, "count")) {
            fprintf(err, "kmer_scrub_count: --scrub-by takes count or prevalence\n");
            return 1;
        }
        scrub_by_prev = scrub_by && !strcmp(scrub_by, "prevalence");
        if (scrub_by_prev && !prevalence) { fprintf(err, "kmer_scrub_count: --scrub-by prevalence needs --prevalence\n"); return 1; }
        if (scrub_by && scrub_fraction < 0.0) { fprintf(err, "kmer_scrub_count: --scrub-by needs --scrub <min_fraction>\n"); return 1; }
        if (scrub_by_prev && scrub_list) {
            fprintf(err, "kmer_scrub_count: --scrub-by prevalence does not go with a list of fractions (the scrub sweep ranks by count)\n");
            return 1;
        }
        if ((prev_min_text || prev_items_file) && !prevalence) {
            fprintf(err, "kmer_scrub_count: --prevalence-min-count and --prevalence-items need --prevalence\n");
            return 1;
        }
        if (prev_min_text) {
            char *e;
            const unsigned long long m = strtoull(prev_min_text, &e, 10);
            if (e == prev_min_text || *e || prev_min_text[0] == '-' || prev_min_text[0] == '+' || m < 1 || m > 0xFFFFFFFFull) {
                fprintf(err, "kmer_scrub_count: --prevalence-min-count needs an integer of at least 1\n");
                return 1;
            }
            prev_min = (uint32_t)m;
        }
        if (prevalence && ((prev_file && !prev_file[0]) || (prev_items_file && !prev_items_file[0]))) {
            fprintf(err, "kmer_scrub_count: --prevalence=FILE and --prevalence-items=FILE need a file name\n");
            return 1;
        }
        if (prevalence) {                             /* (-S with --prevalence is refused by the -S program: skh_kmer_scrub_count_multi_main) */
            if (!sk_item_slots || !sk_item_slot || !sk_item_fold || !sk_dev_alloc || !sk_dev_free || !sk_dev_upload || !sk_dev_download ||
                (scrub_by_prev && !skh_scrub_filter_resident_cols)) {
                fprintf(err, "kmer_scrub_count: this build has no prevalence\n");
                return 1;
            }
        }
    }

    optind = 1;
    while ((c = getopt(argc, argv, "A:B:C:r:p:Hhud")) != -1) {
        switch (c) {
        case 'A': A = optarg; break;
        case 'B': B = optarg; break;
        case 'C': C = optarg; break;
        case 'r': R = optarg; break;
        case 'p': P = optarg; break;
        case 'd': break;
        default:  usage(err); break;                 /* -h/-u/-H/unknown: print and carry on */
        }
    }
    if (!R || !A || !B) { usage(err); return 1; }
    if (detect_argv && (scrub_fraction < 0.0 || world > 1)) {
        fprintf(err, "kmer_scrub_count: --detect needs --scrub <min_fraction> and a single process\n");
        return 1;
    }
    if (world < 1 || rank < 0 || rank >= world) { fprintf(err, "kmer_scrub_count: bad rank %d of %d\n", rank, world); return 1; }
    if (prevalence) {                                 /* the prevalence table's name: FILE, else <progress file>.prevalence.tsv, else kmer_scrub_count.prevalence.tsv */
        if (prev_file ? strlen(prev_file) + 1 > sizeof prev_path : (P ? strlen(P) : 16) + 16 > sizeof prev_path) {
            fprintf(err, "kmer_scrub_count: the prevalence file's path is too long\n");
            return 1;
        }
        if (prev_file) snprintf(prev_path, sizeof prev_path, "%s", prev_file);
        else snprintf(prev_path, sizeof prev_path, "%s.prevalence.tsv", P ? P : "kmer_scrub_count");
        prev_base = detect_argv ? 6 : 4;
    }
    if (P && rank == 0) {
        progress = fopen(P, "w");
        if (!progress) { fprintf(err, "could not open progress file %s\n", P); return 1; }
        fputs("adding kmer counts for:\n", progress);
    }
    if ((env = getenv("SK_DEVICE")) != NULL) device = atoi(env);

    memset(&ks, 0, sizeof ks);
    t0 = now_s();
    sk_ctxjob_start(&cj, device);                      /* the HIP runtime comes up while the key set is built */
    rc = skh_keyset_from_file(&ks, R, SK_REF_TABLE_SLOTS, 1, 1);
    t1 = now_s();
    crc = sk_ctxjob_join(&cj, &ctx);
    t2 = now_s();
    {   /* set-up problems are reported here; with several ranks the others are told before anyone enters the collective */
        int setup_failed = 0;
        if (rc == SK_E_OPEN) { fprintf(err, "could not read file %s GEN_hash_sequences_set_count_vec()\n", R); setup_failed = 1; }
        else if (rc != SK_OK) { fprintf(err, "kmer_scrub_count: %s\n", sk_strerror(rc)); setup_failed = 1; }
        else if (ks.short_records && rank == 0)
            fprintf(err, "kmer_scrub_count: skipped %llu reference record(s) shorter than %d bases "
                         "(the original program crashes on these)\n", (unsigned long long)ks.short_records, SK_K - 1);
        if (crc != SK_OK) {
            if (!setup_failed) fprintf(err, "kmer_scrub_count: cannot use HIP device %d: %s\n", device, sk_strerror(crc));
            setup_failed = 1; ctx = NULL;
        }
        if (use_comm) {
            char path[256];
            int timeout_s = 120;
            if ((env = getenv("SK_RCCL_ID_FILE")) != NULL) snprintf(path, sizeof path, "%s", env);
            else if ((env = getenv("MASTER_PORT")) != NULL) snprintf(path, sizeof path, "/tmp/sk_rccl_id.%s", env);
            else snprintf(path, sizeof path, "/tmp/sk_rccl_id.%d", (int)getuid());
            if ((env = getenv("SK_RENDEZVOUS_TIMEOUT")) != NULL && atoi(env) > 0) timeout_s = atoi(env);
            {   /* RCCL prints its version banner on stdout, which here is the TSV: park fd 1 on stderr meanwhile */
                int saved;
                fflush(stdout);
                saved = dup(1);
                dup2(2, 1);
                rc = sk_comm_init_ex(ctx, rank, world, path, timeout_s, setup_failed);
                fflush(stdout);
                dup2(saved, 1);
                close(saved);
            }
            if (rc != SK_OK && !setup_failed)
                fprintf(err, "kmer_scrub_count: RCCL rendezvous failed: %s (%s)\n", sk_strerror(rc), ctx ? sk_last_error(ctx) : "no context");
            if (rc != SK_OK) goto done;
        } else if (setup_failed) goto done;
    }
    rc = skh_keyset_load(ctx, &ks, (detect_argv ? 6u : 4u) + (prevalence ? 3u : 0u));        /* (strain_detect's table has six columns; the prevalence columns lie behind) */
    t3 = now_s();
    if (rc != SK_OK) { fprintf(err, "kmer_scrub_count: table load failed: %s (%s)\n", sk_strerror(rc), sk_last_error(ctx)); failed = 1; }
    if (rc == SK_OK && world > 1) rc = sk_counts_zero(ctx, 0);      /* column 0 must not be summed world times: keep it on rank 0 */
    if (rc == SK_OK && world > 1 && rank == 0) rc = sk_counts_set(ctx, 0, ks.first_count);
    if (rc != SK_OK && !failed) {                                   /* (a wrong column 0 must not reach the all-reduce) */
        fprintf(err, "kmer_scrub_count: could not set up the reference_count column: %s (%s)\n", sk_strerror(rc), sk_last_error(ctx));
        failed = 1;
    }

    if (use_comm) {
        /* a rank whose table did not load must not leave the others alone in the lists' agreements: from here to the big
         * all-reduce every rank issues the same collectives (skh_scan_list returns the same status on all of them) */
        rc = sk_comm_sum_u32(ctx, (uint32_t)failed, &nfailed);
        if (rc != SK_OK) { fprintf(err, "kmer_scrub_count: %s (%s)\n", sk_strerror(rc), sk_last_error(ctx)); goto done; }
        if (nfailed) {
            if (!failed) fprintf(err, "kmer_scrub_count: another rank could not load the table; nothing is reported\n");
            goto done;
        }
    }
    if (prevalence) {
        if (!failed && skh_scan_list_prevalence(ctx, A, NULL, 1, prev_base, prev_min, &prev_items[0], progress, err, (uint32_t)rank, (uint32_t)world, NULL) != SK_OK) failed = 1;
        if (!failed && skh_scan_list_prevalence(ctx, B, NULL, 2, prev_base + 1, prev_min, &prev_items[1], progress, err, (uint32_t)rank, (uint32_t)world, NULL) != SK_OK) failed = 1;
        if (!failed && C && skh_scan_list_prevalence(ctx, C, R, 3, prev_base + 2, prev_min, &prev_items[2], progress, err, (uint32_t)rank, (uint32_t)world, NULL) != SK_OK) failed = 1;
    } else {
        if (!failed && skh_scan_list(ctx, A, NULL, 1, progress, err, (uint32_t)rank, (uint32_t)world, NULL) != SK_OK) failed = 1;
        if (!failed && skh_scan_list(ctx, B, NULL, 2, progress, err, (uint32_t)rank, (uint32_t)world, NULL) != SK_OK) failed = 1;
        if (!failed && C && skh_scan_list(ctx, C, R, 3, progress, err, (uint32_t)rank, (uint32_t)world, NULL) != SK_OK) failed = 1;
    }
    if (use_comm) {
        /* agree once more (the lists' own agreements have made `failed` the same everywhere: a belt to those braces) */
        rc = sk_comm_sum_u32(ctx, (uint32_t)failed, &nfailed);
        if (rc != SK_OK) { fprintf(err, "kmer_scrub_count: %s (%s)\n", sk_strerror(rc), sk_last_error(ctx)); goto done; }
        if (nfailed) goto done;
        rc = sk_counts_allreduce(ctx, NULL);
        if (rc != SK_OK) { fprintf(err, "kmer_scrub_count: all-reduce failed: %s (%s)\n", sk_strerror(rc), sk_last_error(ctx)); goto done; }
    } else if (failed) goto done;
    if (prevalence && rank == 0) {
        /* the prevalence table: the count table's shape, the items of each list that hold the k-mer in place of its counts; and the
         * items' own records */
        const uint32_t from[4] = {0, prev_base, prev_base + 1, prev_base + 2};
        char extra[160];
        FILE *pf = fopen(prev_path, "w");
        if (!pf) { fprintf(err, "kmer_scrub_count: cannot write %s\n", prev_path); goto done; }
        snprintf(extra, sizeof extra, "#items\t%u\t%u\t%u\n#min_count\t%u\n", prev_items[0].n, prev_items[1].n, prev_items[2].n, prev_min);
        rc = print_table(ctx, &ks, pf, C != NULL, from, extra);
        if (fclose(pf) != 0 && rc == SK_OK) rc = SK_E_OPEN;
        if (rc != SK_OK) { fprintf(err, "kmer_scrub_count: %s: %s (%s)\n", prev_path, sk_strerror(rc), sk_last_error(ctx)); goto done; }
        if (prev_items_file) {
            uint32_t l, k;
            if (!(pf = fopen(prev_items_file, "w"))) { fprintf(err, "kmer_scrub_count: cannot write %s\n", prev_items_file); goto done; }
            fputs("#list\tline\tfile\tbases\tkmers_present\tkmer_hits\n", pf);
            for (l = 0; l < 3; l++)
                for (k = 0; k < prev_items[l].n; k++) {
                    const skh_prev_item *t = &prev_items[l].item[k];
                    fprintf(pf, "%c\t%u\t%s\t%llu\t%llu\t%llu\n", "ABC"[l], t->line, t->path, (unsigned long long)t->bases,
                            (unsigned long long)t->kmers_present, (unsigned long long)t->kmer_hits);
                }
            if (fclose(pf) != 0) { fprintf(err, "kmer_scrub_count: cannot write %s\n", prev_items_file); goto done; }
        }
    }
    t4 = now_s();
    if (rank == 0 && scrub_fraction >= 0.0) {
        FILE *so = out;
        char tmp_path[64] = "", cls_path[4200] = "";
        const char *list_path = scrub_out;
        if (detect_argv && !scrub_out) {              /* step 3 reads the list from a file: a temporary one, copied to stdout */
            int fd;
            snprintf(tmp_path, sizeof tmp_path, "/tmp/sk_scrubbed.XXXXXX");
            fd = mkstemp(tmp_path);
            if (fd < 0) { fprintf(err, "kmer_scrub_count: cannot create a temporary file for the informative k-mers\n"); goto done; }
            close(fd);
            list_path = tmp_path;
        }
        if (list_path && !(so = fopen(list_path, "w"))) { fprintf(err, "kmer_scrub_count: cannot write %s\n", list_path); goto done; }
        if (scrub_list) {                             /* (a list goes with --detect: list_path is a file) */
            if (strlen(list_path) + 9 > sizeof cls_path) { fprintf(err, "kmer_scrub_count: %s: the path is too long\n", list_path); fclose(so); goto done; }
            snprintf(cls_path, sizeof cls_path, "%s.classes", list_path);
            status = skh_scrub_filter_resident_sweep(ctx, &ks, C != NULL, scrub_list, scrub_independent, cls_path, so, err);
        } else if (scrub_by_prev) {
            const uint32_t pcols[3] = {prev_base, prev_base + 1, prev_base + 2};
            status = skh_scrub_filter_resident_cols(ctx, &ks, C != NULL, pcols, scrub_fraction, scrub_independent, so, err);
        } else
            status = skh_scrub_filter_resident(ctx, &ks, C != NULL, scrub_fraction, scrub_independent, so, err);
        if (so != out) fclose(so);
        if (tmp_path[0] && status == 0) {             /* no --scrub-out: the list still goes to stdout, as --scrub alone does */
            FILE *f = fopen(tmp_path, "r");
            char blk[65536];
            size_t got;
            while (f && (got = fread(blk, 1, sizeof blk, f)) > 0) fwrite(blk, 1, got, out);
            if (f) fclose(f);
            fflush(out);
        }
        t5 = now_s();
        if (status == 0 && detect_argv) {
            sk_ctx *c2 = ctx;
            ctx = NULL;                               /* ctx and ks now belong to strain_detect, which releases them */
            skh_pack_cache_set(c2, NULL, NULL);       /* (step 1's counters end here; strain_detect forgets the context when it lets it go) */
            if (skh_resident_genomes_) skh_resident_genomes_((const char *const *)&R, 1);      /* (--coverage-regions reads the records' names from it) */
            status = skh_strain_detect_resident(c2, &ks, list_path, detect_argc, detect_argv, out, err);
        }
        if (tmp_path[0]) unlink(tmp_path);
        if (tmp_path[0] && cls_path[0]) unlink(cls_path);
        goto done;
    }
    if (rank == 0) {
        rc = skh_print_counts(ctx, &ks, out, C != NULL);
        if (rc != SK_OK) { fprintf(err, "kmer_scrub_count: %s (%s)\n", sk_strerror(rc), sk_last_error(ctx)); goto done; }
    }
    t5 = now_s();
    status = 0;
done:
    if (getenv("SK_TIMING") && t5 > 0)
        fprintf(err, "kmer_scrub_count timing: key set %.2f s (+%.2f s more for the HIP context), table load %.2f s, scans %.2f s, "
                     "%s %.2f s\n", t1 - t0, t2 - t1, t3 - t2, t4 - t3, scrub_fraction >= 0.0 ? "filter + print" : "print", t5 - t4);
    if (ctx) skh_pack_cache_set(ctx, NULL, NULL);    /* (the context's address may be another context's later) */
    if (ctx && sk_pack_release) sk_pack_release(ctx);
    if (ctx) sk_ctx_destroy(ctx);
    skh_keyset_free(&ks);
    if (progress) fclose(progress);
    for (c = 0; c < 3; c++) skh_prev_items_free(&prev_items[c]);
    return status;
}
