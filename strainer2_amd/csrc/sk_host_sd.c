/* sk_host_sd.c -- host layer of the strain_detect program (reference src/strain_detect.c).
 *
 * What runs where:
 *   device  every k-mer lookup: the per-read tallies (all hits / informative hits) and the log of
 *           informative hits come from sk_tally_batch (sk_scan_grid in TALLY mode); the informative
 *           k-mer list (-a) is itself looked up as a batch of 31-byte records; the -g background
 *           counts use the ordinary counting scan.
 *   host    file grammar, the reference's sequential read-pair bookkeeping (src/strain_detect.c:443-626,
 *           including its carry-over of tallies and of the PE1 copy across reads shorter than k), the
 *           background threshold arithmetic (:160-240), gz output, messages, exit codes.
 *
 * Known, documented divergences: reads of 10,000+ bases are handled (the reference
 * overflows fixed buffers); a blank line in the -B list is reported, not a crash; after a malformed
 * FASTQ record in a PE2 file the file is treated as ended.
 */
#define _GNU_SOURCE
#include <assert.h>
#include <dirent.h>
#include <errno.h>
#include <fcntl.h>
#include <pthread.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <sys/resource.h>
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
#include "sk_internal.h"
#include "sk_ctxjob.h"
#include "sk_gzpipe.h"
#include "sk_cpus.h"
#include "sk_gzout.h"
#include "sk_pcache.h"


enum { SD_TYPE = 0, SD_BACKGROUND = 5, SD_INFORMATIVE = 2, SD_PLAIN = 1, SD_NCOLS = 6 };
enum { SD_SE = 0, SD_PE = 1, SD_PEI = 2, SD_UNKNOWN = -1 };
#define SD_BATCH_BYTES (32u << 20)
#define SD_PARSERS_MAX 16                 /* parser threads on one file, at most (SK_PARSE_THREADS) */
#define SD_PARSERS_MAPPED 12              /* ... on a mapped plain file with the whole thread budget behind it, by default (8 until round 4: the main thread was what the pass waited for) */
/* ONE process, ONE decode pipeline, several devices (strain_detect -S with SK_DEVICES=n; BASELINE configs[4]: 256 strains on the 8
 * GPUs of a node).  The strains are dealt to the devices in groups of SK_UNION_MAX (one union table per group: group g lives on
 * logical device g mod n); a decoded chunk of the metagenome is uploaded ONCE PER DEVICE from the same page-locked buffer (every
 * GPU has its own PCIe link: the copies run side by side), every device scans it against its own strains, and the results come
 * back to the one host that replays each strain's bookkeeping.  Against `torchrun`-style one-process-per-GPU with the strains
 * dealt to ranks (which still works: RANK/WORLD_SIZE) the metagenome is inflated and parsed once instead of once per GPU.
 * New relative to the reference, which is one process, one strain (src/strain_detect.c:263-384).
 * phys[d] = the HIP device behind logical device d: SK_DEVICES=n -> SK_DEVICE + 0..n-1; SK_DEVICES=0,0,0 -> as listed (several
 * logical devices on one card: how the path is tested on a one-GPU box). */
#define SD_MAX_DEV 8
static struct { int n; int phys[SD_MAX_DEV]; sk_ctx *ctx[SD_MAX_DEV]; } sd_dev = { 1, {0}, {NULL} };
static uint32_t sd_group = SK_UNION_MAX;                  /* strains per union table (SK_SD_GROUP: smaller groups, for tests of the dealing) */
static int sd_dev_of_strain(uint32_t s) { return (int)((s / sd_group) % (uint32_t)sd_dev.n); }
/* SK_SD_CHUNK_BYTES: smaller chunks (tests: chunk boundaries between mates, carried state across chunks) or bigger ones (up to 1 GiB) */
/* strain_detect never shows the order of the table's rows (hits are printed read by read with the k-mer's text; the
 * trailer counts rows), so the 0.2 s replay of BIO_hash's slot order (sk_host.c) is left out: rows in strain order.
 * SK_SD_REF_ROW_ORDER=1 replays it all the same (tests compare the two). */
#define SD_ROW_ORDER (getenv("SK_SD_REF_ROW_ORDER") ? SK_REF_TABLE_SLOTS : SK_ROWS_IN_STRAIN_ORDER)

static size_t sd_chunk_bytes(void)
{
    const char *e = getenv("SK_SD_CHUNK_BYTES");
    const long v = e ? atol(e) : 0;
    return v >= 64 && v <= (1l << 30) ? (size_t)v : SD_BATCH_BYTES;
}

/* ---------------------------------------------------------------------------------------------
 * program state: one per strain (table on the device, type column, output, replay state)
 * ------------------------------------------------------------------------------------------- */
typedef struct {
    sk_ctx     *ctx;
    int         ctx_rc;        /* status of a context opened in the background (0 = fine or not tried) */
    int         table_on_device;/* the key set was built on the device (skh_keyset_build_on_device): the table is loaded already */
    skh_keyset  ks;
    uint32_t   *type;          /* host copy of the type column */
    FILE       *out, *err;
    /* quantification */
    skzo_file  *zo;            /* -o: gzip members compressed on the output pool (sk_gzout.h) */
    unsigned    genome_inf;    /* informative rows after -a / -g */
    int         h1, i1, h2, i2;            /* tallies carried from read to read (src/strain_detect.c:444-454,497-500) */
    uint32_t   *copy_rows; uint32_t copy_n, copy_cap;   /* informative rows of the PE1 read last copied (:451) */
    skc_acc    *cov; char *cov_path, *o_path;           /* --coverage-depth: step 4 of the workflow, fed at emission */
    sk_hit     *hitbuf; uint64_t hitcap;   /* landing area of the hit log */
    uint32_t   *tallybuf; uint32_t tallycap;
    int         job_rc;                    /* result of this strain's part of a pool job */
    uint32_t   *co_rows; uint64_t co_n, co_cap;   /* --coverage-only: rows of host-replayed passing hits on their way to the device's counters */
    uint32_t   *co_tot;                        /* --coverage-thresholds: beside every such row its pair's h1 + h2 (the rows then pass min(--min-kmer-hits, t[0])) */
    char *th_path;                             /* --coverage-thresholds: the table's path */
    /* --coverage-rarefaction: the table's path and its text so far; beside every row on its way to the device its pair's ordinal; the
     * pair the replay is at; and, where the lines are counted on the host, every row's highest class and the lines per class of the
     * target being read */
    char *ra_path, *ra_buf; size_t ra_len; FILE *ra_f;
    uint64_t *co_pair, rar_pair;
    uint8_t *rar_best; uint64_t rar_lines[SK_COVACC_RAREFACTION_MAX + 1];
    char *su_path;                             /* --coverage-support: the table's path */
    /* --coverage-scrub-sweep: the table's path, the strain's class file, its k-mers' rows and classes (the device's sparse list), and
     * every row's class (the host fold's) */
    char *sw_path; skc_classes sw_c; uint32_t *sw_rows; uint8_t *row_class;
    /* --coverage-regions: the strain's region table, every row's region (rg.n = unplaced), informative rows per region, the table's path */
    skh_regions rg; uint32_t *row_region; uint64_t *reg_inf; char *rg_path;
    char *sp_path;                             /* --coverage-spectrum: the table's path */
    char *rc_path, *rp_path;                   /* --coverage-recurrence, --recurrence-pairs: the tables' paths */
    char *bg_path, *bgs_path; skb_table *bg;   /* --coverage-background, --background-spectrum: the tables' paths, the targets' blocks */
} sd_prog;

/* ---------------------------------------------------------------------------------------------
 * one metagenome file as a stream of chunks: a decode thread parses ahead, the main thread tallies
 * each chunk against every strain and walks its records
 * ------------------------------------------------------------------------------------------- */
typedef struct sd_chunk {
    uint8_t  *buf; uint64_t blen, bcap;      /* record stream: the records of length >= k, '\n' after each */
    int       pinned;                        /* buf belongs to the pool of page-locked buffers */
    int       packed;                        /* buf holds the stream in sk_pack_stream's form (blen, pstart: of the byte stream it was packed from) */
    uint32_t *pstart, *prec; uint32_t np, pcap;   /* those records: offset in buf, index in len[] */
    uint64_t *len; uint32_t nrec, rcap;      /* every record, length as the reference sees it */
    int       last, end_kind; size_t end_len;/* last chunk of the file: how the parser ended */
    uint64_t  rec0, co_base;                 /* the file's records in front of the chunk; a folded chunk: the target's ordinal of its run's pair 0 (--coverage-rarefaction) */
    /* per strain, filled by sd_tally_chunk: the records that hit the strain at all, ascending -- their tallies and their
     * informative rows (CSR).  Nothing here is proportional to records x strains: against a metagenome nearly every
     * (read, strain) pair is a blank */
    struct sd_sp *sp;
    uint32_t  nstrains;
    /* what the scan of this chunk brought back, strain by strain (round 4: owned by the chunk, so that the per-strain work on it
     * -- sort, spread, replay -- runs on the lanes while the main thread is on to the next chunk): strain s's hit records are
     * res_recs[res_off[s] .. res_off[s + 1]), its log entries res_hits[res_hoff[s] .. res_hoff[s + 1]) */
    sk_tally_rec *res_recs; sk_hit *res_hits; uint64_t *res_off, *res_hoff;
    int       refs;                          /* holders: the stream (queue, current chunk), every lane job that names it */
    /* a piece of plain text for the device's parser (sd_text_read): buf holds text[toff .. toff + tlen) of the file and tla bytes of
     * look-ahead; the arrays above are filled from the device's record starts once the piece is accepted (sd_text_resolve) */
    int       text;                          /* SD_TEXT_*: 0 = a chunk the host parsed */
    int       t_eof, tla;                    /* the file's last piece; bytes of look-ahead behind the piece (0 or 1) */
    uint64_t  toff, tlen;
    uint64_t  t_reads, t_eval;               /* accepted: records of k bases or more, and their windows */
    int       tc_handed;                     /* the target cache's writer has been given this chunk */
    int       cache_err;                     /* the serving thread's marker: its cache file failed a check here (SKPC_*) */
    /* --coverage-only: SD_CO_FOLDED the chunk's pairs were counted on the device and res_* holds only its first and last records'
     * results; SD_CO_HELD (a PE1 chunk) the accumulators hold its results until the PE2 chunk shows whether the two fold together */
    int       co; uint32_t co_a0;            /* (co_a0: PEI, the chunk's first record is the mate of the last chunk's last: 1) */
} sd_chunk;
enum { SD_CO_NONE = 0, SD_CO_FOLDED = 1, SD_CO_HELD = 2 };
enum { SD_TEXT_PENDING = 1, SD_TEXT_ACCEPTED = 2, SD_TEXT_DECLINED = 3 };   /* (DECLINED before it went up: the reader found no piece to send) */
typedef struct sd_sp { uint32_t n; uint32_t *rec, *all, *inf, *hbeg /* n + 1 */, *rows; } sd_sp;

typedef struct {
    const char *path;
    int gz_threads;                 /* threads inflating this file (sk_gzpar.h when > 1) */
    gzFile      g;
    pthread_t   th; int started;
    pthread_mutex_t mu; pthread_cond_t cv;
    sd_chunk   *q[3]; int qn, cancel;        /* decoded chunks waiting for the main thread */
    sd_chunk   *cur;                         /* producer: chunk under construction (serial decode) */
    size_t      chunk_bytes;
    /* several parser threads on ONE file (sd_decode_thread): the text is cut into segments at guessed record starts,
     * every segment is parsed on its own and CHECKED to end between two records, chunks are queued in segment order */
    int         par;                         /* parser threads (0/1 = the decode thread parses itself) */
    pthread_mutex_t pmu; pthread_cond_t pcv;
    struct sd_seg *segq[20]; int segn, seg_done;   /* segments waiting for a parser thread; no more will come */
    uint64_t    next_push;                   /* sequence number of the segment whose chunks go to q next */
    size_t      carry_last_len;              /* length of the last record handed out so far (for an END_STALE ending) */
    int         split_failed;                /* a segment did not end between two records */
    int         cancel_segments;             /* the file is over for the reader (truncated record): later segments are dropped */
    int         in_mode;                     /* SKI_*: how the parser threads get at the bytes of a mapped plain file's segments */
    /* plain text parsed on the device (sd_text_read): the reader sends pieces of text until the main thread's verdict */
    int         text_mode;                   /* the option is on and the entry points are there */
    int         text_verdict;                /* 0 none yet, SD_VERDICT_DONE the last piece was accepted, SD_VERDICT_HOST the piece at text_off declined */
    uint64_t    text_off;
    /* consumer */
    sd_chunk   *c; uint32_t ci;
    int         eof, end_kind; size_t end_len;
    /* two device batches in turn: while the chunk in one is scanned, the next chunk of the queue is uploaded into the other;
     * with several devices (sd_dev) every device has its own pair -- one decoded chunk goes up to all of them */
    sk_batch   *bat[2][SD_MAX_DEV]; int bcur;
    sd_chunk   *pre;                         /* the queued chunk whose bytes are already in bat[bcur ^ 1] */
    sd_chunk   *ahead;                       /* ... and whose scan has been launched as well (solo streams: see sd_launch_ahead) */
    uint32_t    co_next;                     /* --coverage-only, PEI: the next chunk's co_a0 */
    uint64_t    nrec_seen;                   /* records of the chunks taken so far */
    int         solo;                        /* the only stream that uses the tables now (SE, PEI): its next chunk may be scanned while this one is replayed */
    /* the target cache (sd_tc): a file that is served has a serving thread in the decode thread's place; one that is filled has a writer */
    int         serving, cache_failed;
    skpc_reader tcr;
    char       *tc_path;
    struct sd_tcw *tcw;
} sd_stream;

/* Page-locked chunk buffers, recycled.  The upload of a chunk from ordinary memory goes through the runtime's
 * staging path, which collapses (measured: 17 -> 1.7 GB/s) as soon as other threads of the process fault pages
 * in at a high rate -- which is what the decode threads do when one .gz file is inflated by eight of them. */
#define SD_PIN_MAX 32                    /* (1 GiB at the default chunk size: every parser thread holds one, the queue three, the device pair two) */
static struct {
    pthread_mutex_t mu;
    sk_ctx *ctx; size_t bytes;
    void *idle[SD_PIN_MAX]; int nidle, total;
} sd_pin = { PTHREAD_MUTEX_INITIALIZER, NULL, 0, {NULL}, 0, 0 };

static unsigned long n_unpinned_chunks;     /* chunks whose text had to live in ordinary memory (their upload goes through the runtime's staging path) */
static void *sd_pin_get(void)
{
    void *q = NULL;
    pthread_mutex_lock(&sd_pin.mu);
    if (sd_pin.nidle) q = sd_pin.idle[--sd_pin.nidle];
    else if (sd_pin.ctx && sd_pin.total < SD_PIN_MAX && sk_pinned_alloc(sd_pin.ctx, &q, sd_pin.bytes) == SK_OK) sd_pin.total++;
    else q = NULL;
    pthread_mutex_unlock(&sd_pin.mu);
    return q;
}
static void sd_pin_put(void *q)
{
    pthread_mutex_lock(&sd_pin.mu);
    sd_pin.idle[sd_pin.nidle++] = q;                     /* (at most `total` <= SD_PIN_MAX are ever out) */
    pthread_mutex_unlock(&sd_pin.mu);
}
static void sd_pin_open(sk_ctx *ctx, size_t bytes) { sd_pin.ctx = ctx; sd_pin.bytes = bytes; }
static void sd_pin_close(void)
{
    while (sd_pin.nidle) { sk_pinned_free(sd_pin.ctx, sd_pin.idle[--sd_pin.nidle]); sd_pin.total--; }
    sd_pin.ctx = NULL;
}

static void sd_unmap_later(void *p, size_t n);
static double now_s(void);
static double t_pw_seg, t_pw_parse, t_pw_turn, t_pw_push;   /* SK_SD_TIMING: the parser threads' time, summed over them */
static double cpu_parsers, cpu_readers, cpu_lanes;          /* SK_SD_TIMING: CPU time (user + system) of those threads, summed when they end */
static double thread_cpu_s(void)
{
    struct rusage ru;
    if (getrusage(RUSAGE_THREAD, &ru) != 0) return 0.0;
    return (double)ru.ru_utime.tv_sec + 1e-6 * (double)ru.ru_utime.tv_usec + (double)ru.ru_stime.tv_sec + 1e-6 * (double)ru.ru_stime.tv_usec;
}
static pthread_mutex_t t_pw_mu = PTHREAD_MUTEX_INITIALIZER;

static sd_chunk *chunk_new(void)
{
    sd_chunk *c = (sd_chunk *)calloc(1, sizeof *c);
    if (c) c->refs = 1;
    return c;
}
static void chunk_ref(sd_chunk *c) { if (c) __atomic_add_fetch(&c->refs, 1, __ATOMIC_RELAXED); }

/* drop one holder's claim; the last one frees */
static void chunk_free(sd_chunk *c)
{
    uint32_t s;
    if (!c) return;
    if (__atomic_sub_fetch(&c->refs, 1, __ATOMIC_ACQ_REL) > 0) return;
    for (s = 0; c->sp && s < c->nstrains; s++) { free(c->sp[s].rec); free(c->sp[s].rows); }   /* (rec, all, inf, hbeg: one block) */
    free(c->sp);
    free(c->res_recs); free(c->res_hits); free(c->res_off);                                    /* (res_off, res_hoff: one block) */
    if (c->pinned) sd_pin_put(c->buf); else free(c->buf);
    free(c->pstart); free(c->prec); free(c->len);
    free(c);
}

static void stream_push(sd_stream *st, sd_chunk *c)
{
    pthread_mutex_lock(&st->mu);
    while (st->qn == 3 && !st->cancel && !(c->text && st->text_verdict)) pthread_cond_wait(&st->cv, &st->mu);
    if (st->cancel || (c->text && st->text_verdict)) { pthread_mutex_unlock(&st->mu); chunk_free(c); return; }   /* (text read ahead beyond a declined piece) */
    st->q[st->qn++] = c;
    pthread_cond_broadcast(&st->cv);
    pthread_mutex_unlock(&st->mu);
}

/* chunk builder of one parser: where finished chunks go depends on who parses */
typedef struct sd_seg { unsigned char *buf; size_t n; uint64_t seq; int is_last, borrowed; int fd; uint64_t off; } sd_seg;   /* borrowed: buf points into the mapped file */
typedef struct {
    sd_stream *st;
    sd_chunk  *cur;                          /* chunk under construction */
    sd_chunk **done; int ndone, dcap;        /* parallel parse: finished chunks of this segment, pushed later in order */
    int        direct;                       /* serial decode: finished chunks go straight to the stream's queue */
} sd_builder;

/* SK_SD_PACK=1: the finished chunk packed by the thread that built it -- 6 bytes per 16 bases go up instead of 16 (sk_pack.h; the scan's
 * first phase then only copies).  Out of one pool buffer into another, the first given back at once; a chunk with a byte for the
 * byte-string kernel, or one outside the pool, stays as it is.  OFF by default: the pass is bound by these threads' CPU time as much
 * as by the link, and the packing is theirs to pay. */
static int sd_pack_on(void) { const char *e = getenv("SK_SD_PACK"); return e && e[0] == '1'; }

static void chunk_pack(sd_chunk *c)
{
    void *pk;
    int odd = 0;
    if (!c || !c->pinned || !c->np || c->packed || c->blen > sd_chunk_bytes() || !sd_pack_on()) return;
    if ((pk = sd_pin_get()) == NULL) return;
    if (sk_pack_stream(c->buf, c->blen, pk, &odd) != SK_OK || odd) { sd_pin_put(pk); return; }
    sd_pin_put(c->buf);
    c->buf = (uint8_t *)pk;
    c->packed = 1;
}

static void builder_finish_chunk(sd_builder *b)
{
    chunk_pack(b->cur);
    if (b->direct) stream_push(b->st, b->cur);
    else {
        if (b->ndone == b->dcap) { b->dcap = b->dcap ? b->dcap * 2 : 4; b->done = (sd_chunk **)realloc(b->done, (size_t)b->dcap * sizeof *b->done); }
        b->done[b->ndone++] = b->cur;
    }
    b->cur = NULL;
}

/* parser callback: one record */
static int sd_on_record(void *user, char *seq, size_t len)
{
    sd_builder *b = (sd_builder *)user;
    sd_stream *st = b->st;
    sd_chunk *c = b->cur;
    if (st->cancel) return 1;
    if (c && c->nrec && (c->blen + len + 1 > st->chunk_bytes || c->nrec >= (1u << 22))) { builder_finish_chunk(b); c = NULL; }
    if (!c) c = b->cur = chunk_new();
    if (c->nrec == c->rcap) {
        c->rcap = c->rcap ? c->rcap * 2 : 1u << 16;
        c->len = (uint64_t *)realloc(c->len, (size_t)c->rcap * sizeof *c->len);
    }
    c->len[c->nrec] = len;
    if (len >= SK_K) {
        if (c->np == c->pcap) {
            c->pcap = c->pcap ? c->pcap * 2 : 1u << 16;
            c->pstart = (uint32_t *)realloc(c->pstart, (size_t)c->pcap * sizeof *c->pstart);
            c->prec = (uint32_t *)realloc(c->prec, (size_t)c->pcap * sizeof *c->prec);
        }
        if (!c->buf && len + 1 <= st->chunk_bytes && (c->buf = (uint8_t *)sd_pin_get()) != NULL) {
            c->pinned = 1;                                 /* the usual case: a whole chunk's worth, page-locked */
            c->bcap = st->chunk_bytes;
        }
        if (!c->buf) __atomic_add_fetch(&n_unpinned_chunks, 1, __ATOMIC_RELAXED);     /* (SK_SD_TIMING: the pool was empty or the record too long) */
        if (c->blen + len + 1 > c->bcap) {                 /* a record never straddles chunks: grow instead */
            uint64_t cap = c->bcap ? c->bcap : 1u << 20;
            while (cap < c->blen + len + 1) cap *= 2;
            c->buf = (uint8_t *)realloc(c->buf, cap);      /* (never a pool buffer: those hold chunk_bytes, the most a chunk takes) */
            c->bcap = cap;
        }
        c->pstart[c->np] = (uint32_t)c->blen;
        c->prec[c->np++] = c->nrec;
        memcpy(c->buf + c->blen, seq, len);
        c->blen += len;
        c->buf[c->blen++] = '\n';
    }
    c->nrec++;
    return 0;
}

/* ---- several parser threads on one file ------------------------------------------------------------------------
 * The decode thread (below) only cuts: it gathers the decoded text into segments of about a chunk's worth, each ending
 * at the first line start in its last 64 KiB that looks like a record start (parser_guess_start), and hands them out.
 * A parser thread parses a segment as a file of its own -- the same state machine, its own chunk builder -- and then
 * CHECKS that it stands between two records (parser_between_records): the first segment starts at the file's start,
 * every other at the checked end of the one before, so if all checks hold the segments' records are the file's records
 * (src/kseq.h:171-211 reads from the top; nothing here changes what a record is).  A failed check fails the run with
 * a message (SK_NO_SPLIT=1 turns the cutting off) -- it is never papered over.  Chunks reach the queue in segment
 * order: the replay of the reference's read-after-read bookkeeping (src/strain_detect.c:443-626) sees the file's order. */
static void *sd_parse_worker(void *arg)
{
    sd_stream *st = (sd_stream *)arg;
    ski_rbuf rb = { NULL, 0 };                             /* this thread's block, should it copy */
    const size_t rblk = ski_read_block((size_t)2 << 20);
    pthread_setname_np(pthread_self(), "sk-parse");
    for (;;) {
        sd_seg *sg;
        sd_builder b;
        parser ps;
        int ok = 1, i;
        double w0 = now_s(), w1, w2, w3;
        pthread_mutex_lock(&st->pmu);
        while (st->segn == 0 && !st->seg_done) pthread_cond_wait(&st->pcv, &st->pmu);
        if (st->segn == 0) {
            pthread_mutex_unlock(&st->pmu);
            pthread_mutex_lock(&t_pw_mu); cpu_parsers += thread_cpu_s(); pthread_mutex_unlock(&t_pw_mu);
            free(rb.buf);
            return NULL;
        }
        sg = st->segq[0];
        for (i = 1; i < st->segn; i++) st->segq[i - 1] = st->segq[i];
        st->segn--;
        pthread_cond_broadcast(&st->pcv);
        pthread_mutex_unlock(&st->pmu);

        w1 = now_s();
        memset(&b, 0, sizeof b);
        b.st = st;
        parser_init(&ps, sd_on_record, &b);
        /* a segment of a plain file points into the mapping of the whole file: its pages populated, copied or faulted in (sk_input.h;
         * SK_SD_INPUT=populate|pread|mapped) */
        if (sg->borrowed) (void)ski_feed_span(&ps, sg->buf - sg->off, sg->fd, sg->off, sg->n, &st->in_mode, &rb, rblk, &st->cancel);
        else if (!st->cancel) parser_feed(&ps, sg->buf, sg->n);
        if (!sg->is_last && ps.state != P_STOP && !parser_between_records(&ps)) ok = 0;
        if (ps.state != P_STOP || ps.end_kind != SKP_END_NONE) { /* (stopped by cancel or by a truncated record: the ending stands) */ }
        parser_eof(&ps);
        if (b.cur && (sg->is_last || b.cur->nrec)) builder_finish_chunk(&b);
        else if (b.cur) { chunk_free(b.cur); b.cur = NULL; }

        w2 = now_s();
        pthread_mutex_lock(&st->pmu);                      /* in segment order */
        while (st->next_push != sg->seq && !st->cancel) pthread_cond_wait(&st->pcv, &st->pmu);
        pthread_mutex_unlock(&st->pmu);
        w3 = now_s();
        if (!ok) st->split_failed = 1;
        {
            size_t end_len = ps.end_len;
            if (ps.nrecords) st->carry_last_len = ps.last_len;
            else if (ps.end_kind == SKP_END_STALE) end_len = st->carry_last_len;       /* "the previous record" lies in an earlier segment */
            if (!st->cancel_segments && (sg->is_last || ps.end_kind == SKP_END_TRUNC || st->split_failed)) {  /* the file ends here (a truncated record ends it for the reference too) */
                sd_chunk *c;
                if (b.ndone == 0) { b.cur = chunk_new(); builder_finish_chunk(&b); }
                c = b.done[b.ndone - 1];
                c->last = 1;
                c->end_kind = ps.end_kind;
                c->end_len = end_len;
            }
        }
        {
            const int dropped = st->cancel_segments;            /* an earlier segment ended the file: this one's records do not exist */
            const int file_over = !dropped && b.ndone && b.done[b.ndone - 1]->last;      /* (read before the chunks change hands) */
            for (i = 0; i < b.ndone; i++) { if (dropped) chunk_free(b.done[i]); else stream_push(st, b.done[i]); }
            pthread_mutex_lock(&st->pmu);
            st->next_push++;
            if (file_over) st->cancel_segments = 1;
            pthread_cond_broadcast(&st->pcv);
            pthread_mutex_unlock(&st->pmu);
        }
        pthread_mutex_lock(&t_pw_mu);
        t_pw_seg += w1 - w0; t_pw_parse += w2 - w1; t_pw_turn += w3 - w2; t_pw_push += now_s() - w3;
        pthread_mutex_unlock(&t_pw_mu);
        free(b.done);
        parser_free(&ps);
        if (!sg->borrowed) free(sg->buf);
        free(sg);
    }
}

static sd_seg *sd_seg_new(unsigned char *buf, size_t n, uint64_t seq, int is_last)
{
    sd_seg *sg = (sd_seg *)calloc(1, sizeof *sg);
    sg->buf = buf; sg->n = n; sg->seq = seq; sg->is_last = is_last;
    return sg;
}

/* hand a segment to the parser threads (blocks while all of them are busy and a few wait) */
static void sd_seg_dispatch(sd_stream *st, sd_seg *sg)
{
    pthread_mutex_lock(&st->pmu);
    while ((st->segn == (int)(sizeof st->segq / sizeof st->segq[0]) || st->segn > st->par) && !st->cancel) pthread_cond_wait(&st->pcv, &st->pmu);
    if (st->cancel) { pthread_mutex_unlock(&st->pmu); if (!sg->borrowed) free(sg->buf); free(sg); return; }
    st->segq[st->segn++] = sg;
    pthread_cond_broadcast(&st->pcv);
    pthread_mutex_unlock(&st->pmu);
}

/* ---- plain text parsed on the device (opt-in: option "device_parse" through sk_text_option, or SK_DEVICE_PARSE=1) -------------
 * With the switch on, a mapped plain file is not parsed here at all: the reader thread copies it, piece by piece, into page-locked
 * buffers and queues the pieces AS TEXT; the main thread sends each up (sk_batch_fill_text, ahead of its turn like any chunk) and the
 * device parses it straight into the batch the TALLY scan reads (sk_text.hip).  A piece starts at a verified record boundary -- the
 * file's start, or the end of an accepted piece -- and ends at a GUESSED one (parser_guess_start, as the segments below): nothing
 * is trusted from the guess, the device must consume exactly the piece.  A piece before the last goes up with one byte of
 * look-ahead, the next piece's first byte, so that both device forms count its last record (FASTQ4: four whole lines; FASTA: the
 * next header's character at a line start).  Whatever the device does not take -- a declined piece, another `consumed`, too many
 * records, no cut within one buffer, a last piece without its final '\n' (whose ending the host parser tells apart) -- hands the
 * REST of the file, from that piece's start, to the host path below (segments and parser threads, started at that offset); pieces
 * read ahead beyond it are dropped.  The entry points are weak: the host-only test builds link this file without them, and without
 * them the switch is the host path. */
#pragma weak sk_text_enabled
#pragma weak sk_batch_fill_text
#pragma weak sk_batch_text_finish
enum { SD_VERDICT_DONE = 1, SD_VERDICT_HOST = 2 };
#define SD_TEXT_PIECE_MAX (256ull << 20)               /* the device parser's offsets are 32-bit */
static unsigned long n_text_taken, n_text_declined;    /* SK_SD_TIMING: pieces the device parsed, pieces handed to the host */

static int sd_text_wanted(void)
{
    if (!sk_text_enabled || !sk_batch_fill_text || !sk_batch_text_finish || !sd_dev.ctx[0]) return 0;
    return sk_text_enabled(sd_dev.ctx[0]);
}

/* Where the piece t[0 .. ) of a text of n > cap bytes ends: a guessed record start g with g + 1 <= cap (the piece and its byte of look-ahead
 * fit one buffer), or 0 when there is none.  Looked for in the buffer's last `tail` bytes first, so that pieces are about a buffer
 * long; when that search overshoots (records longer than the tail: contigs, genomes) from ever earlier places -- half way, a quarter,
 * ... the first line -- so any record start inside the buffer is found.  Never more than cap + tail bytes are looked at. */
static size_t sd_text_cut(const unsigned char *t, size_t n, size_t cap, size_t tail)
{
    const size_t lim = n < cap + tail ? n : cap + tail;
    size_t x = cap - tail;
    for (;;) {
        const size_t g = (size_t)parser_guess_start(t, lim, x, lim == n);
        if (g + 1 <= cap) return g;
        if (x <= 1) return 0;
        x /= 2;
    }
}

/* the reader's side.  1: the file is done (every piece accepted, or the stream cancelled); 0: the host path takes over at *from */
static int sd_text_read(sd_stream *st, const unsigned char *map, size_t mlen, int fd, size_t *from)
{
    const size_t room = st->chunk_bytes < sd_pin.bytes ? st->chunk_bytes : sd_pin.bytes;
    const size_t cap = room < SD_TEXT_PIECE_MAX ? room : (size_t)SD_TEXT_PIECE_MAX;      /* piece + look-ahead */
    const size_t tail = cap / 2 < (64u << 10) ? cap / 2 : (64u << 10);                   /* a cut is looked for in the buffer's last bytes */
    size_t at = 0;
    int verdict = 0;
    sd_chunk *spare = chunk_new();                         /* the marker that ends the text, should a chunk not be had later */
    if (!spare) { *from = 0; return 0; }                   /* (nothing is queued yet: the host path takes the whole file) */
    while (at < mlen && !verdict) {
        sd_chunk *c;
        size_t cut = mlen;
        pthread_mutex_lock(&st->mu);
        verdict = st->cancel ? SD_VERDICT_DONE : st->text_verdict;
        pthread_mutex_unlock(&st->mu);
        if (verdict) break;
        if (mlen - at > cap) cut = at + sd_text_cut(map + at, mlen - at, cap, tail);
        if ((c = chunk_new()) == NULL) { c = spare; spare = NULL; cut = at; }      /* (no memory: the host path from here, not a wait for a verdict nobody gives) */
        c->toff = at;
        if (cut == at || (cut == mlen && map[mlen - 1] != '\n')) c->text = SD_TEXT_DECLINED;      /* no cut within one buffer; a last line without its '\n' */
        else {
            size_t have;
            c->text = SD_TEXT_PENDING;
            c->tlen = cut - at;
            c->tla = cut < mlen;
            c->t_eof = cut == mlen;
            if ((c->buf = (uint8_t *)sd_pin_get()) != NULL) c->pinned = 1;
            else { c->buf = (uint8_t *)malloc(cap); __atomic_add_fetch(&n_unpinned_chunks, 1, __ATOMIC_RELAXED); }
            if (!c->buf) { c->text = SD_TEXT_DECLINED; c->tlen = 0; }
            have = c->buf && fd >= 0 ? ski_pread_exact(fd, c->buf, c->tlen + (size_t)c->tla, at) : 0;
            if (c->buf && have < c->tlen + (size_t)c->tla) memcpy(c->buf + have, map + at + have, c->tlen + (size_t)c->tla - have);   /* (a failed read: out of the mapping) */
        }
        {
            const int stop = c->text == SD_TEXT_DECLINED;
            stream_push(st, c);
            if (stop) break;
        }
        at = cut;
    }
    chunk_free(spare);
    pthread_mutex_lock(&st->mu);
    while (!st->cancel && !st->text_verdict) pthread_cond_wait(&st->cv, &st->mu);
    verdict = st->cancel ? SD_VERDICT_DONE : st->text_verdict;
    *from = (size_t)st->text_off;
    pthread_mutex_unlock(&st->mu);
    return verdict != SD_VERDICT_HOST;
}

static void *sd_decode_thread(void *arg)
{
    enum { BLK = 1 << 20 };
    sd_stream *st = (sd_stream *)arg;
    unsigned char *blk = (unsigned char *)malloc(BLK);
    int got;
    skzp zp;
    const int own = !getenv("SK_ZLIB") && skzp_open_threads(&zp, st->path, st->gz_threads) == SKZ_OK;
    /* plain text is parsed straight out of the mapped file (zlib's pass-through mode copies every byte once more: 4.9 GB/s of
     * FASTA against what the parser itself does); anything that cannot be mapped, or SK_ZLIB=1: gzread */
    const unsigned char *map = NULL;
    size_t mlen = 0;
    int map_fd = -1;
    size_t map_from = 0;                                  /* where the host path starts in a mapped file: behind the text the device took */
    if (!own && !getenv("SK_ZLIB")) {
        const int fd = open(st->path, O_RDONLY);
        struct stat sb;
        if (fd >= 0 && fstat(fd, &sb) == 0 && S_ISREG(sb.st_mode) && sb.st_size > 0) {
            void *m = mmap(NULL, (size_t)sb.st_size, PROT_READ, MAP_PRIVATE, fd, 0);
            if (m != MAP_FAILED) { map = (const unsigned char *)m; mlen = (size_t)sb.st_size; madvise(m, mlen, MADV_SEQUENTIAL); }
        }
        if (fd >= 0 && map) map_fd = fd; else if (fd >= 0) close(fd);       /* (kept open for the parser threads' pread, should they go that way) */
        if (map && mlen >= 2 && map[0] == 0x1f && map[1] == 0x8b) { munmap((void *)map, mlen); map = NULL; }   /* (gzip after all: zlib) */
    }
    if (map && st->text_mode && sd_text_read(st, map, mlen, map_fd, &map_from)) {
        /* (every piece of the text went to the device, or the stream was cancelled) */
    } else
    if (st->par > 1 && (own || map)) {
        /* a .gz file inflated by several threads delivers text faster than one thread parses it (measured, 3 Gbase of FASTA,
         * 16 inflate threads: waiting for the decode side 0.73 s with one parser, 0.47 s with four), and so does a mapped
         * plain file when many strains wait for it (32 strains x 10 Gbase of FASTA: the one parser thread, 3 GB/s, was what the
         * whole pass waited for).  Cut the text into segments for the parser threads -- copied out of the inflate stream, or
         * simply pointing into the map: */
        pthread_t wk[SD_PARSERS_MAX];
        int nw = 0, i;
        uint64_t seq = 0;
        const size_t want = st->chunk_bytes;              /* about a chunk's worth of text per segment */
        {   /* a mapped file costs nothing to read: with a whole thread budget behind one file, eight parsers (an inflating
             * file keeps its four: the inflate threads need the CPUs) */
            const int npar = map && !getenv("SK_PARSE_THREADS") && st->gz_threads >= 16 ? SD_PARSERS_MAPPED : st->par;
            for (i = 0; i < npar && i < SD_PARSERS_MAX; i++) if (pthread_create(&wk[nw], NULL, sd_parse_worker, st) == 0) nw++;
        }
        if (map) {
            size_t at = map_from;
            while (at < mlen && nw) {
                size_t cut = mlen;
                int over;
                sd_seg *sg;
                pthread_mutex_lock(&st->pmu);
                over = st->cancel_segments;
                pthread_mutex_unlock(&st->pmu);
                if (st->cancel || over) break;
                if (mlen - at > want + ski_cut_tail(want)) cut = at + (size_t)parser_guess_start(map + at, mlen - at, want, 1);
                sg = sd_seg_new((unsigned char *)map + at, cut - at, seq++, cut == mlen);
                sg->borrowed = 1; sg->fd = map_fd; sg->off = at;
                sd_seg_dispatch(st, sg);
                at = cut;
            }
        } else {
            ski_cutter ct;                                 /* the inflated text gathered and cut (sk_input.h) */
            unsigned char *buf; size_t len;
            ski_cutter_init(&ct, want);
            for (;;) {
                const unsigned char *data = NULL;
                size_t n = 0;
                int over;
                pthread_mutex_lock(&st->pmu);
                over = st->cancel_segments;
                pthread_mutex_unlock(&st->pmu);
                if (st->cancel || over || nw == 0) break;
                if (own) n = skzp_next(&zp, &data);
                else { got = gzread(st->g, blk, BLK); n = got > 0 ? (size_t)got : 0; data = blk; }
                if (n == 0) break;
                ski_cutter_add(&ct, data, n);
                if (ski_cutter_take(&ct, &buf, &len)) sd_seg_dispatch(st, sd_seg_new(buf, len, seq++, 0));     /* (one cut per delivery) */
            }
            ski_cutter_rest(&ct, &buf, &len);
            if (nw) sd_seg_dispatch(st, sd_seg_new(buf, len, seq++, 1)); else free(buf);
        }
        pthread_mutex_lock(&st->pmu);
        st->seg_done = 1;
        pthread_cond_broadcast(&st->pcv);
        pthread_mutex_unlock(&st->pmu);
        for (i = 0; i < nw; i++) pthread_join(wk[i], NULL);
        if (nw == 0) {                                     /* no thread could be started: an empty, failed file rather than a hang */
            sd_chunk *c = chunk_new();
            c->last = 1; c->end_kind = SKP_END_RESET;
            st->split_failed = 1;
            stream_push(st, c);
        }
    } else {
        /* this thread parses: gzip through the library's own inflate on a helper thread (sk_gzpipe.h); plain files, or
         * SK_ZLIB=1, through zlib */
        parser ps;
        sd_builder b;
        sd_chunk *c;
        memset(&b, 0, sizeof b);
        b.st = st; b.direct = 1;
        parser_init(&ps, sd_on_record, &b);
        if (own) {
            const unsigned char *data;
            size_t n;
            while (ps.state != P_STOP && !st->cancel && (n = skzp_next(&zp, &data)) > 0) parser_feed(&ps, data, n);
        } else {
            if (map) {
                size_t at = map_from;
                while (ps.state != P_STOP && !st->cancel && at < mlen) {
                    const size_t n = mlen - at < (4u << 20) ? mlen - at : (4u << 20);
                    parser_feed(&ps, map + at, n);
                    at += n;
                }
            } else
                while (ps.state != P_STOP && !st->cancel && (got = gzread(st->g, blk, BLK)) > 0) parser_feed(&ps, blk, (size_t)got);
        }
        parser_eof(&ps);
        c = b.cur ? b.cur : chunk_new();
        b.cur = NULL;
        c->last = 1;
        c->end_kind = ps.end_kind;
        c->end_len = !ps.nrecords && ps.end_kind == SKP_END_STALE ? st->carry_last_len : ps.end_len;   /* ("the previous record" may lie in text the device took: 0 otherwise, as end_len) */
        stream_push(st, c);
        parser_free(&ps);
    }
    if (own) skzp_close(&zp);
    if (map) sd_unmap_later((void *)map, mlen);
    if (map_fd >= 0) close(map_fd);
    free(blk);
    pthread_mutex_lock(&t_pw_mu); cpu_readers += thread_cpu_s(); pthread_mutex_unlock(&t_pw_mu);
    return NULL;
}


/* ---- the target cache (opt-in: --target-cache DIR or SK_TARGET_CACHE=DIR; SK_TARGET_CACHE_MODE=rw|ro) -----------------------------
 * The same metagenomes are tracked again for every new strain, drug or donor, and each run inflates and parses them from scratch.
 * With the switch on, what the decode side hands to the main thread for one target file -- its chunks: the record stream and the
 * length of every record -- is kept in DIR, one file per target (sk_pcache.h, version 2, .skt), the stream in sk_pack_stream's form,
 * and a later run is SERVED from it: one thread per file reads segment after segment into a pool buffer, checks its sum, rebuilds
 * len/pstart/prec by sd_on_record's rule and queues the chunk -- no inflate, no parser threads, no segments; the chunks go up through
 * sk_batch_fill_packed as SK_SD_PACK=1 chunks do.
 * FILLING costs the decode threads nothing: a chunk goes up as bytes as ever, the DEVICE packs it where it lies in the batch, behind
 * its upload and beside its scans (sk_batch_pack_home), and one writer thread per stream waits for the packed form and appends it --
 * or the chunk's bytes, when it holds a byte for the byte-string kernel.  The main thread hands the chunk on (with a reference) and
 * goes on; the writer's queue holds four chunks, so memory stays bounded and the appends come in the file's order -- a writer that
 * falls four chunks behind is waited for.  Without the device entry points (the host-only builds) the writer packs with
 * sk_pack_stream.  A file takes its name only when the chunk with `last` set was appended and nothing failed: a cancelled stream, a
 * failed split, a PE1 abandoned because PE2 ended first leave nothing.  Pieces of text for the device's parser are not written.
 * A served file that fails a sum or a structure check FAILS the run (SK_E_CACHE, the file named): hit lines of earlier chunks are
 * out already. */
#pragma weak sk_batch_pack_home
#pragma weak sk_batch_pack_wait
typedef struct { uint64_t served, written, stale, not_cached; double t_sum, t_read, t_write, t_pack; } sd_tc_counts;
static struct { char *dir; int ro; } sd_tc;
static sd_tc_counts sd_tc_run, sd_tc_all;             /* this run's; the process's (skh_target_cache_stats) */
static pthread_mutex_t sd_tc_mu = PTHREAD_MUTEX_INITIALIZER;

int skh_target_cache_stats(uint64_t *served, uint64_t *written, uint64_t *stale, uint64_t *not_cached, int reset)
{
    pthread_mutex_lock(&sd_tc_mu);
    if (served) *served = sd_tc_all.served;
    if (written) *written = sd_tc_all.written;
    if (stale) *stale = sd_tc_all.stale;
    if (not_cached) *not_cached = sd_tc_all.not_cached;
    if (reset) memset(&sd_tc_all, 0, sizeof sd_tc_all);
    pthread_mutex_unlock(&sd_tc_mu);
    return SK_OK;
}

#define SD_TCW_QUEUE 4
typedef struct sd_tcw {
    skpc_writer *w;
    pthread_t th;
    pthread_mutex_t mu; pthread_cond_t cv;
    struct { sd_chunk *c; sk_batch *b; uint8_t *pk; } q[SD_TCW_QUEUE];      /* b, pk: the batch that packs the chunk and where its packed form lands (or none) */
    int qn, closing;
    int failed, saw_last;                    /* (the writer thread's own until it is joined) */
    uint64_t records, bases;
    double t_pack;
} sd_tcw;

/* where the device's odd flag lands in a pool buffer: its last aligned u32 */
static uint32_t *sd_tc_flag(uint8_t *pk) { return (uint32_t *)(pk + ((sd_pin.bytes - 4u) & ~(size_t)3u)); }

/* one chunk into the file */
static void sd_tcw_append(sd_tcw *w, sd_chunk *c, uint8_t *pk, int pk_ok)
{
    uint32_t kind = SKPC_PACKED, i;
    const uint8_t *src = NULL;
    uint8_t *own = NULL, *dst;
    uint64_t raw = 0, part, plen, bases = 0;
    if (c->np) {
        if (pk_ok && !*sd_tc_flag(pk)) src = pk;
        else if (c->packed) src = c->buf;
        else if (pk_ok) { kind = SKPC_BYTES; src = c->buf; }                  /* (the device saw a byte for the byte-string kernel) */
        else {
            int odd = 0;
            own = (uint8_t *)malloc((size_t)skpt_payload_len(SKPC_PACKED, c->blen, c->nrec) + 8u);
            if (!own || sk_pack_stream(c->buf, c->blen, own, &odd) != SK_OK) { free(own); w->failed = 1; return; }
            if (odd) { free(own); own = NULL; kind = SKPC_BYTES; src = c->buf; } else src = own;
        }
        raw = kind == SKPC_PACKED ? skpc_packed_bytes(c->blen) : c->blen;
    }
    for (i = 0; i < c->nrec; i++) {
        if (c->len[i] > 0xFFFFFFFFull) { free(own); w->failed = 1; return; }   /* a record of 2^32 bases or more: this target is not cached */
        bases += c->len[i];
    }
    part = skpt_stream_part(kind, c->blen);
    plen = skpt_payload_len(kind, c->blen, c->nrec);
    if (src && src == own) dst = own;
    else if (pk && plen <= sd_pin.bytes) dst = pk;
    else dst = own = (uint8_t *)malloc((size_t)plen + 8u);
    if (!dst) { w->failed = 1; return; }
    if (src && src != dst) memcpy(dst, src, (size_t)raw);
    memset(dst + raw, 0, (size_t)(part - raw));
    for (i = 0; i < c->nrec; i++) skpc_put32(dst + part + 4u * (size_t)i, (uint32_t)c->len[i]);
    skpt_append(w->w, kind, c->blen, c->nrec, c->np, c->last, (uint32_t)c->end_kind, (uint64_t)c->end_len, dst);
    w->records += c->nrec; w->bases += bases;
    if (c->last) w->saw_last = 1;
    free(own);
}

static void *sd_tcw_thread(void *arg)
{
    sd_tcw *w = (sd_tcw *)arg;
    pthread_setname_np(pthread_self(), "sk-tcache");
    for (;;) {
        sd_chunk *c; sk_batch *b; uint8_t *pk;
        int i, pk_ok = 0;
        pthread_mutex_lock(&w->mu);
        while (w->qn == 0 && !w->closing) pthread_cond_wait(&w->cv, &w->mu);
        if (w->qn == 0) { pthread_mutex_unlock(&w->mu); return NULL; }
        c = w->q[0].c; b = w->q[0].b; pk = w->q[0].pk;
        for (i = 1; i < w->qn; i++) w->q[i - 1] = w->q[i];
        w->qn--;
        pthread_cond_broadcast(&w->cv);
        pthread_mutex_unlock(&w->mu);
        if (b) {                                           /* (always waited for: the copy home must have landed before the buffer goes back to the pool) */
            const double t0 = now_s();
            pk_ok = sk_batch_pack_wait(b) == SK_OK;
            w->t_pack += now_s() - t0;
            if (!pk_ok) { w->failed = 1; pk = NULL; }      /* (a device error: the buffer is not reused) */
        }
        if (!w->failed) sd_tcw_append(w, c, pk, pk_ok);
        if (pk) sd_pin_put(pk);
        chunk_free(c);
    }
}

/* the main thread's side: chunk c, whose bytes device 0's batch b0 has just been sent (NULL: a chunk without a record of k bases), is
 * the next of its stream's file */
static void sd_tc_hand(sd_stream *st, sd_chunk *c, sk_batch *b0)
{
    sd_tcw *w = st ? st->tcw : NULL;
    uint8_t *pk = NULL;
    sk_batch *pb = NULL;
    if (!w || c->tc_handed || c->text) return;
    c->tc_handed = 1;
    if (b0 && c->np && !c->packed && sk_batch_pack_home && sk_batch_pack_wait && skpc_pad8(skpc_packed_bytes(c->blen)) + 8u <= sd_pin.bytes &&
        (pk = (uint8_t *)sd_pin_get()) != NULL) {
        if (sk_batch_pack_home(b0, pk, sd_tc_flag(pk)) == SK_OK) pb = b0;
        else { sd_pin_put(pk); pk = NULL; }                /* (the writer packs it) */
    }
    chunk_ref(c);
    pthread_mutex_lock(&w->mu);
    while (w->qn == SD_TCW_QUEUE) pthread_cond_wait(&w->cv, &w->mu);
    w->q[w->qn].c = c; w->q[w->qn].b = pb; w->q[w->qn].pk = pk;
    w->qn++;
    pthread_cond_broadcast(&w->cv);
    pthread_mutex_unlock(&w->mu);
}

/* the stream is over (its batches are still there): the writer runs dry, and the file is kept if it holds the whole target */
static void sd_tc_finish(sd_stream *st)
{
    sd_tcw *w = st->tcw;
    int kept;
    if (!w) return;
    pthread_mutex_lock(&w->mu);
    w->closing = 1;
    pthread_cond_broadcast(&w->cv);
    pthread_mutex_unlock(&w->mu);
    pthread_join(w->th, NULL);
    pthread_mutex_lock(&sd_tc_mu);
    sd_tc_run.t_sum += w->w->t_sum; sd_tc_run.t_write += w->w->t_write; sd_tc_run.t_pack += w->t_pack;
    pthread_mutex_unlock(&sd_tc_mu);
    kept = skpc_end(w->w, w->saw_last && !w->failed && !st->split_failed, w->records, w->bases);
    pthread_mutex_lock(&sd_tc_mu);
    if (kept) sd_tc_run.written++; else sd_tc_run.not_cached++;
    pthread_mutex_unlock(&sd_tc_mu);
    pthread_mutex_destroy(&w->mu);
    pthread_cond_destroy(&w->cv);
    free(w);
    st->tcw = NULL;
}

/* the serving thread: the decode thread's place for a file whose cache holds */
static void *sd_serve_thread(void *arg)
{
    sd_stream *st = (sd_stream *)arg;
    double t_sum = 0, t_read = 0;
    int rc;
    pthread_setname_np(pthread_self(), "sk-tserve");
    for (;;) {
        skpt_seg sg;
        sd_chunk *c;
        const uint8_t *tab;
        uint64_t at = 0;
        uint32_t i, np = 0;
        pthread_mutex_lock(&st->mu);
        i = (uint32_t)st->cancel;
        pthread_mutex_unlock(&st->mu);
        if (i) { rc = SKPC_OK; break; }
        if ((rc = skpt_next(&st->tcr, &sg)) != SKPC_OK) { if (rc == SKPC_MISS) rc = SKPC_OK; break; }     /* (behind the last segment) */
        if ((c = chunk_new()) == NULL) { rc = SKPC_IO; break; }
        if (sg.payload_len <= sd_pin.bytes && (c->buf = (uint8_t *)sd_pin_get()) != NULL) { c->pinned = 1; c->bcap = sd_pin.bytes; }
        else {                                             /* a chunk longer than a pool buffer: ordinary memory, as the builder does */
            c->buf = (uint8_t *)malloc((size_t)sg.payload_len + 8u);
            c->bcap = sg.payload_len + 8u;
            if (sg.np) __atomic_add_fetch(&n_unpinned_chunks, 1, __ATOMIC_RELAXED);
        }
        c->len = (uint64_t *)malloc(((size_t)sg.nrec + 1) * sizeof *c->len);
        c->pstart = (uint32_t *)malloc(((size_t)sg.np + 1) * sizeof *c->pstart);
        c->prec = (uint32_t *)malloc(((size_t)sg.np + 1) * sizeof *c->prec);
        if (!c->buf || !c->len || !c->pstart || !c->prec) { chunk_free(c); rc = SKPC_IO; break; }
        if ((rc = skpt_payload(&st->tcr, &sg, c->buf, &t_sum, &t_read)) != SKPC_OK || (rc = skpt_lengths(&sg, c->buf)) != SKPC_OK) { chunk_free(c); break; }
        tab = skpt_table(&sg, c->buf);
        for (i = 0; i < sg.nrec; i++) {                    /* sd_on_record's rule */
            const uint32_t l = skpc_le32(tab + 4u * (size_t)i);
            c->len[i] = l;
            if (l >= SK_K) { c->pstart[np] = (uint32_t)at; c->prec[np++] = i; at += (uint64_t)l + 1u; }
        }
        c->nrec = c->rcap = sg.nrec; c->np = np; c->pcap = sg.np + 1;
        c->blen = sg.stream_len;
        c->packed = sg.kind == SKPC_PACKED && sg.np;
        c->last = (sg.flags & SKPT_LAST) != 0; c->end_kind = (int)sg.end_kind; c->end_len = (size_t)sg.end_len;
        stream_push(st, c);
    }
    if (rc != SKPC_OK) {                                   /* the main thread fails the run when it comes to this marker */
        sd_chunk *c = chunk_new();
        if (c) { c->last = 1; c->cache_err = rc; c->end_kind = SKP_END_RESET; stream_push(st, c); }
    }
    pthread_mutex_lock(&sd_tc_mu);
    sd_tc_run.t_sum += t_sum; sd_tc_run.t_read += t_read;
    pthread_mutex_unlock(&sd_tc_mu);
    pthread_mutex_lock(&t_pw_mu); cpu_readers += thread_cpu_s(); pthread_mutex_unlock(&t_pw_mu);
    return NULL;
}

/* stream_open's part: is the file served, and if not, is it filled?  (Decided before the device's text parser gets a say: a file that
 * is served is not text for it; one it may take is not written.) */
static void sd_tc_stream(sd_stream *st)
{
    struct stat sb;
    int rc;
    if (!sd_tc.dir) return;
    if (stat(st->path, &sb) != 0 || !S_ISREG(sb.st_mode) || (st->tc_path = skpt_path(sd_tc.dir, st->path)) == NULL) {
        pthread_mutex_lock(&sd_tc_mu); sd_tc_run.not_cached++; pthread_mutex_unlock(&sd_tc_mu);
        return;
    }
    rc = skpt_open(&st->tcr, st->tc_path, &sb);
    if (rc == SKPC_OK) {
        st->serving = 1;
        st->text_mode = 0;
        pthread_mutex_lock(&sd_tc_mu); sd_tc_run.served++; pthread_mutex_unlock(&sd_tc_mu);
        return;
    }
    if (rc == SKPC_INVALID) { pthread_mutex_lock(&sd_tc_mu); sd_tc_run.stale++; pthread_mutex_unlock(&sd_tc_mu); }
    if (sd_tc.ro) return;
    if (st->text_mode) { pthread_mutex_lock(&sd_tc_mu); sd_tc_run.not_cached++; pthread_mutex_unlock(&sd_tc_mu); return; }
    {
        sd_tcw *w = (sd_tcw *)calloc(1, sizeof *w);
        if (w && (w->w = skpt_begin(st->tc_path, &sb)) != NULL) {
            pthread_mutex_init(&w->mu, NULL);
            pthread_cond_init(&w->cv, NULL);
            if (pthread_create(&w->th, NULL, sd_tcw_thread, w) == 0) { st->tcw = w; return; }
            pthread_mutex_destroy(&w->mu);
            pthread_cond_destroy(&w->cv);
            skpc_end(w->w, 0, 0, 0);
        }
        free(w);
        pthread_mutex_lock(&sd_tc_mu); sd_tc_run.not_cached++; pthread_mutex_unlock(&sd_tc_mu);
    }
}

/* the run's switch: DIR from the command line or SK_TARGET_CACHE; a directory that cannot be used is said once and the run goes on
 * uncached */
static void sd_tc_open(const char *dir, FILE *err)
{
    const char *m = getenv("SK_TARGET_CACHE_MODE");
    struct stat sb;
    memset(&sd_tc_run, 0, sizeof sd_tc_run);
    sd_tc.dir = NULL;
    if (!dir || !*dir) dir = getenv("SK_TARGET_CACHE");
    if (!dir || !*dir) return;
    sd_tc.ro = m && !strcmp(m, "ro");
    if (stat(dir, &sb) != 0 || !S_ISDIR(sb.st_mode) || access(dir, sd_tc.ro ? R_OK | X_OK : R_OK | W_OK | X_OK) != 0) {
        fprintf(err, "strain_detect: the target cache directory %s cannot be used (%s): going on without it\n", dir, sb.st_mode && !S_ISDIR(sb.st_mode) ? "not a directory" : strerror(errno));
        return;
    }
    sd_tc.dir = strdup(dir);
}

static void sd_tc_close(FILE *err)
{
    if (sd_tc.dir && (getenv("SK_SD_TIMING") || getenv("SK_TIMING")))
        fprintf(err, "target cache: %s: %llu files served, %llu written, %llu stale, %llu not cached; checksums %.2f s, reading %.2f s, writing %.2f s, "
                     "waiting for the device pack %.2f s\n", sd_tc.dir, (unsigned long long)sd_tc_run.served, (unsigned long long)sd_tc_run.written,
                (unsigned long long)sd_tc_run.stale, (unsigned long long)sd_tc_run.not_cached, sd_tc_run.t_sum, sd_tc_run.t_read, sd_tc_run.t_write, sd_tc_run.t_pack);
    pthread_mutex_lock(&sd_tc_mu);
    sd_tc_all.served += sd_tc_run.served; sd_tc_all.written += sd_tc_run.written; sd_tc_all.stale += sd_tc_run.stale; sd_tc_all.not_cached += sd_tc_run.not_cached;
    memset(&sd_tc_run, 0, sizeof sd_tc_run);
    pthread_mutex_unlock(&sd_tc_mu);
    free(sd_tc.dir);
    sd_tc.dir = NULL;
}

/* how many threads may inflate each of the `nfiles` files read at the same time: SK_GZ_THREADS, or the host
 * thread budget (SK_THREADS, default min(16, usable CPUs)) shared out -- used when it leaves three or more per
 * file, below that the one helper thread of sk_gzpipe.h does as well */
static int sd_gz_threads(int nfiles)
{
    const long ncpu = sk_cpu_budget();
    const int budget = getenv("SK_THREADS") ? atoi(getenv("SK_THREADS")) : (int)(ncpu < 1 ? 1 : ncpu > 16 ? 16 : ncpu);
    int per = budget / nfiles;
    if (getenv("SK_GZ_THREADS")) per = atoi(getenv("SK_GZ_THREADS"));
    return per >= 3 ? (per > 16 ? 16 : per) : 1;
}

/* SK_E_OPEN if the file cannot be opened (nothing started) */
static int stream_open(sd_stream *st, const char *path, int gz_threads)
{
    memset(st, 0, sizeof *st);
    st->path = path;
    st->gz_threads = gz_threads;
    st->chunk_bytes = sd_chunk_bytes();
    {   /* SK_SD_INPUT=populate|pread|mapped (SK_SD_MAPPED=1: the round-3 way, kept for the A/B) */
        const char *e = getenv("SK_SD_INPUT");
        st->in_mode = e && !strcmp(e, "pread") ? SKI_PREAD : (e && !strcmp(e, "mapped")) || getenv("SK_SD_MAPPED") ? SKI_MAPPED : SKI_POPULATE;
    }
    {   /* parser threads for this file: when the budget leaves several threads per file (the case of one or two big
         * metagenomes), a quarter of them parse; SK_PARSE_THREADS sets the number, SK_NO_SPLIT=1 means one */
        const char *e = getenv("SK_PARSE_THREADS");
        st->par = e ? atoi(e) : (gz_threads >= 8 ? 4 : gz_threads >= 3 ? 2 : 1);
        if (getenv("SK_NO_SPLIT") || st->par < 2) st->par = 1;
        if (st->par > SD_PARSERS_MAX) st->par = SD_PARSERS_MAX;
    }
    st->text_mode = sd_text_wanted();
    pthread_mutex_init(&st->pmu, NULL);
    pthread_cond_init(&st->pcv, NULL);
    st->g = gzopen(path, "r");
    if (!st->g) return SK_E_OPEN;
    gzbuffer(st->g, 1 << 18);
    pthread_mutex_init(&st->mu, NULL);
    pthread_cond_init(&st->cv, NULL);
    sd_tc_stream(st);
    if (pthread_create(&st->th, NULL, st->serving ? sd_serve_thread : sd_decode_thread, st)) {
        if (st->serving) skpc_close(&st->tcr);
        if (st->tcw) { st->split_failed = 1; sd_tc_finish(st); }
        free(st->tc_path);
        gzclose(st->g); st->g = NULL; return SK_E_NOMEM;
    }
    st->started = 1;
    return SK_OK;
}

static void sd_drain_scans(void);

/* Device batches outlive the file they were made for: a `-B` list opens and closes a stream per line, and making and freeing a
 * batch (two device buffers, a stream, an event) per file cost more than scanning a small file.  A closed stream's batches wait
 * here, per device, for the next stream; sd_run frees them at its end. */
static struct { sk_batch *b[SD_MAX_DEV][4]; int n[SD_MAX_DEV]; } sd_bcache;
static int sd_batch_get(int d, sk_batch **out)
{
    if (sd_bcache.n[d] > 0) { *out = sd_bcache.b[d][--sd_bcache.n[d]]; return SK_OK; }
    return sk_batch_create(sd_dev.ctx[d], out);
}
static void sd_batch_put(int d, sk_batch *b)
{
    if (!b) return;
    if (sd_bcache.n[d] < 4 && sk_batch_sync(b) == SK_OK) sd_bcache.b[d][sd_bcache.n[d]++] = b;   /* (sync: an upload in flight must land before the chunks go) */
    else sk_batch_destroy(b);
}
static void sd_batch_cache_close(void)
{
    int d;
    for (d = 0; d < SD_MAX_DEV; d++) while (sd_bcache.n[d] > 0) sk_batch_destroy(sd_bcache.b[d][--sd_bcache.n[d]]);
}

/* Unmapping a plain file that was parsed out of its mapping (10 GB: 0.2 s of page-table work) happens behind the next file's scan,
 * on a thread of its own; one at a time, the last one joined by sd_run. */
static struct { pthread_t th; int live; void *p; size_t n; } sd_unmapper;
static pthread_mutex_t sd_unmapper_mu = PTHREAD_MUTEX_INITIALIZER;
static void *sd_unmap_thread(void *arg) { (void)arg; munmap(sd_unmapper.p, sd_unmapper.n); return NULL; }
static void sd_unmap_wait(void)
{
    pthread_mutex_lock(&sd_unmapper_mu);
    if (sd_unmapper.live) { pthread_join(sd_unmapper.th, NULL); sd_unmapper.live = 0; }
    pthread_mutex_unlock(&sd_unmapper_mu);
}
static void sd_unmap_later(void *p, size_t n)
{
    /* wait for the one before and start this one under ONE hold of the lock: with the lock let go in between, two decode threads
     * could both find nobody to wait for, and the second would overwrite what the first one's thread is about to unmap */
    pthread_mutex_lock(&sd_unmapper_mu);
    if (sd_unmapper.live) { pthread_join(sd_unmapper.th, NULL); sd_unmapper.live = 0; }
    sd_unmapper.p = p; sd_unmapper.n = n;
    if (pthread_create(&sd_unmapper.th, NULL, sd_unmap_thread, NULL) == 0) sd_unmapper.live = 1;
    else munmap(p, n);
    pthread_mutex_unlock(&sd_unmapper_mu);
}

static void stream_close(sd_stream *st)
{
    int i;
    if (!st->g) return;
    if (st->ahead) sd_drain_scans();                       /* scans started ahead on a batch that is about to go */
    if (st->started) {
        pthread_mutex_lock(&st->mu);
        st->cancel = 1;
        pthread_cond_broadcast(&st->cv);
        pthread_mutex_unlock(&st->mu);
        pthread_mutex_lock(&st->pmu);                      /* parser threads waiting for a segment or for their turn */
        pthread_cond_broadcast(&st->pcv);
        pthread_mutex_unlock(&st->pmu);
        pthread_join(st->th, NULL);
        pthread_mutex_destroy(&st->mu);
        pthread_cond_destroy(&st->cv);
        pthread_mutex_destroy(&st->pmu);
        pthread_cond_destroy(&st->pcv);
    }
    sd_tc_finish(st);                                   /* (before the batches go: the writer waits for their packs) */
    if (st->serving) skpc_close(&st->tcr);
    free(st->tc_path);
    for (i = 0; i < SD_MAX_DEV; i++) {
        sd_batch_put(i, st->bat[0][i]);                 /* (waits for an upload in flight before the chunks go) */
        sd_batch_put(i, st->bat[1][i]);
    }
    for (i = 0; i < st->qn; i++) chunk_free(st->q[i]);
    chunk_free(st->c);
    chunk_free(st->cur);
    gzclose(st->g);
    memset(st, 0, sizeof *st);
}

/* SK_SD_TIMING=1: where the wall clock went, on stderr at exit */
static double t_wait, t_tally, t_setup, t_fill, t_launch, t_post, t_close, t_lens, t_replay, t_sopen, t_sclose, t_uclose, t_cfree;
static double t_open_ctx, t_open_load, t_open_flags;     /* thread time summed over the strains' worker threads (SK_SD_TIMING) */
static pthread_mutex_t t_open_mu = PTHREAD_MUTEX_INITIALIZER;
static double now_s(void) { struct timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec; }

/* The strains are independent once a chunk is on the device: the per-strain work -- collecting and spreading a
 * chunk's tallies, replaying a run (and with it the gz compression of each strain's own output), closing a strain
 * -- is dealt out strain by strain to a few threads.  pool_run(pool, n, fn, arg) calls fn(arg, s) for every s < n,
 * the calling thread being one of the workers, and returns when all are done. */
typedef void (*sd_job_fn)(void *arg, uint32_t s);
typedef struct {
    pthread_t th[16]; int nth;
    pthread_mutex_t mu; pthread_cond_t cv_work, cv_done;
    unsigned long gen; int quit;
    sd_job_fn fn; void *arg; uint32_t ns;
    uint64_t ticket;                 /* (job number << 32) | next item: an item is claimed by a CAS that also proves the job is still the same */
    uint32_t done;
} sd_pool;

/* Items of job `job` are claimed through ONE word that holds the job's number beside the item counter: a worker that comes late
 * out of the previous job cannot take an item of the next one (nor read that job's fn/arg/ns half written) -- its CAS fails on
 * the job number.  fn, arg and ns are written before the release store that opens the job and read after an acquire load of the
 * ticket that shows the job's number.  (ThreadSanitizer found the old form -- a bare counter, ns read without order -- with five
 * strains on four threads.) */
static void pool_drain(sd_pool *pl, uint32_t job, uint32_t ns, sd_job_fn fn, void *arg)     /* (the job's own ns/fn/arg, read under the mutex) */
{
    uint32_t mine = 0;
    for (;;) {
        uint64_t t = __atomic_load_n(&pl->ticket, __ATOMIC_ACQUIRE);
        if ((uint32_t)(t >> 32) != job || (uint32_t)t >= ns) break;
        if (!__atomic_compare_exchange_n(&pl->ticket, &t, t + 1, 0, __ATOMIC_ACQ_REL, __ATOMIC_ACQUIRE)) continue;
        fn(arg, (uint32_t)t);
        mine++;
    }
    if (!mine) return;
    pthread_mutex_lock(&pl->mu);
    pl->done += mine;
    if (pl->done == pl->ns) pthread_cond_broadcast(&pl->cv_done);
    pthread_mutex_unlock(&pl->mu);
}

static void *pool_worker_sd(void *arg)
{
    sd_pool *pl = (sd_pool *)arg;
    unsigned long seen = 0;
    pthread_setname_np(pthread_self(), "sk-pool");
    for (;;) {
        pthread_mutex_lock(&pl->mu);
        while (pl->gen == seen && !pl->quit) pthread_cond_wait(&pl->cv_work, &pl->mu);
        if (pl->quit) { pthread_mutex_unlock(&pl->mu); return NULL; }
        seen = pl->gen;
        {
            const uint32_t ns = pl->ns;
            const sd_job_fn fn = pl->fn;
            void *const arg = pl->arg;
            pthread_mutex_unlock(&pl->mu);
            pool_drain(pl, (uint32_t)seen, ns, fn, arg);
        }
    }
}

static void pool_start(sd_pool *pl, uint32_t ns)
{
    int want = getenv("SK_THREADS") ? atoi(getenv("SK_THREADS")) : 8, i;
    memset(pl, 0, sizeof *pl);
    if (want > 16) want = 16;
    if ((uint32_t)want > ns) want = (int)ns;
    pthread_mutex_init(&pl->mu, NULL);
    pthread_cond_init(&pl->cv_work, NULL);
    pthread_cond_init(&pl->cv_done, NULL);
    for (i = 0; i + 1 < want; i++)                       /* the calling thread is one of the workers */
        if (pthread_create(&pl->th[pl->nth], NULL, pool_worker_sd, pl) == 0) pl->nth++;
}

static void pool_stop(sd_pool *pl)
{
    int i;
    pthread_mutex_lock(&pl->mu);
    pl->quit = 1;
    pthread_cond_broadcast(&pl->cv_work);
    pthread_mutex_unlock(&pl->mu);
    for (i = 0; i < pl->nth; i++) pthread_join(pl->th[i], NULL);
    pthread_mutex_destroy(&pl->mu);
    pthread_cond_destroy(&pl->cv_work);
    pthread_cond_destroy(&pl->cv_done);
}

static void pool_run(sd_pool *pl, uint32_t ns, sd_job_fn fn, void *arg)
{
    if (!pl || pl->nth == 0 || ns < 2) {
        uint32_t s;
        for (s = 0; s < ns; s++) fn(arg, s);
        return;
    }
    uint32_t job;
    pthread_mutex_lock(&pl->mu);                         /* (every item of the previous job is done: nobody reads fn/arg/ns now) */
    pl->fn = fn; pl->arg = arg; pl->ns = ns;
    pl->done = 0;
    pl->gen++;
    job = (uint32_t)pl->gen;
    __atomic_store_n(&pl->ticket, (uint64_t)job << 32, __ATOMIC_RELEASE);
    pthread_cond_broadcast(&pl->cv_work);
    pthread_mutex_unlock(&pl->mu);
    pool_drain(pl, job, ns, fn, arg);
    pthread_mutex_lock(&pl->mu);
    while (pl->done != pl->ns) pthread_cond_wait(&pl->cv_done, &pl->mu);
    pthread_mutex_unlock(&pl->mu);
}

static int tally_rec_cmp(const void *a, const void *b)
{
    const sk_tally_rec *x = (const sk_tally_rec *)a, *y = (const sk_tally_rec *)b;
    return x->rec < y->rec ? -1 : x->rec > y->rec;
}

static int hit_cmp(const void *a, const void *b)
{
    const sk_hit *x = (const sk_hit *)a, *y = (const sk_hit *)b;
    return x->pos < y->pos ? -1 : x->pos > y->pos;
}

/* One strain's share of a chunk's scan results (c->res_*: collected and dealt out by the main thread) -> the per-record tallies
 * and per-record lists of informative rows, in window order (c->sp[s]). */
static void tally_one(sd_prog *p, sd_chunk *c, uint32_t s)
{
    uint64_t nh = 0, h = 0;
    uint32_t n = 0, k;
    sd_sp *sp = &c->sp[s];
    memset(sp, 0, sizeof *sp);
    if (c->np == 0 || !c->res_off) return;
    /* only the pieces that hit this strain at all came back (compacted on the device): with many strains against one
     * metagenome nearly every (read, strain) pair is a blank */
    sk_tally_rec *sparse = c->res_recs + c->res_off[s];
    sk_hit *hits = c->res_hits + c->res_hoff[s];
    const uint64_t nsp = c->res_off[s + 1] - c->res_off[s];
    uint64_t e;
    nh = c->res_hoff[s + 1] - c->res_hoff[s];
    (void)p;
    /* in the order of the pieces (they come back unordered): a sort when they are few, a sweep over a piece-indexed
     * array when most pieces hit (one strain, reads from that strain) */
    if (nsp * 8 > c->np) {
        uint32_t *by = (uint32_t *)calloc((size_t)c->np, 2 * sizeof(uint32_t));
        uint64_t w = 0;
        for (e = 0; e < nsp; e++) { by[2 * (size_t)sparse[e].rec] = sparse[e].all; by[2 * (size_t)sparse[e].rec + 1] = sparse[e].inf; }
        for (k = 0; k < c->np; k++) if (by[2 * (size_t)k]) { sparse[w].rec = k; sparse[w].all = by[2 * (size_t)k]; sparse[w].inf = by[2 * (size_t)k + 1]; w++; }
        free(by);
    } else qsort(sparse, (size_t)nsp, sizeof *sparse, tally_rec_cmp);
    qsort(hits, (size_t)nh, sizeof(sk_hit), hit_cmp);
    sp->rec = (uint32_t *)malloc(((size_t)nsp * 4 + 2) * sizeof(uint32_t));
    sp->all = sp->rec + nsp; sp->inf = sp->all + nsp; sp->hbeg = sp->inf + nsp;
    sp->rows = (uint32_t *)malloc(((size_t)nh + 1) * sizeof(uint32_t));
    for (e = 0; e < nsp; ) {                              /* (a record cut into pieces: the pieces' windows add up) */
        const uint32_t rec = c->prec[sparse[e].rec];
        uint32_t last = sparse[e].rec, all = 0, inf = 0, end;
        while (e < nsp && c->prec[sparse[e].rec] == rec) { all += sparse[e].all; inf += sparse[e].inf; last = sparse[e].rec; e++; }
        while (last + 1 < c->np && c->prec[last + 1] == rec) last++;              /* the record's last piece: its rows end where the next record begins */
        end = last + 1 < c->np ? c->pstart[last + 1] : 0xFFFFFFFFu;
        sp->rec[sp->n] = rec; sp->all[sp->n] = all; sp->inf[sp->n] = inf; sp->hbeg[sp->n] = n;
        while (h < nh && hits[h].pos < end) sp->rows[n++] = hits[h++].row;
        sp->n++;
    }
    sp->hbeg[sp->n] = n;
}

/* ---------------------------------------------------------------------------------------------
 * Lanes (round 4): the per-strain work behind a chunk's scan, off the main thread.
 *
 * Round 3's main thread did, chunk after chunk and one thing after the other: upload, launch, collect, then WAIT for the pool to
 * sort and spread the chunk's results strain by strain, then walk the read lengths, then WAIT for the pool to replay the
 * reference's read-after-read bookkeeping (and compress 32 outputs) -- 3.5-4.3 s of a 7-8 s pass over 100 Gbase x 32 strains,
 * beside 2.7-3.3 s of waiting for the decode side, which in turn waited for it (profiles/r03_cfg5_share.json).  The
 * reference's bookkeeping (src/strain_detect.c:443-626) is sequential per STRAIN, not across strains: strain s owns its carried
 * tallies, its copy of the last PE1 read's rows, its output.  So: L lane threads, strain s belongs to lane s mod L, and the main
 * thread only POSTS jobs -- "spread chunk c" (tally_one), "replay this run of read pairs" -- which every lane works off in the
 * order posted, for its own strains.  A lane's strains see the chunks and runs in file order, which is all the bookkeeping needs;
 * the main thread goes on to the next chunk's collection at once.  Chunks are reference-counted: a job holds the chunks it names.
 * Back-pressure: a lane's ring holds SD_RING jobs; the main thread waits when the slowest lane is that far behind.  At the end of
 * a file the main thread waits for the lanes to run dry (the trailer lines follow the last hit line), and reads the strains'
 * error states there.
 * ------------------------------------------------------------------------------------------- */
#define SD_LANES_MAX 16
#define SD_RING 8
enum { SD_JOB_TALLY, SD_JOB_REPLAY, SD_JOB_SYNC };
typedef struct sd_job {
    int kind;
    sd_chunk *ca, *cb;                         /* TALLY: ca; REPLAY: the run's chunks (cb may be NULL) */
    const char *f1;
    uint32_t a0, b0, astep, n, first_valid;
    int have_copy;
    int mute;                                  /* REPLAY: nothing is emitted, only the carried state moves on (a run the device counted) */
    uint64_t pair_base;                        /* REPLAY: the target's ordinal of the run's pair 0 (--coverage-rarefaction) */
    int pending;                               /* lanes that still have it (atomic) */
    sks_list *sup; int sup_sample;             /* REPLAY with --coverage-support: the run's emissions, a list per strain, and the target's sample */
} sd_job;
struct sd_lanes;
typedef struct sd_lane {
    pthread_t th; int started;
    pthread_mutex_t mu; pthread_cond_t cv_in, cv_out;
    sd_job *ring[SD_RING]; uint32_t head, count; int quit;
    struct sd_lanes *all; uint32_t id;
    double busy;                               /* (SK_SD_TIMING) */
} sd_lane;
typedef struct sd_lanes {
    sd_lane lane[SD_LANES_MAX]; uint32_t n, ns;
    sd_prog *p;
    pthread_mutex_t smu; pthread_cond_t scv; uint64_t syncs_done;     /* SYNC jobs completed */
} sd_lanes;
static sd_lanes sd_ln;
/* device calls of the main thread (uploads, launches, collections) and the one a lane can make (a hit line's k-mer fetched on the
 * spot, emit_rows) never run at the same time: a context takes one caller at a time */
static pthread_mutex_t sd_dev_mu = PTHREAD_MUTEX_INITIALIZER;
static double t_lane_busy, t_lane_backpressure, t_lane_drain;

static void sd_replay_run(sd_prog *p, uint32_t s, const char *f1, const sd_chunk *ca, uint32_t a0, const sd_chunk *cb, uint32_t b0,
                          uint32_t astep, uint32_t n, int have_copy_in, uint32_t first_valid, int mute, sks_list *sup, uint64_t pair_base);

/* --coverage-support[=FILE] [--support-pairs=FILE] (include/strainer_kmer.h has the rule): the read pairs behind the table's numbers.
 * A run the device folds is counted there (sk_covacc_set_support; the numbers come home at the target's end beside the sweep's);
 * a run replayed here records its emissions at sd_replay_run's emission site into the lists its job owns, and the last lane through
 * the job merges them across each group's strains (sks_merge, sk_host_support.c).  A pair is counted by one of the two and never by
 * both: a run is folded or replayed for ALL strains alike (sd_quantify decides per run, not per strain), the job of a folded run is
 * mute and owns no lists.  sk_host_support.c's entries are weak, as the device's are: host-only test builds link without that file,
 * and there the flag is refused. */
#pragma weak sks_create
#pragma weak sks_destroy
#pragma weak sks_sample
#pragma weak sks_list_push
#pragma weak sks_list_free
#pragma weak sks_merge
#pragma weak sks_add_device
#pragma weak sks_write_support
#pragma weak sks_write_pairs
static struct {
    int on; const char *pairs_path;
    sks_acc *acc; int sample;                  /* the run's numbers; the sample of the target being read */
    int failed;                                /* a merge ran out of memory (any lane) */
    double ms_take, ms_finish;                 /* SK_SD_TIMING */
} sd_sup;

static void lane_job_done(sd_lanes *L, sd_job *j)
{
    if (__atomic_sub_fetch(&j->pending, 1, __ATOMIC_ACQ_REL) > 0) return;
    if (j->kind == SD_JOB_SYNC) {
        pthread_mutex_lock(&L->smu);
        L->syncs_done++;
        pthread_cond_broadcast(&L->scv);
        pthread_mutex_unlock(&L->smu);
    }
    if (j->sup) {                                          /* every lane is through: the emissions of all strains are in */
        uint32_t s;
        assert(!j->mute);                                  /* (a run the device counted records nothing here) */
        if (sks_merge(sd_sup.acc, (uint32_t)j->sup_sample, j->sup)) __atomic_store_n(&sd_sup.failed, 1, __ATOMIC_RELAXED);
        for (s = 0; s < L->ns; s++) sks_list_free(&j->sup[s]);
        free(j->sup);
    }
    chunk_free(j->ca);
    chunk_free(j->cb);
    free(j);
}

static void *lane_main(void *arg)
{
    sd_lane *ln = (sd_lane *)arg;
    sd_lanes *L = ln->all;
    pthread_setname_np(pthread_self(), "sk-lane");
    for (;;) {
        sd_job *j;
        uint32_t s;
        pthread_mutex_lock(&ln->mu);
        while (ln->count == 0 && !ln->quit) pthread_cond_wait(&ln->cv_in, &ln->mu);
        if (ln->count == 0) {
            pthread_mutex_unlock(&ln->mu);
            pthread_mutex_lock(&t_pw_mu); cpu_lanes += thread_cpu_s(); pthread_mutex_unlock(&t_pw_mu);
            return NULL;
        }
        j = ln->ring[ln->head];
        pthread_mutex_unlock(&ln->mu);
        {
            const double t0 = now_s();
            for (s = ln->id; s < L->ns; s += L->n) {
                sd_prog *p = &L->p[s];
                if (j->kind == SD_JOB_TALLY) tally_one(p, j->ca, s);
                else if (j->kind == SD_JOB_REPLAY && p->job_rc == SK_OK)
                    sd_replay_run(p, s, j->f1, j->ca, j->a0, j->cb, j->b0, j->astep, j->n, j->have_copy, j->first_valid, j->mute, j->sup ? &j->sup[s] : NULL, j->pair_base);
            }
            ln->busy += now_s() - t0;
        }
        pthread_mutex_lock(&ln->mu);                  /* (the job leaves the ring only now: "ring empty" means "nothing in work") */
        ln->head = (ln->head + 1u) % SD_RING;
        ln->count--;
        pthread_cond_signal(&ln->cv_out);
        pthread_mutex_unlock(&ln->mu);
        lane_job_done(L, j);
    }
}

static void lanes_start(sd_prog *p, uint32_t ns)
{
    sd_lanes *L = &sd_ln;
    uint32_t want = getenv("SK_SD_LANES") ? (uint32_t)atoi(getenv("SK_SD_LANES")) : getenv("SK_THREADS") ? (uint32_t)atoi(getenv("SK_THREADS")) : 8u, i;
    memset(L, 0, sizeof *L);
    if (want < 1) want = 1;
    if (want > SD_LANES_MAX) want = SD_LANES_MAX;
    if (want > ns) want = ns;
    L->n = want; L->ns = ns; L->p = p;
    pthread_mutex_init(&L->smu, NULL);
    pthread_cond_init(&L->scv, NULL);
    for (i = 0; i < L->n; i++) {
        sd_lane *ln = &L->lane[i];
        ln->all = L; ln->id = i;
        pthread_mutex_init(&ln->mu, NULL);
        pthread_cond_init(&ln->cv_in, NULL);
        pthread_cond_init(&ln->cv_out, NULL);
        ln->started = pthread_create(&ln->th, NULL, lane_main, ln) == 0;
    }
}

/* hand a job to every lane (it takes over the caller's claims on ca and cb: pass chunks already chunk_ref'ed) */
static void lanes_post(sd_job *j)
{
    sd_lanes *L = &sd_ln;
    uint32_t i;
    j->pending = (int)L->n;
    for (i = 0; i < L->n; i++) {
        sd_lane *ln = &L->lane[i];
        if (!ln->started) {                               /* (no thread could be made for this lane: its strains are done here) */
            uint32_t s;
            for (s = ln->id; s < L->ns; s += L->n) {
                if (j->kind == SD_JOB_TALLY) tally_one(&L->p[s], j->ca, s);
                else if (j->kind == SD_JOB_REPLAY && L->p[s].job_rc == SK_OK)
                    sd_replay_run(&L->p[s], s, j->f1, j->ca, j->a0, j->cb, j->b0, j->astep, j->n, j->have_copy, j->first_valid, j->mute, j->sup ? &j->sup[s] : NULL, j->pair_base);
            }
            lane_job_done(L, j);
            continue;
        }
        pthread_mutex_lock(&ln->mu);
        if (ln->count == SD_RING) {
            const double t0 = now_s();
            while (ln->count == SD_RING) pthread_cond_wait(&ln->cv_out, &ln->mu);
            t_lane_backpressure += now_s() - t0;
        }
        ln->ring[(ln->head + ln->count) % SD_RING] = j;
        ln->count++;
        pthread_cond_signal(&ln->cv_in);
        pthread_mutex_unlock(&ln->mu);
    }
}

static sd_job *job_new(int kind, sd_chunk *ca, sd_chunk *cb)
{
    sd_job *j = (sd_job *)calloc(1, sizeof *j);
    j->kind = kind; j->ca = ca; j->cb = cb;
    chunk_ref(ca); chunk_ref(cb);
    return j;
}

/* wait until every lane has worked off everything posted so far */
static void lanes_drain(void)
{
    sd_lanes *L = &sd_ln;
    uint64_t want;
    if (!L->n) return;
    pthread_mutex_lock(&L->smu);
    want = L->syncs_done + 1;
    pthread_mutex_unlock(&L->smu);
    lanes_post(job_new(SD_JOB_SYNC, NULL, NULL));
    pthread_mutex_lock(&L->smu);
    while (L->syncs_done < want) pthread_cond_wait(&L->scv, &L->smu);
    pthread_mutex_unlock(&L->smu);
}

static void lanes_stop(void)
{
    sd_lanes *L = &sd_ln;
    uint32_t i;
    for (i = 0; i < L->n; i++) {
        sd_lane *ln = &L->lane[i];
        if (ln->started) {
            pthread_mutex_lock(&ln->mu);
            ln->quit = 1;
            pthread_cond_signal(&ln->cv_in);
            pthread_mutex_unlock(&ln->mu);
            pthread_join(ln->th, NULL);
        }
        t_lane_busy += ln->busy;
        pthread_mutex_destroy(&ln->mu);
        pthread_cond_destroy(&ln->cv_in);
        pthread_cond_destroy(&ln->cv_out);
    }
    if (L->n) { pthread_mutex_destroy(&L->smu); pthread_cond_destroy(&L->scv); }
    L->n = 0;
}

/* --coverage-background [--background-spectrum] [--background-max D] (include/strainer_kmer.h has the rule): every table above slices
 * the strain's INFORMATIVE k-mers; this one counts all of them.  With the flag a strain's table has one more column, SD_BGCOUNT, and
 * every batch of every file of a target is COUNT-scanned as it lies on the device (sk_scan_batch) right behind its TALLY launch, on
 * the same stream -- into that column strain by strain, or ONCE per union table into a count column of the union's own context.  The
 * TALLY scan cannot give this: it keeps the "all hits" count per read, not per row.  Where a target ends one sweep per strain or per
 * union (sk_background_finish, sk_union_background_finish) turns the column into the target's block and leaves it zero.  The entries
 * are weak, as the accumulators' are: the host-only test builds link this file without them, and there the flag fails the run. */
#pragma weak sk_scan_batch
#pragma weak sk_scan_timing
#pragma weak sk_union_scan_timing
#pragma weak sk_background_finish
#pragma weak sk_union_background_finish
#pragma weak sk_union_count_enable
#pragma weak sk_union_context
#pragma weak skb_create
#pragma weak skb_destroy
#pragma weak skb_add
#pragma weak skb_write
#pragma weak skb_write_spectrum
enum { SD_BGCOUNT = SD_NCOLS };
static struct { int on; uint32_t max; int failed; double ms_sweep; uint64_t scans; } sd_bg;
static uint32_t sd_ncols(void) { return sd_bg.on ? SD_NCOLS + 1u : SD_NCOLS; }
static const char *sd_bg_error;            /* the text of the context (a strain's, a union's) whose sweep failed */

/* Many strains on one device: one union table per group of up to SK_UNION_MAX strains (sk_union_*), so that a batch is
 * scanned once per group instead of once per strain (BASELINE configs[4]: 32 strains per GPU).  Built by sd_run when the
 * strains are open and flagged; a strain the union cannot hold (byte-string keys, no text stage), SK_SD_NO_UNION=1, or a
 * batch of 64 MiB or more (one huge record) leave the member-by-member way below, which gives the same results. */
static struct { sk_union **u; uint32_t n; sk_tally_rec *recs; uint64_t recs_cap; sk_hit *hits; uint64_t *hcap; } sd_un;

/* every scan that may still be in flight (a stream closed early with a chunk launched ahead): wait before its batch is freed */
static sd_prog *sd_all_p; static uint32_t sd_all_ns;
static void sd_drain_scans(void)
{
    uint32_t g, s;
    for (g = 0; g < sd_un.n; g++) sk_union_sync(sd_un.u[g]);
    for (s = 0; !sd_un.n && s < sd_all_ns; s++) if (sd_all_p[s].ctx) sk_sync(sd_all_p[s].ctx);
}

static void sd_unions_close(void)
{
    uint32_t g;
    for (g = 0; g < sd_un.n; g++) sk_union_destroy(sd_un.u[g]);
    free(sd_un.u); free(sd_un.recs); free(sd_un.hits); free(sd_un.hcap);
    memset(&sd_un, 0, sizeof sd_un);
}

static void sd_unions_open(sd_prog *p, uint32_t ns)
{
    uint32_t g, ng = (ns + sd_group - 1) / sd_group;
    const double t0 = now_s();
    memset(&sd_un, 0, sizeof sd_un);
    if (ns < 2 || getenv("SK_SD_NO_UNION")) return;
    sd_un.u = (sk_union **)calloc(ng, sizeof *sd_un.u);
    sd_un.hcap = (uint64_t *)calloc(ng, sizeof *sd_un.hcap);
    for (g = 0; g < ng; g++) {
        sk_ctx *m[SK_UNION_MAX];
        const uint32_t a = g * sd_group, n = ns - a < sd_group ? ns - a : sd_group;
        uint32_t k;
        int rc;
        for (k = 0; k < n; k++) m[k] = p[a + k].ctx;
        rc = sk_union_create(m, n, SD_TYPE, SD_INFORMATIVE, &sd_un.u[g]);
        if (rc == SK_OK && sd_bg.on && (rc = sk_union_count_enable(sd_un.u[g], 1)) != SK_OK) { sk_union_destroy(sd_un.u[g]); sd_un.u[g] = NULL; }
        if (rc != SK_OK) {
            if (getenv("SK_SD_TIMING")) fprintf(p[0].err, "strain_detect: no union table (%s: %s): strain by strain\n", sk_strerror(rc), sk_last_error(m[0]));
            sd_un.n = g;
            sd_unions_close();
            return;
        }
        sd_un.n = g + 1;
        sd_un.hcap[g] = 1u << 18;
    }
    if (getenv("SK_SD_TIMING")) fprintf(p[0].err, "strain_detect timing: %u union table(s) for %u strains in %.2f s\n", ng, ns, now_s() - t0);
}

/* ---------------------------------------------------------------------------------------------
 * --panel-share=FILE (-S only; include/strainer_kmer.h has the table): how many k-mers the strains of the panel share, every ordered
 * pair of them, from the masks the union tables carry -- sk_union_share(u[g], NULL) for every group, (u[g], u[h]) for every ordered
 * pair of groups -- before the first target is read.  The table depends on the strains alone.  The device's entry is weak, as the
 * accumulators' are: the host-only test builds link this file without it, and there the flag fails the run.
 * ------------------------------------------------------------------------------------------- */
#pragma weak sk_union_share
static struct { const char *path; double ms; unsigned calls; } sd_ps;

/* the coverage tables' strain_name: the -o file's basename without a trailing "<any>kmer_hits<any>gz" */
static char *sd_strain_name(const char *o_path)
{
    const char *b = strrchr(o_path, '/');
    char *n = strdup(b ? b + 1 : o_path);
    const size_t l = n ? strlen(n) : 0;
    if (l >= 13 && !memcmp(n + l - 12, "kmer_hits", 9) && !memcmp(n + l - 2, "gz", 2)) n[l - 13] = 0;
    return n;
}

static int sd_panel_share(sd_prog *p, uint32_t ns)
{
    const uint32_t M = SK_UNION_MAX, ng = (ns + sd_group - 1) / sd_group;
    const size_t cells = (size_t)3 * M * M;
    const double t0 = now_s();
    FILE *err = p[0].err, *f = NULL;
    sk_union *one = NULL, **u = sd_un.u;
    uint64_t *blk = NULL, *mat = NULL;
    char **name = NULL;
    uint32_t g, h, s, t;
    int rc = SK_OK, bad = 1;
    sd_ps.ms = 0; sd_ps.calls = 0;
    if (!sk_union_share) { fprintf(err, "strain_detect: --panel-share: this build has no sk_union_share\n"); return 1; }
    if (!sd_un.n && ns == 1 && !getenv("SK_SD_NO_UNION")) {          /* (a panel of one: a union for this table only) */
        if (sk_union_create(&p[0].ctx, 1, SD_TYPE, SD_INFORMATIVE, &one) == SK_OK) u = &one;
    }
    if (!u || (!one && sd_un.n != ng)) {
        fprintf(err, "strain_detect: --panel-share: the strains cannot all be held in union tables (a strain with byte-string keys or "
                     "without a text stage, a union that could not be built, or SK_SD_NO_UNION): no table of the panel\n");
        return 1;
    }
    blk = (uint64_t *)malloc(cells * sizeof *blk);
    mat = (uint64_t *)calloc((size_t)3 * ns * ns, sizeof *mat);
    name = (char **)calloc(ns, sizeof *name);
    for (s = 0; name && s < ns; s++) if (!(name[s] = sd_strain_name(p[s].o_path))) break;
    if (!blk || !mat || !name || s < ns) { fprintf(err, "strain_detect: out of memory\n"); goto out; }
    for (g = 0; g < ng; g++)
        for (h = 0; h < ng; h++) {
            const uint32_t a0 = g * sd_group, b0 = h * sd_group;
            const uint32_t na = ns - a0 < sd_group ? ns - a0 : sd_group, nb = ns - b0 < sd_group ? ns - b0 : sd_group;
            uint32_t k;
            if ((rc = sk_union_share(u[g], g == h ? NULL : u[h], blk)) != SK_OK) {
                fprintf(err, "strain_detect: --panel-share: device error: %s (%s)\n", sk_strerror(rc), sk_union_last_error(u[g]));
                goto out;
            }
            sd_ps.calls++;
            for (k = 0; k < 3; k++)
                for (s = 0; s < na; s++)
                    for (t = 0; t < nb; t++)
                        mat[((size_t)k * ns + a0 + s) * ns + b0 + t] = blk[((size_t)k * M + s) * M + t];
        }
    sd_ps.ms = (now_s() - t0) * 1e3;
    if (!(f = fopen(sd_ps.path, "w"))) { fprintf(err, "strain_detect: could not write %s\n", sd_ps.path); goto out; }
    fputs("strain_a\tstrain_b\tkmers_a\tinformative_a\tshared_kmers\tinformative_a_in_b\tinformative_both\n", f);
    for (s = 0; s < ns; s++)
        for (t = 0; t < ns; t++)
            fprintf(f, "%s\t%s\t%llu\t%llu\t%llu\t%llu\t%llu\n", name[s], name[t],
                    (unsigned long long)mat[(size_t)s * ns + s], (unsigned long long)mat[((size_t)ns + s) * ns + s],
                    (unsigned long long)mat[(size_t)s * ns + t], (unsigned long long)mat[((size_t)ns + s) * ns + t],
                    (unsigned long long)mat[((size_t)2 * ns + s) * ns + t]);
    bad = ferror(f) != 0;
    if (fclose(f)) bad = 1;
    if (bad) fprintf(err, "strain_detect: error writing %s\n", sd_ps.path);
out:
    sk_union_destroy(one);
    for (s = 0; name && s < ns; s++) free(name[s]);
    free(name); free(blk); free(mat);
    return bad;
}

/* while the device scans the current chunk: the next chunk of the stream's queue (if the reader is ahead) goes up into the
 * stream's other batch -- the upload of a 32 MiB chunk takes about twice as long as its scan against a union table */
static void sd_prefetch(sd_stream *st)
{
    sd_chunk *n = NULL;
    const double t0 = now_s();
    int d, ok = 1;
    if (!st) return;
    pthread_mutex_lock(&st->mu);
    if (st->qn > 0) n = st->q[0];                          /* (only this thread takes chunks off the queue: n stays) */
    pthread_mutex_unlock(&st->mu);
    if (!n || n == st->pre || (n->text ? n->text != SD_TEXT_PENDING : !n->np)) return;
    for (d = 0; d < sd_dev.n && ok; d++) {
        sk_batch **b = &st->bat[st->bcur ^ 1][d];
        if (!*b && sd_batch_get(d, b) != SK_OK) { *b = NULL; ok = 0; break; }
        if (n->text) ok = sk_batch_fill_text(*b, n->buf, n->tlen + (uint64_t)n->tla, n->t_eof) == SK_OK;     /* (a piece of text: upload + parse, enqueued) */
        else
        ok = (n->packed ? sk_batch_fill_packed(*b, n->buf, n->blen, n->pstart, n->np) : sk_batch_fill(*b, n->buf, n->blen, n->pstart, n->np)) == SK_OK;
        if (ok && d == 0) sd_tc_hand(st, n, *b);           /* (the target cache: packed behind this upload) */
    }
    if (ok) st->pre = n;                                   /* (all devices or none: a chunk that is not everywhere goes up again) */
    t_fill += now_s() - t0;
}

/* ---------------------------------------------------------------------------------------------
 * --coverage-only: step 4's table without the hit list (scripts/coverage_depth.py:62-129 over src/strain_detect.c:443-626).
 * One coverage accumulator (sk_covacc) per launch unit -- a union table's group of strains, or a strain -- on the unit's device.
 * A chunk all of whose records have k bases or more is counted where its scan left its results (sk_covacc_add): single reads
 * whole, interleaved pairs as far as both mates are in the chunk, two files when the PE1 chunk and the PE2 chunk hold the same
 * records (the PE1 chunk's results wait in the accumulator: sk_covacc_hold).  Of such a chunk only the results of its first and
 * its last three records come home (sk_covacc_pick): the last pair's tallies and rows are what a short read behind it would
 * repeat -- a muted replay of that pair carries them on -- and a pair that straddles two chunks is replayed as ever.  Every
 * other chunk is collected and replayed as without the flag, and emit_rows hands the passing pairs' rows to
 * sk_covacc_add_rows.  At a target's end sk_covacc_finish_target gives each strain's two numbers to its skc_acc.
 * ------------------------------------------------------------------------------------------- */
/* The device's entry points are weak, as the text parser's are: the host-only test builds link this file without them, and there
 * the flag counts every target on the host accumulator (co_open). */
#pragma weak sk_covacc_create
#pragma weak sk_covacc_destroy
#pragma weak sk_covacc_hold
#pragma weak sk_covacc_add
#pragma weak sk_covacc_add_rows
#pragma weak sk_covacc_finish_target
#pragma weak sk_covacc_pick
#pragma weak sk_covacc_fetch_hold
#pragma weak sk_tally_collect_counts
#pragma weak sk_union_tally_collect_counts
#pragma weak sk_union_tally_launch_ex
/* --coverage-regions (include/strainer_kmer.h has the rule): the strain's region table comes from its file (sk_host_regions.c), a
 * row's region from its first text position -- the key set's on the host, the table's own (sk_table_first_pos) for a key set built
 * on the device.  With --coverage-only the accumulators fold by region in the sweep that ends a target
 * (sk_covacc_finish_target_regions; replayed runs reach the same counters through sk_covacc_add_rows); with --coverage-depth, and
 * where --coverage-only counts on the host, skc_report_regions folds the host accumulator's (sample, row) list. */
#pragma weak skh_regions_from_file
#pragma weak skh_regions_free
#pragma weak sk_table_first_pos
#pragma weak sk_covacc_set_regions
#pragma weak sk_covacc_region_rows
#pragma weak sk_covacc_finish_target_regions
#pragma weak sk_covacc_timing_
/* --coverage-spectrum (include/strainer_kmer.h has the rule): with --coverage-only the sweep that ends a target also bins the
 * counters by depth (sk_covacc_finish_target_spectrum, with the region pairs when --coverage-regions is on too); with
 * --coverage-depth, and where --coverage-only counts on the host, skc_report_spectrum folds the host accumulator's list. */
#pragma weak sk_covacc_set_spectrum
#pragma weak sk_covacc_finish_target_spectrum
static struct { int on; uint32_t max; } sd_spec;
/* --coverage-thresholds [--threshold-list t1,t2,...] (include/strainer_kmer.h has the rule): with the accumulators on the device every
 * fold also classifies its entries by the list (sk_covacc_set_thresholds), replayed rows travel unfiltered with their pairs' totals
 * (sk_covacc_add_rows_hits) and a pass of its own in front of the target's sweep yields the numbers
 * (sk_covacc_finish_target_thresholds); with --coverage-depth, and where --coverage-only counts on the host, the host accumulator
 * keeps the lines above t[0] and skc_report_thresholds folds them. */
#pragma weak sk_covacc_set_thresholds
#pragma weak sk_covacc_add_rows_hits
#pragma weak sk_covacc_finish_target_thresholds
#pragma weak sk_covacc_thresholds_timing_
static struct { int on; uint32_t n; int64_t t[SK_COVACC_THRESHOLDS_MAX]; double ms_finish; } sd_thr;
/* --coverage-scrub-sweep [--scrub-classes FILE] (include/strainer_kmer.h has the rule): the run is made with the informative list of
 * the largest fraction; every strain's class file says in how many of the listed fractions' sets each informative k-mer is.  With the
 * accumulators on the device the classes go up once as one byte per row (sk_covacc_set_classes) and a pass of its own in front of the
 * target's sweep bins the non-zero rows by class (sk_covacc_finish_target_classes); with --coverage-depth, and where --coverage-only
 * counts on the host, skc_report_classes folds the host accumulator's list. */
/* --coverage-rarefaction [--rarefaction-list f0,f1,...] [--rarefaction-seed S] (include/strainer_kmer.h has the rule): every read pair
 * draws a number from its ordinal in the target, and the table gives step 4's numbers over the pairs below each listed fraction.  The
 * main loop of sd_quantify knows every run's first ordinal (the pairs of the runs before it); a chunk folded on the device gets the same
 * number from the records in front of it (co_collect), and the two are compared.  Folded runs are classified and their pairs counted on
 * the device (sk_covacc_set_pair_base in front of sk_covacc_add); a replayed run's lines travel with their ordinals
 * (sk_covacc_add_rows_hits_pairs) and its pairs are counted here; with --coverage-depth, and where --coverage-only counts on the host,
 * every strain keeps its rows' highest classes of the target being read.  sk_host_rarefaction.c has the parser, the class and the
 * table's lines. */
#pragma weak sk_covacc_set_rarefaction
#pragma weak sk_covacc_set_pair_base
#pragma weak sk_covacc_add_rows_hits_pairs
#pragma weak sk_covacc_finish_target_rarefaction
#pragma weak sk_covacc_rarefaction_timing_
#pragma weak skh_rarefaction_parse
#pragma weak skh_rarefaction_class
#pragma weak skh_rarefaction_write
static struct {
    int on, named;                              /* the flag; the lines begin with the strain's name (-S) */
    long long min;                              /* --min-kmer-hits */
    skh_rarefaction r;
    uint64_t host_pairs[SK_COVACC_RAREFACTION_MAX + 1];    /* the pairs of the target's replayed runs, by class */
    double ms_class, ms_finish;                 /* SK_SD_TIMING */
} sd_rar;
#pragma weak sk_covacc_set_classes
#pragma weak sk_covacc_finish_target_classes
#pragma weak sk_covacc_classes_timing_
#pragma weak sk_covacc_set_support
#pragma weak sk_covacc_finish_target_support
#pragma weak sk_covacc_support_timing_
static struct { int on; double ms_cls; } sd_sw;
/* --coverage-recurrence [--recurrence-pairs] (include/strainer_kmer.h has the rule): with the accumulators on the device every unit
 * has one set of bit planes (sk_recur) over the run's target lines; the end of a target sets the bits of its non-zero rows
 * (sk_covacc_mark_target, right before the sweep) and the end of the run takes both tables once (sk_recur_finish) and hands them to
 * the strains' skc_acc; with --coverage-depth, and where --coverage-only counts on the host, skc_report_recurrence folds the host
 * accumulator's list. */
#pragma weak sk_recur_create
#pragma weak sk_recur_destroy
#pragma weak sk_recur_finish
#pragma weak sk_recur_timing_
#pragma weak sk_covacc_set_recurrence
#pragma weak sk_covacc_mark_target
#pragma weak sk_covacc_mark_timing_
static struct {
    int on, pairs;
    uint32_t T;                                 /* the run's target lines */
    uint32_t next; char **name;                 /* the targets counted so far, and ordinal -> the target's path */
    sk_recur **r; uint32_t nr;                  /* one per unit, beside sd_co.acc */
    double ms_mark, ms_hist, ms_gram;           /* SK_SD_TIMING */
} sd_rec;
static double sd_co_ms_fold, sd_co_ms_sweep;          /* SK_SD_TIMING: the accumulators' device time, folds and target sweeps */
static struct {
    int on; uint64_t window;
    const char *const *genomes; uint32_t ngenomes;         /* the strain files of adopted strains (skh_resident_genomes_) */
} sd_rg;
void skh_resident_genomes_(const char *const *paths, uint32_t n) { sd_rg.genomes = paths; sd_rg.ngenomes = n; }

static int chunk_res_reserve(sd_chunk *c, uint64_t *rcap, uint64_t *hcap, uint64_t nrec_total, uint64_t nhit_total);
static struct {
    int on, host;                               /* the flag; every target through the host accumulator (two targets share a basename) */
    long long min;                              /* --min-kmer-hits */
    int mode; sd_stream *pe_a;                  /* the target being read: SD_*, and the PE1 stream of two files */
    sk_covacc **acc; uint32_t nacc;             /* one per unit; NULL: nothing is counted on the device */
    sk_tally_rec *recs; uint64_t rcap; sk_hit *hits; uint64_t hcap;    /* landing area of picks and fetched holds */
    uint64_t flush_rows;                        /* a strain's replayed rows go to the device when this many wait (SK_SD_CO_FLUSH_ROWS: tests) */
    sd_chunk *post;                             /* a PE1 chunk whose TALLY job waits for the device mutex to be let go */
} sd_co;
static uint64_t sd_co_dev, sd_co_replayed, sd_co_hostacc;
static uint64_t sd_res_bytes;                   /* scan results copied device to host by this run (SK_SD_RESULT_BYTES=1 prints it) */

void skh_coverage_only_stats(uint64_t *runs_on_device, uint64_t *runs_replayed, uint64_t *targets_host_accumulated, int reset)
{
    if (runs_on_device) *runs_on_device = sd_co_dev;
    if (runs_replayed) *runs_replayed = sd_co_replayed;
    if (targets_host_accumulated) *targets_host_accumulated = sd_co_hostacc;
    if (reset) sd_co_dev = sd_co_replayed = sd_co_hostacc = 0;
}

static uint32_t co_units(uint32_t ns) { return sd_un.n ? sd_un.n : ns; }
static uint32_t co_unit_first(uint32_t unit) { return sd_un.n ? unit * sd_group : unit; }
static uint32_t co_unit_members(uint32_t unit) { return sd_un.n ? sk_union_members(sd_un.u[unit]) : 1u; }

static void co_close(void)
{
    uint32_t k;
    for (k = 0; k < sd_co.nacc; k++) {
        double f = 0, w = 0;
        if (sk_covacc_timing_ && sd_co.acc[k] && sk_covacc_timing_(sd_co.acc[k], 0, &f, &w) == SK_OK) { sd_co_ms_fold += f; sd_co_ms_sweep += w; }
        if (sd_rec.on && sk_covacc_mark_timing_ && sd_co.acc[k] && sk_covacc_mark_timing_(sd_co.acc[k], &f) == SK_OK) sd_rec.ms_mark += f;
        if (sd_thr.on && sk_covacc_thresholds_timing_ && sd_co.acc[k] && sk_covacc_thresholds_timing_(sd_co.acc[k], &f) == SK_OK) sd_thr.ms_finish += f;
        if (sd_sw.on && sk_covacc_classes_timing_ && sd_co.acc[k] && sk_covacc_classes_timing_(sd_co.acc[k], &f) == SK_OK) sd_sw.ms_cls += f;
        if (sd_sup.on && sk_covacc_support_timing_ && sd_co.acc[k] && sk_covacc_support_timing_(sd_co.acc[k], &f, &w) == SK_OK) { sd_sup.ms_take += f; sd_sup.ms_finish += w; }
        if (sd_rar.on && sk_covacc_rarefaction_timing_ && sd_co.acc[k] && sk_covacc_rarefaction_timing_(sd_co.acc[k], &f, &w) == SK_OK) { sd_rar.ms_class += f; sd_rar.ms_finish += w; }
        if (sk_covacc_destroy) sk_covacc_destroy(sd_co.acc[k]);
    }
    for (k = 0; k < sd_rec.nr; k++) {
        double f = 0, w = 0;
        if (sk_recur_timing_ && sd_rec.r[k] && sk_recur_timing_(sd_rec.r[k], 0, &f, &w) == SK_OK) { sd_rec.ms_hist += f; sd_rec.ms_gram += w; }
        if (sk_recur_destroy) sk_recur_destroy(sd_rec.r[k]);
    }
    for (k = 0; sd_rec.name && k < sd_rec.T; k++) free(sd_rec.name[k]);
    free(sd_rec.r); free(sd_rec.name);
    sd_rec.r = NULL; sd_rec.nr = 0; sd_rec.name = NULL; sd_rec.next = 0;
    free(sd_co.acc); free(sd_co.recs); free(sd_co.hits);
    sd_co.acc = NULL; sd_co.nacc = 0; sd_co.recs = NULL; sd_co.hits = NULL; sd_co.rcap = sd_co.hcap = 0; sd_co.post = NULL;
}

static int co_open(sd_prog *p, uint32_t ns)
{
    const uint32_t nu = co_units(ns);
    uint32_t k, m;
    if (!sd_co.on || sd_co.host) return SK_OK;
    if (!sk_covacc_create || !sk_covacc_pick || !sk_tally_collect_counts || !sk_union_tally_launch_ex ||
        (sd_rg.on && (!sk_covacc_set_regions || !sk_covacc_region_rows || !sk_covacc_finish_target_regions)) ||
        (sd_spec.on && (!sk_covacc_set_spectrum || !sk_covacc_finish_target_spectrum)) ||
        (sd_thr.on && (!sk_covacc_set_thresholds || !sk_covacc_add_rows_hits || !sk_covacc_finish_target_thresholds)) ||
        (sd_sw.on && (!sk_covacc_set_classes || !sk_covacc_finish_target_classes)) ||
        (sd_sup.on && (!sk_covacc_set_support || !sk_covacc_finish_target_support)) ||
        (sd_rar.on && (!sk_covacc_set_rarefaction || !sk_covacc_set_pair_base || !sk_covacc_add_rows_hits_pairs || !sk_covacc_finish_target_rarefaction)) ||
        (sd_rec.on && (!sk_recur_create || !sk_recur_finish || !sk_covacc_set_recurrence || !sk_covacc_mark_target))) {
        fprintf(p[0].err, "strain_detect: --coverage-only: this build has no coverage accumulator on the device: this run is counted on the host\n");
        sd_co.host = 1;
        return SK_OK;
    }
    sd_co.acc = (sk_covacc **)calloc(nu, sizeof *sd_co.acc);
    if (!sd_co.acc) return SK_E_NOMEM;
    if (sd_rec.on) {
        sd_rec.r = (sk_recur **)calloc(nu, sizeof *sd_rec.r);
        sd_rec.name = (char **)calloc(sd_rec.T ? sd_rec.T : 1u, sizeof *sd_rec.name);
        if (!sd_rec.r || !sd_rec.name) { co_close(); return SK_E_NOMEM; }
    }
    for (k = 0; k < nu; k++) {
        const uint32_t a = co_unit_first(k), n = co_unit_members(k);
        uint32_t nrows[SK_UNION_MAX];
        int rc;
        for (m = 0; m < n; m++) nrows[m] = (uint32_t)p[a + m].ks.nrows;
        rc = sk_covacc_create(p[a].ctx, n, nrows, (int64_t)sd_co.min, &sd_co.acc[k]);
        sd_co.nacc = k + 1;
        if (rc != SK_OK) { sd_co.nacc = k; co_close(); return rc; }
        if (getenv("SK_SD_TIMING") && sk_covacc_timing_) (void)sk_covacc_timing_(sd_co.acc[k], 1, NULL, NULL);
        if (sd_spec.on && (rc = sk_covacc_set_spectrum(sd_co.acc[k], sd_spec.max)) != SK_OK) { co_close(); return rc; }
        if (sd_thr.on && (rc = sk_covacc_set_thresholds(sd_co.acc[k], sd_thr.t, sd_thr.n)) != SK_OK) { co_close(); return rc; }
        if (sd_sup.on && (rc = sk_covacc_set_support(sd_co.acc[k], 1)) != SK_OK) { co_close(); return rc; }
        if (sd_rar.on && (rc = sk_covacc_set_rarefaction(sd_co.acc[k], sd_rar.r.T, sd_rar.r.n, sd_rar.r.seed)) != SK_OK) { co_close(); return rc; }
        for (m = 0; m < n && sd_sw.on; m++) {             /* every member's class bytes, from its class file's k-mers */
            const sd_prog *q = &p[a + m];
            uint8_t one = 0;
            rc = sk_covacc_set_classes(sd_co.acc[k], m, q->sw_rows, q->sw_c.n ? q->sw_c.cls : &one, q->sw_c.n, q->sw_c.F);
            if (rc != SK_OK) { co_close(); return rc; }
        }
        if (sd_rec.on) {                                  /* every member's informative rows ranked: its bits of the unit's planes */
            uint32_t nbits[SK_UNION_MAX];
            for (m = 0; m < n; m++) {
                if ((rc = sk_covacc_set_recurrence(sd_co.acc[k], m, p[a + m].ctx, SD_TYPE, SD_INFORMATIVE, &nbits[m])) != SK_OK) { co_close(); return rc; }
                if ((uint64_t)nbits[m] != (uint64_t)p[a + m].genome_inf) {
                    fprintf(p[0].err, "strain_detect: --coverage-recurrence: the table of strain %u has %u informative rows, its trailer says %llu\n",
                            a + m, nbits[m], (unsigned long long)p[a + m].genome_inf);
                    co_close();
                    return SK_E_STATE;
                }
            }
            rc = sk_recur_create(p[a].ctx, n, nbits, sd_rec.T, &sd_rec.r[k]);
            sd_rec.nr = k + 1;
            if (rc != SK_OK) { sd_rec.nr = k; co_close(); return rc; }
            if (getenv("SK_SD_TIMING") && sk_recur_timing_) (void)sk_recur_timing_(sd_rec.r[k], 1, NULL, NULL);
        }
        for (m = 0; m < n && sd_rg.on; m++) {             /* every member's rows to their regions, and the regions' denominators */
            sd_prog *q = &p[a + m];
            uint32_t *starts = (uint32_t *)malloc(((size_t)q->rg.n + 1) * sizeof *starts), r;
            uint64_t *rows = (uint64_t *)malloc(((size_t)q->rg.n + 1) * sizeof *rows);
            if (!starts || !rows) { free(starts); free(rows); co_close(); return SK_E_NOMEM; }
            for (r = 0; r < q->rg.n; r++) starts[r] = q->rg.text_off[r] < 0xFFFFFFFEull ? (uint32_t)q->rg.text_off[r] : 0xFFFFFFFEu;   /* (no row starts that far out) */
            rc = sk_covacc_set_regions(sd_co.acc[k], m, q->ctx, starts, q->rg.n);
            if (rc == SK_OK) rc = sk_covacc_region_rows(sd_co.acc[k], m, q->ctx, SD_TYPE, SD_INFORMATIVE, rows, q->reg_inf);
            free(starts); free(rows);
            if (rc != SK_OK) { co_close(); return rc; }
        }
    }
    return SK_OK;
}

/* every record of the chunk has k bases or more and is one record of its batch */
static int co_chunk_clean(const sd_chunk *c)
{
    uint32_t i;
    if (!c->np || c->np != c->nrec) return 0;
    if (c->text) return c->t_reads == c->nrec;
    for (i = 0; i < c->np; i++) if (c->prec[i] != i) return 0;
    return 1;
}

/* the rows of a replayed, passing pair wait here for the device (a lane's strain; the main thread at a target's end) */
static void co_flush(sd_prog *p, uint32_t s)
{
    const uint32_t unit = sd_un.n ? s / sd_group : s;
    int rc;
    if (!p->co_n) return;
    pthread_mutex_lock(&sd_dev_mu);
    rc = sd_rar.on ? sk_covacc_add_rows_hits_pairs(sd_co.acc[unit], s - co_unit_first(unit), p->co_rows, p->co_tot, p->co_pair, p->co_n) :
         sd_thr.on ? sk_covacc_add_rows_hits(sd_co.acc[unit], s - co_unit_first(unit), p->co_rows, p->co_tot, p->co_n)
                   : sk_covacc_add_rows(sd_co.acc[unit], s - co_unit_first(unit), p->co_rows, p->co_n);
    pthread_mutex_unlock(&sd_dev_mu);
    p->co_n = 0;
    if (rc != SK_OK) p->job_rc = rc;
}

enum { CO_PICK, CO_PICK_HOLD, CO_HOLD_ALL };
/* c->res_*: a few records' results of the unit's launches (CO_PICK), of the launches held (CO_PICK_HOLD), or the held launches'
 * results in full (CO_HOLD_ALL), dealt to the strains as sd_collect deals a chunk's */
static int co_deal(uint32_t ns, sd_prog *p, sd_chunk *c, int src, int first, uint32_t ntail)
{
    const uint32_t nu = co_units(ns);
    uint64_t rcap = 0, hcap = 0, nr = 0, nhit = 0, e;
    uint32_t k, s;
    int rc;
    free(c->res_off);
    c->res_off = (uint64_t *)calloc(2 * ((size_t)ns + 1), sizeof(uint64_t));
    if (!c->res_off) return SK_E_NOMEM;
    c->res_hoff = c->res_off + ns + 1;
    for (k = 0; k < nu; k++) {
        const uint32_t a = co_unit_first(k), n = co_unit_members(k);
        uint64_t nsp = 0, nh = 0, cnt[SK_UNION_MAX + 1], hcnt[SK_UNION_MAX + 1];
        for (;;) {
            if (!sd_co.recs) { sd_co.rcap = 4096; sd_co.recs = (sk_tally_rec *)malloc((size_t)sd_co.rcap * sizeof *sd_co.recs); }
            if (!sd_co.hits) { sd_co.hcap = 1u << 16; sd_co.hits = (sk_hit *)malloc((size_t)sd_co.hcap * sizeof *sd_co.hits); }
            if (!sd_co.recs || !sd_co.hits) return SK_E_NOMEM;
            if (src == CO_HOLD_ALL) rc = sk_covacc_fetch_hold(sd_co.acc[k], sd_co.recs, sd_co.rcap, &nsp, sd_co.hits, sd_co.hcap, &nh);
            else rc = sk_covacc_pick(sd_co.acc[k], src == CO_PICK && !sd_un.n ? p[a].ctx : NULL, src == CO_PICK && sd_un.n ? sd_un.u[k] : NULL,
                                     src == CO_PICK_HOLD, first, ntail, sd_co.recs, sd_co.rcap, &nsp, sd_co.hits, sd_co.hcap, &nh);
            if (rc != SK_OK) return rc;
            if (nsp <= sd_co.rcap && nh <= sd_co.hcap) break;
            if (nsp > sd_co.rcap) { free(sd_co.recs); sd_co.recs = NULL; sd_co.rcap = nsp + nsp / 4; sd_co.recs = (sk_tally_rec *)malloc((size_t)sd_co.rcap * sizeof *sd_co.recs); }
            if (nh > sd_co.hcap) { free(sd_co.hits); sd_co.hits = NULL; sd_co.hcap = nh + nh / 4; sd_co.hits = (sk_hit *)malloc((size_t)sd_co.hcap * sizeof *sd_co.hits); }
        }
        sd_res_bytes += nsp * sizeof(sk_tally_rec) + nh * sizeof(sk_hit) + 8;
        if ((rc = chunk_res_reserve(c, &rcap, &hcap, nr + nsp, nhit + nh)) != SK_OK) return rc;
        if (!sd_un.n) {
            memcpy(c->res_recs + nr, sd_co.recs, (size_t)nsp * sizeof(sk_tally_rec));
            memcpy(c->res_hits + nhit, sd_co.hits, (size_t)nh * sizeof(sk_hit));
            c->res_off[a] = nr; c->res_hoff[a] = nhit;
            nr += nsp; nhit += nh;
            continue;
        }
        memset(cnt, 0, sizeof cnt); memset(hcnt, 0, sizeof hcnt);
        for (e = 0; e < nsp; e++) cnt[sd_co.recs[e].rec % n]++;
        for (e = 0; e < nh; e++) hcnt[sd_co.hits[e].row >> SK_UNION_ROW_BITS]++;
        for (s = 0; s < n; s++) {
            c->res_off[a + s] = nr; c->res_hoff[a + s] = nhit;
            nr += cnt[s]; nhit += hcnt[s];
            cnt[s] = c->res_off[a + s]; hcnt[s] = c->res_hoff[a + s];
        }
        for (e = 0; e < nsp; e++) {
            sk_tally_rec *out = c->res_recs + cnt[sd_co.recs[e].rec % n]++;
            out->rec = sd_co.recs[e].rec / n; out->all = sd_co.recs[e].all; out->inf = sd_co.recs[e].inf;
        }
        for (e = 0; e < nh; e++) {
            sk_hit *out = c->res_hits + hcnt[sd_co.hits[e].row >> SK_UNION_ROW_BITS]++;
            out->pos = sd_co.hits[e].pos; out->row = sd_co.hits[e].row & ((1u << SK_UNION_ROW_BITS) - 1u);
        }
    }
    c->res_off[ns] = nr; c->res_hoff[ns] = nhit;
    return SK_OK;
}

enum { CO_PLAN_NONE, CO_PLAN_SELF, CO_PLAN_HOLD, CO_PLAN_MATE };
static int co_plan(const sd_stream *st, const sd_chunk *c)
{
    if (!sd_co.acc || !st || !co_chunk_clean(c)) return CO_PLAN_NONE;
    if (sd_co.mode != SD_PE) return CO_PLAN_SELF;
    if (st == sd_co.pe_a) return CO_PLAN_HOLD;
    {
        const sd_stream *A = sd_co.pe_a;
        return A && A->c && A->c->co == SD_CO_HELD && A->ci == 0 && A->c->nrec == c->nrec ? CO_PLAN_MATE : CO_PLAN_NONE;
    }
}

/* the chunk's launches are in flight and its plan is to count it on the device: only the counters come home, then the picks */
static int co_collect(sd_prog *p, uint32_t ns, sk_batch **batches, sd_chunk *c, int plan)
{
    const uint32_t nu = co_units(ns);
    uint32_t k;
    int rc;
    for (k = 0; k < nu; k++) {
        const uint32_t a = co_unit_first(k);
        sk_union *u = sd_un.n ? sd_un.u[k] : NULL;
        sk_ctx *ctx = u ? NULL : p[a].ctx;
        uint64_t nsp = 0, nh = 0;
        for (;;) {
            uint64_t *cap = u ? &sd_un.hcap[k] : &p[a].hitcap;
            if ((rc = u ? sk_union_tally_collect_counts(u, &nsp, &nh) : sk_tally_collect_counts(ctx, &nsp, &nh)) != SK_OK) return rc;
            sd_res_bytes += 24;
            if (nh <= *cap) break;
            *cap = nh + nh / 4;                                 /* the log overflowed: once more with room */
            if (!u) p[a].hitbuf = (sk_hit *)realloc(p[a].hitbuf, (size_t)p[a].hitcap * sizeof(sk_hit));
            rc = u ? sk_union_tally_launch_ex(u, batches[sd_dev_of_strain(a)], *cap, 1) : sk_tally_launch(ctx, batches[sd_dev_of_strain(a)], SD_TYPE, SD_INFORMATIVE, *cap);
            if (rc != SK_OK) return rc;
        }
        if (sd_rar.on && plan != CO_PLAN_HOLD) {             /* the ordinal of the run's pair 0: PE the PE1 chunk's first record, PEI two records a pair */
            c->co_base = plan == CO_PLAN_MATE ? sd_co.pe_a->c->rec0 : sd_co.mode == SD_PEI ? (c->rec0 + c->co_a0) / 2 : c->rec0;
            if (plan == CO_PLAN_MATE) sd_co.pe_a->c->co_base = c->co_base;
            if ((rc = sk_covacc_set_pair_base(sd_co.acc[k], c->co_base)) != SK_OK) return rc;
        }
        if (plan == CO_PLAN_HOLD) rc = sk_covacc_hold(sd_co.acc[k], ctx, u);
        else if (plan == CO_PLAN_MATE) {
            const sk_covacc_mate mate = { 1, 0, 1 };
            rc = sk_covacc_add(sd_co.acc[k], ctx, u, 0, 0, 1, c->nrec, &mate);
        } else if (sd_co.mode == SD_PEI) {
            const sk_covacc_mate mate = { 0, c->co_a0 + 1, 2 };
            const uint32_t npairs = c->nrec > c->co_a0 ? (c->nrec - c->co_a0) / 2 : 0;
            rc = npairs ? sk_covacc_add(sd_co.acc[k], ctx, u, 0, c->co_a0, 2, npairs, &mate) : SK_OK;
        } else rc = sk_covacc_add(sd_co.acc[k], ctx, u, 0, 0, 1, c->nrec, NULL);
        if (rc != SK_OK) return rc;
    }
    if (plan == CO_PLAN_HOLD) { c->co = SD_CO_HELD; return SK_OK; }
    if ((rc = co_deal(ns, p, c, CO_PICK, c->co_a0 == 1, 3)) != SK_OK) return rc;
    c->co = SD_CO_FOLDED;
    if (plan == CO_PLAN_MATE) {
        sd_chunk *ca = sd_co.pe_a->c;
        if ((rc = co_deal(ns, p, ca, CO_PICK_HOLD, 0, 3)) != SK_OK) return rc;
        ca->co = SD_CO_FOLDED;
        sd_co.post = ca;
    }
    return SK_OK;
}

/* a held PE1 chunk that does not fold with its mates' chunk after all: its results come home in full, and it goes the usual way */
static int co_materialise(sd_prog *p, uint32_t ns, sd_chunk *c)
{
    int rc;
    pthread_mutex_lock(&sd_dev_mu);
    rc = co_deal(ns, p, c, CO_HOLD_ALL, 0, 0);
    pthread_mutex_unlock(&sd_dev_mu);
    if (rc != SK_OK) return rc;
    c->co = SD_CO_NONE;
    lanes_post(job_new(SD_JOB_TALLY, c, NULL));
    return SK_OK;
}

/* start the scans of one uploaded chunk: against every union table, or strain by strain (they overlap on the devices) */
/* --coverage-background: the COUNT scans of the chunk, each on the stream of the TALLY launch just made on the same batch and so
 * done when that launch has been collected -- before the batch is refilled.  Made once per chunk, here and nowhere else: a launch
 * that is repeated with more room for its log (sd_collect, co_collect) counts nothing again.  A failure stays: a chunk whose count
 * scans started only in part is never launched again as if nothing had been counted. */
static int sd_background_scans(sd_prog *p, uint32_t ns, sk_batch **batches)
{
    uint32_t g, s;
    if (sd_bg.failed) return sd_bg.failed;
    for (g = 0; g < sd_un.n && !sd_bg.failed; g++, sd_bg.scans++)
        sd_bg.failed = sk_scan_batch(sk_union_context(sd_un.u[g]), batches[sd_dev_of_strain(g * sd_group)], 0);
    for (s = 0; !sd_un.n && s < ns && !sd_bg.failed; s++, sd_bg.scans++)
        sd_bg.failed = sk_scan_batch(p[s].ctx, batches[sd_dev_of_strain(s)], SD_BGCOUNT);
    return sd_bg.failed;
}

static int sd_launch(sd_prog *p, uint32_t ns, sk_batch **batches)
{
    uint32_t g, s;
    int rc;
    if (sd_bg.on && sd_bg.failed) return sd_bg.failed;
    if (sd_un.n) {
        for (g = 0; g < sd_un.n; g++)
            if ((rc = sd_co.acc ? sk_union_tally_launch_ex(sd_un.u[g], batches[sd_dev_of_strain(g * sd_group)], sd_un.hcap[g], 1)
                                : sk_union_tally_launch(sd_un.u[g], batches[sd_dev_of_strain(g * sd_group)], sd_un.hcap[g])) != SK_OK) return rc;
        return sd_bg.on ? sd_background_scans(p, ns, batches) : SK_OK;
    }
    for (s = 0; s < ns; s++) {
        if (p[s].hitcap == 0) { p[s].hitcap = 1u << 16; p[s].hitbuf = (sk_hit *)malloc((size_t)p[s].hitcap * sizeof(sk_hit)); }
        if ((rc = sk_tally_launch(p[s].ctx, batches[sd_dev_of_strain(s)], SD_TYPE, SD_INFORMATIVE, p[s].hitcap)) != SK_OK) return rc;
    }
    return sd_bg.on ? sd_background_scans(p, ns, batches) : SK_OK;
}

/* room for n more records and m more log entries in the chunk's own result arrays */
static int chunk_res_reserve(sd_chunk *c, uint64_t *rcap, uint64_t *hcap, uint64_t nrec_total, uint64_t nhit_total)
{
    if (nrec_total > *rcap || !c->res_recs) {
        *rcap = nrec_total + nrec_total / 2 + 256;
        c->res_recs = (sk_tally_rec *)realloc(c->res_recs, (size_t)*rcap * sizeof(sk_tally_rec));
    }
    if (nhit_total > *hcap || !c->res_hits) {
        *hcap = nhit_total + nhit_total / 2 + 256;
        c->res_hits = (sk_hit *)realloc(c->res_hits, (size_t)*hcap * sizeof(sk_hit));
    }
    return c->res_recs && c->res_hits ? SK_OK : SK_E_NOMEM;
}


/* The results of the chunk whose scans are in flight, collected and laid out strain by strain IN THE CHUNK (res_recs/res_off,
 * res_hits/res_hoff) -- from the union tables (every group's results dealt to its members by a counting sort), or member by
 * member.  After this the device side may be overwritten by the next launch, and the lanes take it from here. */
static int sd_collect(sd_prog *p, uint32_t ns, sk_batch **batches, sd_chunk *c, const sd_stream *st)
{
    uint32_t g, s;
    int rc;
    uint64_t rcap = 0, hcap = 0, nr = 0, nhit = 0;
    if ((rc = co_plan(st, c)) != CO_PLAN_NONE) return co_collect(p, ns, batches, c, rc);
    c->res_off = (uint64_t *)calloc(2 * ((size_t)ns + 1), sizeof(uint64_t));
    if (!c->res_off) return SK_E_NOMEM;
    c->res_hoff = c->res_off + ns + 1;
    if (!sd_un.n) {
        for (s = 0; s < ns; s++) {
            uint64_t nsp = 0, nh = 0;
            if (p[s].tallycap < c->np || !p[s].tallybuf) {
                p[s].tallycap = c->np + c->np / 4 + 1024;
                p[s].tallybuf = (uint32_t *)realloc(p[s].tallybuf, (size_t)p[s].tallycap * sizeof(sk_tally_rec));
            }
            if ((rc = sk_tally_collect_sparse(p[s].ctx, (sk_tally_rec *)p[s].tallybuf, c->np, &nsp, p[s].hitbuf, &nh)) != SK_OK) return rc;
            if (nh > p[s].hitcap) {                           /* the log overflowed: once more with room */
                p[s].hitcap = nh + nh / 4;
                p[s].hitbuf = (sk_hit *)realloc(p[s].hitbuf, (size_t)p[s].hitcap * sizeof(sk_hit));
                if ((rc = sk_tally_launch(p[s].ctx, batches[sd_dev_of_strain(s)], SD_TYPE, SD_INFORMATIVE, p[s].hitcap)) != SK_OK ||
                    (rc = sk_tally_collect_sparse(p[s].ctx, (sk_tally_rec *)p[s].tallybuf, c->np, &nsp, p[s].hitbuf, &nh)) != SK_OK) return rc;
            }
            sd_res_bytes += 16 + nsp * sizeof(sk_tally_rec) + nh * sizeof(sk_hit);
            if ((rc = chunk_res_reserve(c, &rcap, &hcap, nr + nsp, nhit + nh)) != SK_OK) return rc;
            memcpy(c->res_recs + nr, p[s].tallybuf, (size_t)nsp * sizeof(sk_tally_rec));
            memcpy(c->res_hits + nhit, p[s].hitbuf, (size_t)nh * sizeof(sk_hit));
            c->res_off[s] = nr; c->res_hoff[s] = nhit;
            nr += nsp; nhit += nh;
        }
        c->res_off[ns] = nr; c->res_hoff[ns] = nhit;
        return SK_OK;
    }
    for (g = 0; g < sd_un.n; g++) {
        const uint32_t a = g * sd_group, n = sk_union_members(sd_un.u[g]);
        const uint64_t worst = (uint64_t)c->np * n;
        uint64_t nsp = 0, nh = 0, e;
        uint64_t cnt[SK_UNION_MAX + 1], hcnt[SK_UNION_MAX + 1];
        if (worst > sd_un.recs_cap) {                       /* (address space only: pages are touched as far as results come back) */
            free(sd_un.recs);
            sd_un.recs_cap = worst + worst / 4 + 1024;
            sd_un.recs = (sk_tally_rec *)malloc((size_t)sd_un.recs_cap * sizeof *sd_un.recs);
        }
        for (;;) {
            sd_un.hits = (sk_hit *)realloc(sd_un.hits, (size_t)sd_un.hcap[g] * sizeof(sk_hit));
            if ((rc = sk_union_tally_collect(sd_un.u[g], sd_un.recs, sd_un.recs_cap, &nsp, sd_un.hits, &nh)) != SK_OK) return rc;
            if (nh <= sd_un.hcap[g]) break;
            sd_un.hcap[g] = nh + nh / 4;                    /* the log overflowed: once more with room */
            if ((rc = sd_co.acc ? sk_union_tally_launch_ex(sd_un.u[g], batches[sd_dev_of_strain(a)], sd_un.hcap[g], 1)
                                : sk_union_tally_launch(sd_un.u[g], batches[sd_dev_of_strain(a)], sd_un.hcap[g])) != SK_OK) return rc;
        }
        sd_res_bytes += 24 + nsp * sizeof(sk_tally_rec) + nh * sizeof(sk_hit);
        if ((rc = chunk_res_reserve(c, &rcap, &hcap, nr + nsp, nhit + nh)) != SK_OK) return rc;
        memset(cnt, 0, sizeof cnt); memset(hcnt, 0, sizeof hcnt);
        for (e = 0; e < nsp; e++) cnt[sd_un.recs[e].rec % n]++;
        for (e = 0; e < nh; e++) hcnt[sd_un.hits[e].row >> SK_UNION_ROW_BITS]++;
        for (s = 0; s < n; s++) {                           /* the members' shares, one behind the other */
            c->res_off[a + s] = nr; c->res_hoff[a + s] = nhit;
            nr += cnt[s]; nhit += hcnt[s];
            cnt[s] = c->res_off[a + s]; hcnt[s] = c->res_hoff[a + s];      /* (now: where the member's next entry goes) */
        }
        for (e = 0; e < nsp; e++) {
            sk_tally_rec *out = c->res_recs + cnt[sd_un.recs[e].rec % n]++;
            out->rec = sd_un.recs[e].rec / n; out->all = sd_un.recs[e].all; out->inf = sd_un.recs[e].inf;
        }
        for (e = 0; e < nh; e++) {
            sk_hit *out = c->res_hits + hcnt[sd_un.hits[e].row >> SK_UNION_ROW_BITS]++;
            out->pos = sd_un.hits[e].pos; out->row = sd_un.hits[e].row & ((1u << SK_UNION_ROW_BITS) - 1u);
        }
    }
    c->res_off[ns] = nr; c->res_hoff[ns] = nhit;
    return SK_OK;
}

/* A piece of text whose turn has come (or whose scan is to be started ahead): wait for the device's parse in `batches` (begun: it was
 * sent up ahead) and, if the device took exactly the piece, fill in what the host walk needs from the record starts -- the batch
 * holds EVERY record, short and empty ones included, so the records of the scan are the records of the file (prec is the
 * identity) and len[i] is the distance of two starts less the '\n'.  A record shorter than k has no window: it tallies nothing.
 * 1 accepted, 0 declined (c->text says so), < 0 device error. */
static int sd_text_resolve(sd_stream *st, sd_chunk *c, sk_batch **batches, int begun)
{
    sk_text_info info[SD_MAX_DEV];
    const uint32_t *starts = NULL;
    int d, rc = SK_OK, ok = 1;
    uint32_t i, n;
    if (c->text != SD_TEXT_PENDING) return c->text == SD_TEXT_ACCEPTED;
    pthread_mutex_lock(&sd_dev_mu);
    for (d = 0; d < sd_dev.n && !begun && rc == SK_OK; d++) rc = sk_batch_fill_text(batches[d], c->buf, c->tlen + (uint64_t)c->tla, c->t_eof);
    for (d = 0; d < sd_dev.n && rc == SK_OK; d++) rc = sk_batch_text_finish(batches[d], &info[d], d == 0 ? &starts : NULL);
    pthread_mutex_unlock(&sd_dev_mu);
    if (rc != SK_OK) return rc;
    for (d = 0; d < sd_dev.n; d++)
        ok = ok && info[d].status == SK_TEXT_OK && info[d].consumed == c->tlen && info[d].nrecords <= (1u << 22) && info[d].nrecords == info[0].nrecords &&
             info[d].stream_bytes == info[0].stream_bytes;
    if (c->pinned) sd_pin_put(c->buf); else free(c->buf);      /* (the text is on the device, or nobody wants it) */
    c->buf = NULL; c->pinned = 0;
    if (!ok) { c->text = SD_TEXT_DECLINED; return 0; }
    n = (uint32_t)info[0].nrecords;
    c->len = (uint64_t *)malloc(((size_t)n + 1) * sizeof *c->len);
    c->pstart = (uint32_t *)malloc(((size_t)n + 1) * sizeof *c->pstart);
    c->prec = (uint32_t *)malloc(((size_t)n + 1) * sizeof *c->prec);
    if (!c->len || !c->pstart || !c->prec) return SK_E_NOMEM;
    if (n) memcpy(c->pstart, starts, (size_t)n * sizeof *c->pstart);
    for (i = 0; i < n; i++) {
        const uint64_t l = (i + 1 < n ? (uint64_t)c->pstart[i + 1] : info[0].stream_bytes) - c->pstart[i] - 1;
        c->len[i] = l;
        c->prec[i] = i;
        if (l >= SK_K) { c->t_reads++; c->t_eval += l - (SK_K - 1); }
    }
    c->nrec = c->np = n;
    c->blen = info[0].stream_bytes;
    c->text = SD_TEXT_ACCEPTED;
    n_text_taken++;
    if (n) st->carry_last_len = (size_t)c->len[n - 1];
    if (c->t_eof) {
        /* the file ends behind a whole record and its '\\n': the host parser would stand in P_SEEK after a FASTQ record (END_STALE, the
         * last record's length) and at a line start in FASTA (END_RESET) -- sk_parser.h: parser_eof */
        c->last = 1;
        c->end_kind = info[0].form == SK_TEXT_FASTQ4 ? SKP_END_STALE : SKP_END_RESET;
        c->end_len = info[0].form == SK_TEXT_FASTQ4 ? st->carry_last_len : 0;
        pthread_mutex_lock(&st->mu);
        st->text_verdict = SD_VERDICT_DONE;
        pthread_cond_broadcast(&st->cv);
        pthread_mutex_unlock(&st->mu);
    }
    return 1;
}

/* the piece `c` declined: the reader's host path takes the file from c's start, and the text read ahead beyond it goes */
static void sd_text_decline(sd_stream *st, sd_chunk *c)
{
    int i;
    n_text_declined++;                                           /* (no other piece is on its way up: the next one goes when this one's scan runs) */
    pthread_mutex_lock(&st->mu);
    st->text_verdict = SD_VERDICT_HOST;
    st->text_off = c->toff;
    for (i = 0; i < st->qn; i++) chunk_free(st->q[i]);          /* (all of them text: the host path has not begun) */
    st->qn = 0;
    pthread_cond_broadcast(&st->cv);
    pthread_mutex_unlock(&st->mu);
}

/* One chunk against every strain.  uploaded: its bytes are in `batches` already (prefetched while the chunk before it was scanned);
 * launched: its scans are in flight as well (started while the chunk before it was being replayed: sd_launch_ahead). */
static int sd_tally_chunk(sd_prog *p, uint32_t ns, sk_batch **batches, sd_pool *pool, sd_chunk *c, int uploaded, int launched, sd_stream *st)
{
    int rc;
    double t0 = now_s(), t1;
    (void)pool;
    c->nstrains = ns;
    c->sp = (sd_sp *)calloc(ns, sizeof *c->sp);
    if (c->np) {
        int d;
        pthread_mutex_lock(&sd_dev_mu);
        rc = SK_OK;
        for (d = 0; d < sd_dev.n && !uploaded && rc == SK_OK; d++) { /* (asynchronous copies from page-locked memory: the devices' uploads overlap) */
            rc = c->packed ? sk_batch_fill_packed(batches[d], c->buf, c->blen, c->pstart, c->np) : sk_batch_fill(batches[d], c->buf, c->blen, c->pstart, c->np);
            if (rc == SK_OK && d == 0) sd_tc_hand(st, c, batches[0]);
        }
        t1 = now_s(); t_fill += t1 - t0; t0 = t1;
        if (rc == SK_OK && !launched) rc = sd_launch(p, ns, batches);
        if (rc == SK_OK) {
            sd_prefetch(st);                                     /* the next chunk goes up while this one is scanned */
            rc = sd_collect(p, ns, batches, c, st);
        }
        pthread_mutex_unlock(&sd_dev_mu);
        if (sd_co.post) { lanes_post(job_new(SD_JOB_TALLY, sd_co.post, NULL)); sd_co.post = NULL; }     /* (a PE1 chunk folded with this one) */
        if (rc != SK_OK) return rc;
        if (c->co == SD_CO_HELD) { t_launch += now_s() - t0; return SK_OK; }      /* (its TALLY job follows when the PE2 chunk has shown what becomes of it) */
        t1 = now_s(); t_launch += t1 - t0; t0 = t1;
    }
    else sd_tc_hand(st, c, NULL);                                /* (nothing went up: the target cache still wants its records' lengths) */
    lanes_post(job_new(SD_JOB_TALLY, c, NULL));                  /* sort + spread, strain by strain, behind the main thread's back */
    t_post += now_s() - t0;
    return SK_OK;
}

/* The chunk that follows is uploaded already (st->pre) and this stream is the only user of the tables: start its scans NOW, so
 * that the devices work on it while the host replays the reference's read-after-read bookkeeping over the chunk just collected
 * (and compresses the strains' output) -- the two used to take turns.  Every result buffer of the current chunk has been copied
 * out by now (collect + spread), so the launches may overwrite the device side. */
static void sd_launch_ahead(sd_stream *st, sd_prog *p, uint32_t ns)
{
    const double t0 = now_s();
    if (!st->solo || !st->pre || st->ahead || getenv("SK_SD_NO_AHEAD")) return;
    if (st->pre->text && (sd_text_resolve(st, st->pre, st->bat[st->bcur ^ 1], 1) != 1 || !st->pre->np)) return;   /* (its turn will tell: a decline or an error is dealt with there) */
    pthread_mutex_lock(&sd_dev_mu);
    if (sd_launch(p, ns, st->bat[st->bcur ^ 1]) == SK_OK) st->ahead = st->pre;
    else sd_drain_scans();
    pthread_mutex_unlock(&sd_dev_mu);
    /* (a failed launch is not an error here: the chunk is launched again, and the error reported, when its turn comes -- but
     * the launches that DID start before the one that failed are waited for first: a context takes one launch at a time, and
     * their results are not collected -- ADVICE r03) */
    t_launch += now_s() - t0;
}

/* make sure the stream's current chunk has an unread record: 1 = st->c->...[st->ci] is it, 0 = end of
 * file (end_kind, end_len set), < 0 device error */
static int stream_fill(sd_stream *st, sd_prog *p, uint32_t ns, sk_batch *batch, sd_pool *pool)
{
    for (;;) {
        sd_chunk *c;
        int rc, i;
        if (st->c && st->ci < st->c->nrec) return 1;
        if (st->eof) return 0;
        if (st->c) {
            if (st->c->last) {
                st->eof = 1; st->end_kind = st->c->end_kind; st->end_len = st->c->end_len; chunk_free(st->c); st->c = NULL;
                return st->split_failed ? SK_E_SPLIT : 0;
            }
            { const double t0 = now_s(); chunk_free(st->c); t_cfree += now_s() - t0; }
            st->c = NULL;
        }
        {
            const double t0 = now_s();
            pthread_mutex_lock(&st->mu);
            while (st->qn == 0) pthread_cond_wait(&st->cv, &st->mu);
            t_wait += now_s() - t0;
        }
        c = st->q[0];
        for (i = 1; i < st->qn; i++) st->q[i - 1] = st->q[i];
        st->qn--;
        pthread_cond_broadcast(&st->cv);
        pthread_mutex_unlock(&st->mu);
        if (c->cache_err) { chunk_free(c); st->cache_failed = 1; st->eof = 1; return SK_E_CACHE; }
        {
            const double t0 = now_s();
            int uploaded = st->pre == c;                   /* its bytes went up while the chunk before it was scanned */
            const int launched = uploaded && st->ahead == c;   /* ... and its scans were started while that chunk was replayed */
            (void)batch;
            if (uploaded) st->bcur ^= 1;
            st->pre = NULL;
            st->ahead = NULL;
            for (i = 0; i < sd_dev.n; i++)
                if (!st->bat[st->bcur][i] && (rc = sd_batch_get(i, &st->bat[st->bcur][i])) != SK_OK) { st->bat[st->bcur][i] = NULL; chunk_free(c); return rc; }
            if (c->text) {                                 /* a piece of text: what the device made of it */
                rc = sd_text_resolve(st, c, st->bat[st->bcur], uploaded);
                if (rc < 0) { chunk_free(c); return rc; }
                if (rc == 0) { sd_text_decline(st, c); chunk_free(c); t_tally += now_s() - t0; continue; }      /* the host parser's chunks follow */
                uploaded = 1;                              /* (the batch holds it) */
            }
            c->rec0 = st->nrec_seen; st->nrec_seen += c->nrec;
            if (sd_co.acc && sd_co.mode == SD_PEI) {       /* (interleaved pairs: is the chunk's first record the last chunk's last record's mate?) */
                c->co_a0 = c->nrec ? st->co_next : 0;
                if (c->nrec) st->co_next = (c->nrec - c->co_a0) & 1u;
            }
            rc = sd_tally_chunk(p, ns, st->bat[st->bcur], pool, c, uploaded, launched, st);
            if (rc == SK_OK) sd_launch_ahead(st, p, ns);
            t_tally += now_s() - t0;
        }
        if (rc != SK_OK) { chunk_free(c); return rc; }
        st->c = c;
        st->ci = 0;
    }
}

/* take the current, fully read chunk away from the stream so that it survives the next stream_fill */
static sd_chunk *stream_steal(sd_stream *st)
{
    sd_chunk *c = st->c;
    if (c->last) { st->eof = 1; st->end_kind = c->end_kind; st->end_len = c->end_len; }
    st->c = NULL;
    return c;
}

static unsigned char *put_int(unsigned char *w, int v)
{
    char tmp[12];
    int n = 0;
    unsigned u = v < 0 ? 0u - (unsigned)v : (unsigned)v;
    if (v < 0) *w++ = '-';
    do { tmp[n++] = (char)('0' + u % 10u); u /= 10u; } while (u);
    while (n) *w++ = (unsigned char)tmp[--n];
    return w;
}

/* the hit lines of one read: "<file>\t<hits PE1>\t<informative PE1>\t<hits PE2>\t<informative PE2>\t<k-mer>\n"
 * (src/strain_detect.c:567,608), formatted straight into the output block */
/* --coverage-rarefaction where the lines are counted on the host: the lines of the pair the replay is at, by the pair's class */
static void rar_host_lines(sd_prog *p, const uint32_t *rows, uint32_t n)
{
    uint32_t j, c;
    if (!sd_rar.on || !n || !p->rar_best || !((long long)p->h1 + p->h2 > sd_rar.min)) return;
    c = skh_rarefaction_class(&sd_rar.r, p->rar_pair);
    p->rar_lines[c] += n;
    for (j = 0; j < n; j++) if (rows[j] < p->ks.nrows && c > p->rar_best[rows[j]]) p->rar_best[rows[j]] = (uint8_t)c;
}

static void emit_rows(sd_prog *p, const uint32_t *rows, uint32_t n, const char *name)
{
    const size_t nl = strlen(name);
    uint32_t j;
    char key[32];
    if (sd_co.on) {                                        /* --coverage-only: no line, only what the script would count of it */
        if (!sd_co.acc) { for (j = 0; j < n; j++) skc_add_hit(p->cov, name, p->h1, p->h2, rows[j]); rar_host_lines(p, rows, n); return; }
        if (!n || !((long long)p->h1 + p->h2 > (sd_thr.on && sd_thr.t[0] < sd_co.min ? (long long)sd_thr.t[0] : sd_co.min))) return;
        if (p->co_n + n > p->co_cap) {
            p->co_cap = (p->co_n + n) * 2 + 1024;
            p->co_rows = (uint32_t *)realloc(p->co_rows, (size_t)p->co_cap * sizeof *p->co_rows);
            if (p->co_rows && (sd_thr.on || sd_rar.on)) {
                uint32_t *t2 = (uint32_t *)realloc(p->co_tot, (size_t)p->co_cap * sizeof *p->co_tot);
                if (t2) p->co_tot = t2;
                else { free(p->co_rows); p->co_rows = NULL; }
            }
            if (p->co_rows && sd_rar.on) {
                uint64_t *o2 = (uint64_t *)realloc(p->co_pair, (size_t)p->co_cap * sizeof *p->co_pair);
                if (o2) p->co_pair = o2;
                else { free(p->co_rows); p->co_rows = NULL; }
            }
            if (!p->co_rows) { p->co_cap = p->co_n = 0; p->job_rc = SK_E_NOMEM; return; }
        }
        for (j = 0; j < n && sd_rar.on; j++) p->co_pair[p->co_n + j] = p->rar_pair;
        if (sd_thr.on || sd_rar.on) {                      /* (unfiltered: the device applies --min-kmer-hits and the list to the total) */
            const long long tot = (long long)p->h1 + p->h2;
            for (j = 0; j < n; j++) p->co_tot[p->co_n + j] = tot > 0xFFFFFFFFll ? 0xFFFFFFFFu : (uint32_t)tot;
        }
        memcpy(p->co_rows + p->co_n, rows, (size_t)n * sizeof *rows);
        p->co_n += n;
        if (p->co_n >= sd_co.flush_rows) co_flush(p, (uint32_t)(p - sd_ln.p));
        return;
    }
    for (j = 0; j < n; j++) {
        if (p->table_on_device && p->ks.packed[rows[j]] == 0) {       /* (a row whose key was not fetched with the informative ones: one at a time) */
            int frc;
            pthread_mutex_lock(&sd_dev_mu);
            frc = skh_keyset_fetch_keys(&p->ks, p->ctx, &rows[j], 1);
            pthread_mutex_unlock(&sd_dev_mu);
            if (frc != SK_OK) {
                p->job_rc = SK_E_HIP;
                return;                                      /* never print a line without its k-mer (a key of 0 would decode to thirty-one A's): the run fails */
            }
        }
        skh_keyset_key(&p->ks, rows[j], key);
        if (nl <= 3800) {
            unsigned char *w0 = skzo_reserve(p->zo, nl + 128), *w = w0;
            memcpy(w, name, nl); w += nl;
            *w++ = '\t'; w = put_int(w, p->h1);
            *w++ = '\t'; w = put_int(w, p->i1);
            *w++ = '\t'; w = put_int(w, p->h2);
            *w++ = '\t'; w = put_int(w, p->i2);
            *w++ = '\t';
            { const size_t kl = strlen(key); memcpy(w, key, kl); w += kl; }
            *w++ = '\n';
            p->zo->len += (size_t)(w - w0);
        } else {                                           /* a path longer than a block's slack: the slow way */
            char num[64];
            skzo_append(p->zo, name, nl);
            skzo_append(p->zo, num, (size_t)snprintf(num, sizeof num, "\t%d\t%d\t%d\t%d\t", p->h1, p->i1, p->h2, p->i2));
            skzo_append(p->zo, key, strlen(key));
            skzo_append(p->zo, "\n", 1);
        }
        if (p->cov) skc_add_hit(p->cov, name, p->h1, p->h2, rows[j]);
    }
    if (p->cov) rar_host_lines(p, rows, n);
}

static void emit_trailer(sd_prog *p, const char *f1, const char *what, long long v)
{
    char num[64];
    if (!p->zo) return;                                    /* (--coverage-only: there is no hit list) */
    skzo_append(p->zo, "#", 1);
    skzo_append(p->zo, f1, strlen(f1));
    skzo_append(p->zo, "\t", 1);
    skzo_append(p->zo, what, strlen(what));
    skzo_append(p->zo, num, (size_t)snprintf(num, sizeof num, "\t%lld\n", v));
}

/* One strain over a run of n read pairs whose records sit in the current chunks: PE1 reads are records
 * a0, a0 + astep, ... of chunk ca; their mates (cb != NULL) records b0, b0 + astep, ... of chunk cb.
 * This is the body of the reference's read loop (src/strain_detect.c:443-626) for that strain. */
static uint32_t sp_lower(const sd_sp *q, uint32_t rec)
{
    uint32_t lo = 0, hi = q->n;
    while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (q->rec[mid] < rec) lo = mid + 1; else hi = mid; }
    return lo;
}

/* first_valid: the first pair of the run whose PE1 read has k bases (n if none) -- from there on the copy of "the PE1 read
 * last seen" exists (have_copy; the same for every strain).
 * Only the pairs that matter are walked: a pair with a hit, and the pairs behind it for as long as the carried tallies are
 * not all zero (a read shorter than k refreshes nothing, :444, so it re-emits what the read before it left).  A pair without
 * hits met with all-zero tallies leaves them all zero and emits nothing: skipped. */
static void sd_replay_run(sd_prog *p, uint32_t s, const char *f1, const sd_chunk *ca, uint32_t a0, const sd_chunk *cb, uint32_t b0,
                          uint32_t astep, uint32_t n, int have_copy_in, uint32_t first_valid, int mute, sks_list *sup, uint64_t pair_base)
{
    const sd_sp *A = &ca->sp[s], *B = cb ? &cb->sp[s] : NULL;
    const uint64_t a_end = (uint64_t)a0 + (uint64_t)n * astep, b_end = (uint64_t)b0 + (uint64_t)n * astep;
    uint32_t ia = sp_lower(A, a0), ib = B ? sp_lower(B, b0) : 0, j = 0;
    while (j < n) {
        uint32_t ra, rb;
        int b_valid = 0;
        if (!(p->h1 | p->i1 | p->h2 | p->i2)) {                 /* nothing carried: on to the next pair with a hit */
            uint32_t ja = n, jb = n;
            while (ia < A->n && A->rec[ia] < (uint64_t)a0 + (uint64_t)j * astep) ia++;       /* (behind pair j: done with) */
            while (B && ib < B->n && B->rec[ib] < (uint64_t)b0 + (uint64_t)j * astep) ib++;
            for (; ia < A->n && A->rec[ia] < a_end; ia++) { const uint32_t off = A->rec[ia] - a0; if (off % astep == 0) { ja = off / astep; break; } }
            if (B) for (; ib < B->n && B->rec[ib] < b_end; ib++) { const uint32_t off = B->rec[ib] - b0; if (off % astep == 0) { jb = off / astep; break; } }
            if ((ja < jb ? ja : jb) > j) j = ja < jb ? ja : jb;
            if (j >= n) break;
        }
        ra = a0 + j * astep; rb = b0 + j * astep;
        if (ca->len[ra] >= SK_K) {                       /* a read shorter than k refreshes nothing (:444) */
            uint32_t nrows = 0;
            while (ia < A->n && A->rec[ia] < ra) ia++;
            if (ia < A->n && A->rec[ia] == ra) {
                p->h1 = (int)A->all[ia]; p->i1 = (int)A->inf[ia];
                nrows = A->hbeg[ia + 1] - A->hbeg[ia];
                if (nrows) {
                    if (nrows > p->copy_cap) { p->copy_cap = nrows * 2 + 16; p->copy_rows = (uint32_t *)realloc(p->copy_rows, (size_t)p->copy_cap * 4); }
                    memcpy(p->copy_rows, A->rows + A->hbeg[ia], (size_t)nrows * 4);
                }
            } else p->h1 = p->i1 = 0;
            p->copy_n = nrows;
        }
        if (cb && cb->len[rb] >= SK_K) {
            b_valid = 1;
            while (ib < B->n && B->rec[ib] < rb) ib++;
            if (ib < B->n && B->rec[ib] == rb) { p->h2 = (int)B->all[ib]; p->i2 = (int)B->inf[ib]; }
            else { p->h2 = p->i2 = 0; b_valid = 2; }       /* (valid, no rows) */
        }
        if (!mute && p->h1 + p->h2 >= 1 && p->i1 + p->i2 >= 1) {
            uint32_t la = 0, lb = 0;
            p->rar_pair = pair_base + j;
            if (have_copy_in || first_valid <= j) { emit_rows(p, p->copy_rows, p->copy_n, f1); la = p->copy_n; }
            if (b_valid == 1) { lb = B->hbeg[ib + 1] - B->hbeg[ib]; emit_rows(p, B->rows + B->hbeg[ib], lb, f1); }
            /* support: the emission, by the run's own --min-kmer-hits whatever emit_rows lets through for a threshold list */
            if (sup && la + lb && (long long)p->h1 + p->h2 > sd_co.min && sks_list_push(sup, j, la + lb, (la ? 1u : 0u) | (lb ? 2u : 0u)))
                p->job_rc = SK_E_NOMEM;
        }
        j++;
    }
}

/* Post one run to the lanes (they replay it strain by strain, behind the runs posted before); returns the (strain-independent)
 * have_copy afterwards.  The job holds the two chunks until every lane is through with it. */
static int post_replay(const char *f1, sd_chunk *ca, uint32_t a0, sd_chunk *cb, uint32_t b0, uint32_t astep, uint32_t n, int have_copy,
                       uint64_t pair_base)
{
    sd_job *j = job_new(SD_JOB_REPLAY, ca, cb);
    uint32_t k;
    j->pair_base = pair_base;
    j->f1 = f1; j->a0 = a0; j->b0 = b0; j->astep = astep; j->n = n; j->have_copy = have_copy;
    for (k = 0; k < n && ca->len[a0 + k * astep] < SK_K; k++) { }
    j->first_valid = k;
    if (sd_sup.acc) {                                        /* (no lists: nothing is recorded, and the target's end reports the failure) */
        j->sup = (sks_list *)calloc(sd_ln.ns, sizeof *j->sup);
        j->sup_sample = sd_sup.sample;
        if (!j->sup) __atomic_store_n(&sd_sup.failed, 1, __ATOMIC_RELAXED);
    }
    lanes_post(j);
    return have_copy || k < n;
}

/* one metagenome (pair), for every strain at once.  The read lengths -- hence which read refreshes which
 * tallies, the totals and the "PE2 ended early" failure -- are the same for all strains and are handled
 * here, run by run; the per-strain part is sd_replay_run.  A read shorter than k refreshes nothing, so it
 * re-uses (and may re-emit) the previous read's tallies and sequence, as in the reference. */
/* --coverage-background, where a target ends: the count column(s) of every strain or union, swept into the target's block per
 * strain and left zero for the next target.  Every batch of the target has been collected by now, so every count scan is done. */
static int sd_background_target(sd_prog *p, uint32_t ns, const char *f1)
{
    const uint32_t words = SK_BACKGROUND_WORDS(sd_bg.max);
    uint64_t *blk = (uint64_t *)malloc((size_t)SK_UNION_MAX * words * sizeof *blk);
    const double t0 = now_s();
    uint32_t g, s, m;
    int rc = blk ? SK_OK : SK_E_NOMEM;
    sd_bg_error = NULL;
    if (rc == SK_OK && sd_bg.failed) rc = sd_bg.failed;
    pthread_mutex_lock(&sd_dev_mu);
    for (g = 0; g < sd_un.n && rc == SK_OK; g++) {
        const uint32_t a = g * sd_group, n = sk_union_members(sd_un.u[g]);
        rc = sk_union_background_finish(sd_un.u[g], 0, sd_bg.max, blk);
        if (rc != SK_OK) sd_bg_error = sk_union_last_error(sd_un.u[g]);
        for (m = 0; m < n && rc == SK_OK; m++) if (skb_add(p[a + m].bg, f1, blk + (size_t)m * words)) rc = SK_E_NOMEM;
    }
    for (s = 0; !sd_un.n && s < ns && rc == SK_OK; s++) {
        rc = sk_background_finish(p[s].ctx, SD_BGCOUNT, SD_TYPE, SD_INFORMATIVE, sd_bg.max, blk);
        if (rc != SK_OK) sd_bg_error = sk_last_error(p[s].ctx);
        if (rc == SK_OK && skb_add(p[s].bg, f1, blk)) rc = SK_E_NOMEM;
    }
    pthread_mutex_unlock(&sd_dev_mu);
    free(blk);
    sd_bg.ms_sweep += 1e3 * (now_s() - t0);
    return rc;
}

/* --coverage-rarefaction: a target's lines of strain p's table */
static int sd_rarefaction_line(sd_prog *p, const char *f1, const uint64_t *pairs, const uint64_t *unique, const uint64_t *total)
{
    const char *base = strrchr(f1, '/') ? strrchr(f1, '/') + 1 : f1;
    char *name = sd_rar.named ? sd_strain_name(p->o_path) : NULL;
    int rc = !p->ra_f || (sd_rar.named && !name) ? SK_E_NOMEM : skh_rarefaction_write(p->ra_f, &sd_rar.r, name, base, pairs, unique, total);
    free(name);
    return rc;
}

static int sd_quantify(sd_prog *p, uint32_t ns, sk_batch *batch, sd_pool *pool, const char *f1, const char *f2, int mode)
{
    sd_stream A, B;
    uint32_t s, j;
    int have_copy = 0, rc, got, status = 1;
    uint64_t pairs_done = 0;                             /* the target's pairs in front of the run at hand: its pair 0's ordinal */
    double t_mark;
    unsigned long long evaluated = 0, reads = 0;
    FILE *err = p[0].err;

    memset(&B, 0, sizeof B);
    t_mark = now_s();
    rc = stream_open(&A, f1, sd_gz_threads(mode == SD_PE ? 2 : 1));
    if (rc == SK_E_OPEN) { fprintf(err, "could not read file (read1) %s in quantify_hits_PE() (error: %s)\n", f1, strerror(errno)); return 1; }
    if (rc) { fprintf(err, "strain_detect: cannot start the reader of %s\n", f1); return 1; }
    if (mode == SD_PE) {
        rc = stream_open(&B, f2, sd_gz_threads(2));
        if (rc == SK_E_OPEN) { fprintf(err, "could not read file (read2) is_PE %s in quantify_hits_PE() (error: (null))\n", f2); stream_close(&A); return 1; }
        if (rc) { fprintf(err, "strain_detect: cannot start the reader of %s\n", f2); stream_close(&A); return 1; }
    }
    for (s = 0; s < ns; s++) { p[s].h1 = p[s].i1 = p[s].h2 = p[s].i2 = 0; p[s].copy_n = 0; }
    if (sd_sup.acc && (sd_sup.sample = sks_sample(sd_sup.acc, f1)) < 0) { fprintf(err, "strain_detect: out of memory\n"); goto done; }
    t_sopen += now_s() - t_mark;
    sd_co.mode = mode; sd_co.pe_a = mode == SD_PE ? &A : NULL;
    A.co_next = 0;
    A.nrec_seen = 0; B.nrec_seen = 0;
    if (sd_rar.on) {                                     /* nothing of the target before is left */
        memset(sd_rar.host_pairs, 0, sizeof sd_rar.host_pairs);
        for (s = 0; s < ns; s++) {
            memset(p[s].rar_lines, 0, sizeof p[s].rar_lines);
            if (!p[s].rar_best && !sd_co.acc && !(p[s].rar_best = (uint8_t *)malloc(p[s].ks.nrows ? p[s].ks.nrows : 1u))) { fprintf(err, "strain_detect: out of memory\n"); goto done; }
            if (p[s].rar_best) memset(p[s].rar_best, 0, p[s].ks.nrows ? p[s].ks.nrows : 1u);
        }
    }
    if (sd_co.on && !sd_co.acc) sd_co_hostacc++;
    A.solo = mode != SD_PE;                              /* (two streams take turns at the tables: no scan ahead of the replay) */

    while ((got = stream_fill(&A, p, ns, batch, pool)) == 1) {
        sd_chunk *ca = A.c, *cb = NULL, *held = NULL;
        uint32_t a0 = A.ci, b0 = 0, n = ca->nrec - a0, astep = 1;
        int mate_missing = 0;
        uint64_t stale_len2 = 0;
        if (mode == SD_PE) {
            got = stream_fill(&B, p, ns, batch, pool);
            if (got < 0) break;
            if (got == 1) { cb = B.c; b0 = B.ci; if (cb->nrec - b0 < n) n = cb->nrec - b0; }
            else { mate_missing = 1; stale_len2 = B.end_kind == SKP_END_RESET ? 0 : B.end_len; }   /* PE2 is exhausted for good */
        } else if (mode == SD_PEI) {
            if (n >= 2) { cb = ca; b0 = a0 + 1; astep = 2; n /= 2; }
            else {                                       /* the mate is the first record of the next chunk, or missing */
                held = stream_steal(&A);
                got = stream_fill(&A, p, ns, batch, pool);
                if (got < 0) { chunk_free(held); break; }
                if (got == 1) { cb = A.c; b0 = A.ci; }
                else { mate_missing = 1; stale_len2 = A.end_kind == SKP_END_RESET ? 0 : A.end_len; }
            }
        }
        /* strain-independent part of the run (:444-450,489-512) */
        t_mark = now_s();
        if (!cb && astep == 1 && a0 == 0 && n == ca->nrec) {
            /* a whole chunk of single reads (the usual case): its builder counted the records of k bases or more (np) and laid their
             * bases end to end with a '\n' after each (blen) -- the sums without a walk over 200,000 lengths per chunk */
            if (ca->text) { reads += ca->t_reads; evaluated += ca->t_eval; }     /* (a batch made from text holds the short records too: summed when it was accepted) */
            else {
            reads += ca->np;
            evaluated += (ca->blen - ca->np) - (uint64_t)(SK_K - 1) * ca->np;
            }
        } else
        for (j = 0; j < n; j++) {
            const uint64_t la = ca->len[a0 + j * astep];
            if (la >= SK_K) { reads++; evaluated += la - (SK_K - 1); }
            if (cb) { const uint64_t lb = cb->len[b0 + j * astep]; if (lb >= SK_K) evaluated += lb - (SK_K - 1); }
        }
        if (mate_missing && stale_len2 >= SK_K) {        /* the mate file ended first and its last length still reads as a read (:505-512) */
            fprintf(err, "reached end of PE2 (%s) before end of PE1 (%s), check that file names are correct\n", f2 ? f2 : "(null)", f1);
            chunk_free(held);
            goto done;
        }
        t_lens += now_s() - t_mark; t_mark = now_s();
        if (ca->co == SD_CO_HELD && (got = co_materialise(p, ns, ca)) != SK_OK) { chunk_free(held); break; }
        if (mode == SD_PEI && cb == ca && ca->co == SD_CO_FOLDED && a0 != ca->co_a0) { got = SK_E_STATE; break; }     /* (never: the fold began elsewhere) */
        if (sd_co.acc && n && ca->co == SD_CO_FOLDED &&
            (mode == SD_SE ? !cb : mode == SD_PEI ? cb == ca : cb && cb != ca && cb->co == SD_CO_FOLDED)) {
            /* the run was counted on the device: only the state its last pair leaves behind is replayed, and nothing is emitted */
            sd_job *jb;
            if (sd_rar.on && ca->co_base != pairs_done) { got = SK_E_STATE; break; }      /* (never: the fold numbered its pairs otherwise) */
            jb = job_new(SD_JOB_REPLAY, ca, cb);
            jb->f1 = f1; jb->a0 = a0 + (n - 1) * astep; jb->b0 = b0 + (n - 1) * astep; jb->astep = astep; jb->n = 1; jb->have_copy = 1; jb->mute = 1;
            lanes_post(jb);
            have_copy = 1;
            sd_co_dev++;
        } else {
            have_copy = post_replay(f1, ca, a0, cb, b0, astep, n, have_copy, pairs_done);
            if (sd_co.on) sd_co_replayed++;
            for (j = 0; j < n && sd_rar.on; j++) sd_rar.host_pairs[skh_rarefaction_class(&sd_rar.r, pairs_done + j)]++;
        }
        pairs_done += n;
        t_replay += now_s() - t_mark;
        if (held) { chunk_free(held); if (cb) A.ci++; }  /* PEI across a chunk boundary: the mate was A's next record */
        else {
            A.ci += n * astep;
            if (mode == SD_PE && cb) B.ci += n;
        }
    }
    /* --coverage-background counts every record of every file of the target, paired or not: what PE2 holds beyond PE1's last read
     * is scanned as well (its tallies go nowhere: no run is replayed over it) */
    while (sd_bg.on && mode == SD_PE && got == 0 && (rc = stream_fill(&B, p, ns, batch, pool)) != 0) {
        if (rc < 0) { got = rc; break; }
        B.ci = B.c->nrec;
    }
    {   /* the lanes run dry before anything is said about the file: the trailer lines follow the last hit line, and a strain's error
         * state is read only here */
        const double t0 = now_s();
        lanes_drain();
        t_lane_drain += now_s() - t0;
        for (s = 0; s < ns && got >= 0; s++) if (p[s].job_rc != SK_OK) got = p[s].job_rc;
    }
    if (got == SK_E_SPLIT) {
        fprintf(err, "strain_detect: %s could not be cut at record boundaries for parsing on several threads: nothing from it is reported; "
                     "run again with SK_NO_SPLIT=1\n", A.split_failed || !f2 ? f1 : f2);
        goto done;
    }
    if (got == SK_E_CACHE) {
        const sd_stream *bad = A.cache_failed ? &A : &B;
        fprintf(err, "strain_detect: the target cache file %s of %s failed its checks (a checksum, or lengths that do not give its stream): "
                     "hits of earlier chunks may be out already, the run fails; remove the file and run again\n", bad->tc_path ? bad->tc_path : "?", bad->path);
        status = SK_E_CACHE;
        goto done;
    }
    if (got < 0) {
        fprintf(err, "strain_detect: device error on %s: %s (%s)\n", f1, sk_strerror(got), sk_last_error(p[0].ctx));
        goto done;
    }
    if (sd_co.acc) {                                     /* the target's two numbers per strain, from the device's counters */
        uint32_t k, m;
        for (s = 0; s < ns; s++) { co_flush(&p[s], s); if (p[s].job_rc != SK_OK) got = p[s].job_rc; }
        for (k = 0; k < sd_co.nacc && got >= 0; k++) {
            uint64_t uq[SK_UNION_MAX], tot[SK_UNION_MAX];
            const uint32_t a = co_unit_first(k), n = co_unit_members(k);
            uint64_t *ru = NULL, *rt = NULL, bins = 0, at = 0, *sp = NULL, *deep = NULL;
            const uint32_t nsp = sd_spec.max + 1u;
            if (sd_rg.on) {                                  /* the same sweep, folded by region as well */
                for (m = 0; m < n; m++) bins += (uint64_t)p[a + m].rg.n + 1u;
                ru = (uint64_t *)malloc((size_t)bins * 2 * sizeof *ru);
                if (!ru) { got = SK_E_NOMEM; break; }
                rt = ru + bins;
            }
            if (sd_spec.on) {                                  /* ... and binned by depth */
                sp = (uint64_t *)malloc(((size_t)n * nsp + n) * sizeof *sp);
                if (!sp) { free(ru); got = SK_E_NOMEM; break; }
                deep = sp + (size_t)n * nsp;
            }
            pthread_mutex_lock(&sd_dev_mu);
            if (sd_rec.r) {                                  /* the target's non-zero rows into its plane, before the sweep clears them */
                uint64_t stray = 0;
                rc = sd_rec.next < sd_rec.T ? sk_covacc_mark_target(sd_co.acc[k], sd_rec.r[k], sd_rec.next, &stray) : SK_E_STATE;
                if (rc == SK_OK && stray) rc = SK_E_STATE;       /* (only informative rows are ever logged) */
                if (rc != SK_OK) { pthread_mutex_unlock(&sd_dev_mu); free(ru); free(sp); got = rc; break; }
            }
            if (sd_thr.on) {                                 /* the numbers per threshold: a pass of its own that changes no counter */
                uint64_t tu[SK_UNION_MAX * SK_COVACC_THRESHOLDS_MAX], tt[SK_UNION_MAX * SK_COVACC_THRESHOLDS_MAX];
                rc = sk_covacc_finish_target_thresholds(sd_co.acc[k], tu, tt);
                for (m = 0; m < n && rc == SK_OK; m++)
                    if (skc_add_threshold_counts(p[a + m].cov, f1, tu + (size_t)m * sd_thr.n, tt + (size_t)m * sd_thr.n, sd_thr.n)) rc = SK_E_NOMEM;
                if (rc != SK_OK) { pthread_mutex_unlock(&sd_dev_mu); free(ru); free(sp); got = rc; break; }
            }
            if (sd_sw.on) {                                  /* the numbers per fraction: a pass of its own that changes nothing */
                uint64_t cu[SK_UNION_MAX * SK_SCRUB_SWEEP_MAX], ct[SK_UNION_MAX * SK_SCRUB_SWEEP_MAX], stray = 0;
                uint32_t F = 0;
                for (m = 0; m < n; m++) if (p[a + m].sw_c.F > F) F = p[a + m].sw_c.F;
                rc = sk_covacc_finish_target_classes(sd_co.acc[k], cu, ct, &stray);
                if (rc == SK_OK && stray) rc = SK_E_STATE;       /* (only informative rows are ever logged, and each of them has a class) */
                for (m = 0; m < n && rc == SK_OK; m++)
                    if (skc_add_class_counts(p[a + m].cov, f1, cu + (size_t)m * F, ct + (size_t)m * F, p[a + m].sw_c.F)) rc = SK_E_NOMEM;
                if (rc != SK_OK) { pthread_mutex_unlock(&sd_dev_mu); free(ru); free(sp); got = rc; break; }
            }
            if (sd_rar.on) {                                 /* the numbers per fraction: a pass of its own that changes no counter */
                uint64_t rp[SK_COVACC_RAREFACTION_MAX], ru2[SK_UNION_MAX * SK_COVACC_RAREFACTION_MAX], rt2[SK_UNION_MAX * SK_COVACC_RAREFACTION_MAX], hp = 0;
                uint32_t q;
                rc = sk_covacc_finish_target_rarefaction(sd_co.acc[k], rp, ru2, rt2);
                for (q = sd_rar.r.n; rc == SK_OK && q-- > 0u; ) { hp += sd_rar.host_pairs[q + 1]; rp[q] += hp; }     /* (the replayed runs' pairs) */
                for (m = 0; m < n && rc == SK_OK; m++)
                    rc = sd_rarefaction_line(&p[a + m], f1, rp, ru2 + (size_t)m * sd_rar.r.n, rt2 + (size_t)m * sd_rar.r.n);
                if (rc != SK_OK) { pthread_mutex_unlock(&sd_dev_mu); free(ru); free(sp); got = rc; break; }
            }
            if (sd_sup.acc) {                                /* the pairs behind the numbers, of the runs folded on the device */
                uint64_t *sm = (uint64_t *)malloc(((size_t)3 * n + (size_t)2 * n * n) * sizeof *sm);
                rc = sm ? sk_covacc_finish_target_support(sd_co.acc[k], sm, sm + n, sm + 2 * n, sm + 3 * n, sm + 3 * n + (size_t)n * n) : SK_E_NOMEM;
                if (rc == SK_OK && sks_add_device(sd_sup.acc, (uint32_t)sd_sup.sample, a, n, sm, sm + n, sm + 2 * n, sm + 3 * n, sm + 3 * n + (size_t)n * n)) rc = SK_E_NOMEM;
                free(sm);
                if (rc != SK_OK) { pthread_mutex_unlock(&sd_dev_mu); free(ru); free(sp); got = rc; break; }
            }
            rc = sd_spec.on ? sk_covacc_finish_target_spectrum(sd_co.acc[k], uq, tot, sp, deep, ru, rt) :
                 sd_rg.on ? sk_covacc_finish_target_regions(sd_co.acc[k], uq, tot, ru, rt) : sk_covacc_finish_target(sd_co.acc[k], uq, tot);
            pthread_mutex_unlock(&sd_dev_mu);
            if (rc != SK_OK) { free(ru); free(sp); got = rc; break; }
            for (m = 0; m < n; m++) {
                if (skc_add_counts(p[a + m].cov, f1, uq[m], tot[m])) got = SK_E_NOMEM;
                if (sd_rg.on) {
                    if (skc_add_region_counts(p[a + m].cov, f1, ru + at, rt + at, p[a + m].rg.n + 1u)) got = SK_E_NOMEM;
                    at += (uint64_t)p[a + m].rg.n + 1u;
                }
                if (sd_spec.on && skc_add_spectrum_counts(p[a + m].cov, f1, sp + (size_t)m * nsp, deep[m], nsp)) got = SK_E_NOMEM;
            }
            free(ru); free(sp);
        }
        if (got < 0) { fprintf(err, "strain_detect: device error on %s: %s (%s)\n", f1, sk_strerror(got), sk_last_error(p[0].ctx)); goto done; }
        if (sd_rec.r) {                                      /* the host remembers ordinal -> sample name */
            if (!(sd_rec.name[sd_rec.next] = strdup(f1))) { fprintf(err, "strain_detect: out of memory\n"); goto done; }
            sd_rec.next++;
        }
    }
    if (sd_rar.on && !sd_co.acc) {                       /* counted on the host: every strain's rows by their highest class */
        uint64_t rp[SK_COVACC_RAREFACTION_MAX], ru2[SK_COVACC_RAREFACTION_MAX], rt2[SK_COVACC_RAREFACTION_MAX];
        for (s = 0; s < ns; s++) {
            uint64_t rows[SK_COVACC_RAREFACTION_MAX + 1], hp = 0, hu = 0, ht = 0, i;
            uint32_t q;
            memset(rows, 0, sizeof rows);
            for (i = 0; p[s].rar_best && i < p[s].ks.nrows; i++) rows[p[s].rar_best[i]]++;
            for (q = sd_rar.r.n; q-- > 0u; ) {
                hp += sd_rar.host_pairs[q + 1]; hu += rows[q + 1]; ht += p[s].rar_lines[q + 1];
                rp[q] = hp; ru2[q] = hu; rt2[q] = ht;
            }
            if ((rc = sd_rarefaction_line(&p[s], f1, rp, ru2, rt2)) != SK_OK) { fprintf(err, "strain_detect: --coverage-rarefaction: %s on %s\n", sk_strerror(rc), f1); goto done; }
        }
    }
    if (sd_bg.on && (got = sd_background_target(p, ns, f1)) != SK_OK) {
        fprintf(err, "strain_detect: --coverage-background: %s on %s (%s)\n", sk_strerror(got), f1, sd_bg_error ? sd_bg_error : "");
        goto done;
    }
    if (__atomic_load_n(&sd_sup.failed, __ATOMIC_RELAXED)) { fprintf(err, "strain_detect: --coverage-support: out of memory\n"); goto done; }
    for (s = 0; s < ns; s++) {
        emit_trailer(&p[s], f1, "total_kmer_evaluated", (long long)evaluated);
        emit_trailer(&p[s], f1, "total_reads_evaluated", (long long)reads);
        emit_trailer(&p[s], f1, "total_genome_kmers", (long long)p[s].ks.nrows);
        emit_trailer(&p[s], f1, "total_genome_informative_kmers", (long long)p[s].genome_inf);
        if (p[s].cov) {
            skc_add_trailer(p[s].cov, f1, "total_kmer_evaluated", (int64_t)evaluated);
            skc_add_trailer(p[s].cov, f1, "total_reads_evaluated", (int64_t)reads);
            skc_add_trailer(p[s].cov, f1, "total_genome_kmers", (int64_t)p[s].ks.nrows);
            skc_add_trailer(p[s].cov, f1, "total_genome_informative_kmers", (int64_t)p[s].genome_inf);
        }
    }
    status = 0;
done:
    lanes_drain();                                       /* (every way out: nothing of this file is in work when its streams go) */
    sd_co.pe_a = NULL;
    t_mark = now_s();
    stream_close(&A);
    stream_close(&B);
    t_sclose += now_s() - t_mark;
    return status;
}

/* ---------------------------------------------------------------------------------------------
 * -a: flag the listed k-mers as informative (src/strain_detect.c:668-726)
 * ------------------------------------------------------------------------------------------- */
static int sd_flag_informative(sd_prog *p, const char *path, unsigned *n_out)
{
    gzFile g = gzopen(path, "r");
    char line[100];
    char **piece = NULL; int *kind = NULL;             /* kind: 0 wrong length, 1 looked up on the device, 2 cannot match */
    uint32_t *slot = NULL;
    size_t np = 0, cap = 0, i;
    uint8_t *stream = NULL; uint32_t *start = NULL, *tally = NULL; sk_hit *hits = NULL;
    uint32_t nq = 0;
    uint64_t nh = 0;
    unsigned n = 0;
    int rc = 0;
    if (!g) { fprintf(p->err, "could not read file %s in hash_scrubbed_kmers()\n", path); return 1; }
    while (gzgets(g, line, 100)) {                       /* pieces of at most 99 bytes, as the reference reads */
        char *nl;
        if (line[0] == '#') continue;
        if ((nl = strchr(line, '\n')) != NULL) *nl = '\0';
        if (np == cap) {
            cap = cap ? cap * 2 : 4096;
            piece = (char **)realloc(piece, cap * sizeof *piece);
            kind = (int *)realloc(kind, cap * sizeof *kind);
            slot = (uint32_t *)realloc(slot, cap * sizeof *slot);
        }
        piece[np] = strdup(line);
        kind[np] = 0;
        if (strlen(line) == SK_K) {
            const char *c;
            kind[np] = 1;
            /* the reference does not fold case here: a piece with a lower-case letter is oriented to a
             * string with a lower-case letter, which no (upper-cased) key equals */
            for (c = line; *c; c++) if (*c >= 'a' && *c <= 'z') kind[np] = 2;
            if (kind[np] == 1) slot[np] = nq++;
        }
        np++;
    }
    gzclose(g);
    if (nq) {
        uint32_t q = 0;
        stream = (uint8_t *)malloc((size_t)nq * 32);
        start = (uint32_t *)malloc((size_t)nq * 4);
        tally = (uint32_t *)malloc((size_t)nq * 8);
        hits = (sk_hit *)malloc((size_t)nq * sizeof *hits);
        for (i = 0; i < np; i++) {
            if (kind[i] != 1) continue;
            start[q] = q * 32;
            memcpy(stream + (size_t)q * 32, piece[i], SK_K);
            stream[(size_t)q * 32 + SK_K] = '\n';
            q++;
        }
        /* every row still has type PLAIN, so "informative hits" here are simply all hits */
        rc = sk_tally_batch(p->ctx, stream, (uint64_t)nq * 32, start, nq, SD_TYPE, SD_PLAIN, tally, hits, nq, &nh);
        if (rc) fprintf(p->err, "strain_detect: device error: %s (%s)\n", sk_strerror(rc), sk_last_error(p->ctx));
        else for (i = 0; i < nh && i < nq; i++) p->type[hits[i].row] = SD_INFORMATIVE;
    }
    for (i = 0; i < np && !rc; i++) {
        if (kind[i] == 0)
            fprintf(p->out, "error string length in the scrubbed kmer file (%s) must be the same size as the kmer length "
                            "(scrubbed kmer, scrubbed kmer len, seed len): %s, %d, %d\n", path, piece[i], (int)strlen(piece[i]), SK_K);
        else if (kind[i] == 1 && tally[2 * slot[i]]) n++;
        else fprintf(p->out, "error could not find informative kmer %s in the total kmer list\n", piece[i]);
    }
    if (!rc && p->ks.nrows) {
        /* every row's type is PLAIN on the device already (column 0 after the build: src/strain_detect.c:139): only the rows the
         * list named go up -- 50 k row numbers instead of the 20 MB column */
        uint32_t *rows = (uint32_t *)malloc(((size_t)nq + 1) * sizeof *rows), nr = 0;
        for (i = 0; i < nh && i < nq && rows; i++) rows[nr++] = hits[i].row;      /* (a row named twice is set twice) */
        rc = rows ? sk_counts_set_rows(p->ctx, SD_TYPE, rows, nr, SD_INFORMATIVE) : SK_E_NOMEM;
        free(rows);
        if (rc) fprintf(p->err, "strain_detect: device error: %s (%s)\n", sk_strerror(rc), sk_last_error(p->ctx));
    }
    for (i = 0; i < np; i++) free(piece[i]);
    free(piece); free(kind); free(slot); free(stream); free(start); free(tally); free(hits);
    *n_out = n;
    return rc ? 1 : 0;
}

/* ---------------------------------------------------------------------------------------------
 * -g: background filter (src/strain_detect.c:160-240)
 * ------------------------------------------------------------------------------------------- */
static int cmp_desc(const void *a, const void *b) { return (int)(*(const unsigned *)b - *(const unsigned *)a); }

static int removed_at(unsigned threshold, const unsigned *c, unsigned n)
{
    unsigned i; int r = 0;
    for (i = 0; i < n; i++) if (c[i] >= threshold) r++;
    return r;
}

static int sd_background_filter(sd_prog *p, const char *list, double fraction, unsigned n_inform)
{
    unsigned keep = (unsigned)(int)(n_inform * fraction), *c, *bg, i, n = 0, threshold = 1;
    int demoted = 0, rc;
    fprintf(p->out, "#removing %f proportion of %s kmers; informative %d keep at least %d\n", fraction, list, n_inform, keep);
    if (skh_scan_list(p->ctx, list, NULL, SD_BACKGROUND, NULL, p->err, 0, 1, NULL) != SK_OK) return 1;
    c = (unsigned *)calloc(n_inform ? n_inform : 1, sizeof *c);
    bg = (unsigned *)malloc((size_t)(p->ks.nrows ? p->ks.nrows : 1) * sizeof *bg);
    rc = sk_counts_fetch(p->ctx, SD_BACKGROUND, bg);
    if (rc) { fprintf(p->err, "strain_detect: device error: %s (%s)\n", sk_strerror(rc), sk_last_error(p->ctx)); free(c); free(bg); return 1; }
    for (i = 0; i < p->ks.nrows; i++) {
        if (p->type[i] != SD_INFORMATIVE) continue;
        if (n >= n_inform) { fputs("Error: too many background kmers\n", p->err); free(c); free(bg); return 1; }
        c[n++] = bg[i];
    }
    qsort(c, n_inform, sizeof *c, cmp_desc);
    if (keep >= 1 && c[keep - 1] > threshold) threshold = c[keep - 1];
    while ((unsigned)removed_at(threshold, c, n_inform) > keep) threshold++;
    for (i = 0; i < p->ks.nrows; i++)
        if (p->type[i] == SD_INFORMATIVE && bg[i] >= threshold) { p->type[i] = SD_PLAIN; demoted++; }
    fprintf(p->out, "#final_threshold %d removes %d background kmers %d removed\n", threshold, removed_at(threshold, c, n_inform), demoted);
    free(c);
    free(bg);
    rc = sk_counts_set(p->ctx, SD_TYPE, p->type);
    return rc ? 1 : 0;
}

/* ---------------------------------------------------------------------------------------------
 * main (src/strain_detect.c:61-158, 263-384)
 * ------------------------------------------------------------------------------------------- */
static int file_type(const char *s)
{
    if (!strcmp(s, "SE") || !strcmp(s, "se")) return SD_SE;
    if (!strcmp(s, "PE") || !strcmp(s, "pe")) return SD_PE;
    if (!strcmp(s, "PEI") || !strcmp(s, "pei") || !strcmp(s, "IPE") || !strcmp(s, "ipe")) return SD_PEI;
    return SD_UNKNOWN;
}

static void usage(FILE *err)
{
    fputs("Usage paired end with 2 files:\n\tstrain_detect -r <reference_genome.fna> -a <informative_kmer_file.txt> -b <paired-end-file1> -c <paired-end-file1> -t PE -o <kmer outfile>\n", err);
    fputs("Usage paired end interleaved 1 file:\n\tstrain_detect -r <reference_genome.fna> -a <informative_kmer_file.txt> -b <paired-end-file1>  -t PEI -o <kmer outfile>\n", err);
    fputs("Usage single end 1 file:\n\tstrain_detect -r <reference_genome.fna> -a <informative_kmer_file.txt> -b <single-end-file1>  -t SE -o <kmer outfile>\n", err);
    fputs("Usage single end 1 file:\n\tstrain_detect -r <reference_genome.fna> -a <informative_kmer_file.txt> -B <batch-list-of-metagenomes> -o <kmer outfile>\n\n", err);
    fputs("format for metagenomics batch file is:\n", err);
    fputs("PE\tfile1_PE1.fasta\tfile1_PE2.fasta\n", err);
    fputs("SE\tfile1_PE1.fasta\n", err);
    fputs("PEI\tfile1_PE1.fasta\n", err);
    fputs("\nlines that begin with # are considered comments and ignored\n", err);
    fputs("\ninformative kmer file is a list of all of the kmers left in the reference genome post scrubbing\n", err);
}

static skzo_pool *sd_zpool;             /* compressors of every -o file of the run (set by the main function) */

/* build one strain's state in two steps: the key set (host only; several strains build theirs at the
 * same time on separate threads), then the table on the device, -a flags, optional -g filter, -o file */
/* one strain of a -S list, opened on a worker thread: key set on the host, then its own context, table,
 * -a flags, -g filter and outfile.  What it would have printed is kept in two buffers and replayed by the
 * main thread in list order. */
typedef struct {
    sd_prog *p; const char *r, *a, *g, *o; int device, failed, done;
    int adopted;                          /* the strain is resident already (its context and key set were taken over): sd_strain_adopted */
    char *out_buf, *err_buf; size_t out_len, err_len;
    sk_ctxjob *cj;                        /* the first strain takes the context that was opened while the key sets were built */
} ks_job;
typedef struct { ks_job *jobs; uint32_t njobs, next; pthread_mutex_t mu; pthread_cond_t cv; } ks_pool;

static int sd_strain_finish(sd_prog *p, int ks_rc, const char *r, const char *a, const char *g, const char *o, int device);
static int sd_strain_adopted(sd_prog *p, const char *a, const char *g, const char *o);

/* A strain's key set.  Round 3: built ON THE DEVICE from the strain's text (skh_keyset_build_on_device: the host only parses the
 * file and packs the bases; no hash table of 5 M keys on the host, no 140 MB of keys, permutations and columns over PCIe) -- the
 * context must be there first.  A strain with byte-string keys (U, IUPAC), a context that could not be opened (the caller reports it)
 * or SK_SD_HOST_KEYSET=1 (tests compare the two ways) take the host's builder as before; strain_detect never shows the order of
 * the rows, so either numbering serves. */
static int sd_keyset(sd_prog *p, const char *r, int device)
{
    if (!getenv("SK_SD_HOST_KEYSET")) {
        if (!p->ctx && !p->ctx_rc) p->ctx_rc = sk_ctx_create(&p->ctx, device);
        if (p->ctx) {
            const int rc = skh_keyset_build_on_device(&p->ks, p->ctx, r, sd_ncols(), SD_PLAIN);
            if (rc == SK_OK) { p->table_on_device = 1; return SK_OK; }
            skh_keyset_free(&p->ks);
            if (rc != SK_E_UNSUPPORTED && rc != SK_E_OPEN) return rc;      /* (an unreadable file: the host's builder says so in the reference's words) */
        }
    }
    return skh_keyset_from_file(&p->ks, r, SD_ROW_ORDER, SD_PLAIN, 0);
}

static void *sd_keyset_pool_thread(void *arg)
{
    ks_pool *kp = (ks_pool *)arg;
    for (;;) {
        const uint32_t k = __atomic_fetch_add(&kp->next, 1u, __ATOMIC_RELAXED);
        ks_job *j;
        FILE *real_out, *real_err, *mo, *me;
        int rc;
        if (k >= kp->njobs) return NULL;
        j = &kp->jobs[k];
        if (j->cj) j->p->ctx_rc = sk_ctxjob_join(j->cj, &j->p->ctx);
        rc = j->adopted ? SK_OK : sd_keyset(j->p, j->r, j->device);
        real_out = j->p->out; real_err = j->p->err;
        mo = open_memstream(&j->out_buf, &j->out_len);
        me = open_memstream(&j->err_buf, &j->err_len);
        if (mo && me) { j->p->out = mo; j->p->err = me; }
        j->failed = j->adopted ? sd_strain_adopted(j->p, j->a, j->g, j->o) : sd_strain_finish(j->p, rc, j->r, j->a, j->g, j->o, j->device);
        if (mo) fclose(mo);
        if (me) fclose(me);
        j->p->out = real_out; j->p->err = real_err;
        pthread_mutex_lock(&kp->mu);
        j->done = 1;
        pthread_cond_broadcast(&kp->cv);
        pthread_mutex_unlock(&kp->mu);
    }
}

/* the informative rows, the -g filter, the output file: the part of a strain's opening that follows the table load */
static int sd_strain_flags(sd_prog *p, const char *a, const char *g, const char *o)
{
    unsigned n_inform = 0, i;
    p->type = (uint32_t *)malloc((size_t)(p->ks.nrows ? p->ks.nrows : 1) * sizeof(uint32_t));
    for (i = 0; i < p->ks.nrows; i++) p->type[i] = SD_PLAIN;
    if (sd_flag_informative(p, a, &n_inform)) return 1;
    if (g && sd_background_filter(p, g, 0.5, n_inform)) return 1;
    for (i = 0; i < p->ks.nrows; i++) if (p->type[i] == SD_INFORMATIVE) p->genome_inf++;
    if (p->table_on_device && p->genome_inf) {           /* the k-mers the hit lines will print: the informative rows' keys, and no others */
        uint32_t *rows = (uint32_t *)malloc((size_t)p->genome_inf * sizeof *rows), nr = 0;
        int rc;
        for (i = 0; i < p->ks.nrows; i++) if (p->type[i] == SD_INFORMATIVE) rows[nr++] = i;
        rc = skh_keyset_fetch_keys(&p->ks, p->ctx, rows, nr);
        free(rows);
        if (rc) { fprintf(p->err, "strain_detect: device error: %s (%s)\n", sk_strerror(rc), sk_last_error(p->ctx)); return 1; }
    }
    p->zo = sd_co.on ? NULL : skzo_open(sd_zpool, o);      /* (--coverage-only: -o only names the strain and the table) */
    if (!p->zo && !sd_co.on) { fprintf(p->err, "could not open *gzout file outfile %s in quantify_hits_all_files()\n", o); return 1; }
    p->o_path = strdup(o);
    return 0;
}

static int sd_strain_finish(sd_prog *p, int ks_rc, const char *r, const char *a, const char *g, const char *o, int device)
{   /* p->ctx may already hold a context opened in the background (single-strain start-up) */
    int rc = ks_rc;
    FILE *err = p->err;
    if (rc == SK_E_OPEN) { fprintf(err, "could not read file %s GEN_hash_sequences_set_count_vec()\n", r); return 1; }
    if (rc != SK_OK) { fprintf(err, "strain_detect: %s\n", sk_strerror(rc)); return 1; }
    if (p->ks.short_records)
        fprintf(err, "strain_detect: skipped %llu reference record(s) shorter than %d bases "
                     "(the original program crashes on these)\n", (unsigned long long)p->ks.short_records, SK_K - 1);
    {
        const double t0 = now_s();
        double t1, t2;
        int frc;
        rc = p->ctx ? SK_OK : (p->ctx_rc ? p->ctx_rc : sk_ctx_create(&p->ctx, device));
        if (rc != SK_OK) { fprintf(err, "strain_detect: cannot use HIP device %d: %s\n", device, sk_strerror(rc)); return 1; }
        t1 = now_s();
        rc = p->table_on_device ? SK_OK : skh_keyset_load(p->ctx, &p->ks, sd_ncols());
        if (rc != SK_OK) { fprintf(err, "strain_detect: table load failed: %s (%s)\n", sk_strerror(rc), sk_last_error(p->ctx)); return 1; }
        t2 = now_s();
        frc = sd_strain_flags(p, a, g, o);
        pthread_mutex_lock(&t_open_mu);
        t_open_ctx += t1 - t0; t_open_load += t2 - t1; t_open_flags += now_s() - t2;
        pthread_mutex_unlock(&t_open_mu);
        return frc;
    }
}

/* The strains of a kmer_scrub_count run that goes on into strain_detect in the same process (key set, row
 * order, device table, filters and text are built ONCE for steps 1 and 3; src/strain_detect.c:137-146 rebuilds what
 * src/kmer_scrub_count.c:87-89 built).  sd_strain_adopt takes over ctx and *ks (the caller's copy is cleared), before anything
 * can fail: from then on the strain is closed with the others.  sd_strain_adopted then checks the table (loaded with at least
 * SD_NCOLS columns), puts every column back to what a fresh strain_detect start has, and flags the strain. */
static void sd_strain_adopt(sd_prog *p, sk_ctx *ctx, skh_keyset *ks, FILE *out, FILE *err)
{
    memset(p, 0, sizeof *p);
    p->out = out; p->err = err; p->ctx = ctx; p->ks = *ks;
    memset(ks, 0, sizeof *ks);
}

static int sd_strain_adopted(sd_prog *p, const char *a, const char *g, const char *o)
{
    sk_ctx *ctx = p->ctx;
    FILE *err = p->err;
    uint32_t col;
    int rc = SK_OK;
    if (!ctx) { fprintf(err, "strain_detect: no resident table\n"); return 1; }
    if (sk_table_cols(ctx) < SD_NCOLS || sk_table_rows(ctx) != p->ks.nrows) { fprintf(err, "strain_detect: the resident table does not fit (columns/rows)\n"); return 1; }
    for (col = 0; col < SD_NCOLS && rc == SK_OK; col++) rc = sk_counts_zero(ctx, col);
    if (rc == SK_OK && p->ks.nrows) {
        uint32_t *plain = (uint32_t *)malloc((size_t)p->ks.nrows * sizeof(uint32_t)), i;
        for (i = 0; i < p->ks.nrows; i++) plain[i] = SD_PLAIN;
        rc = sk_counts_set(ctx, SD_TYPE, plain);               /* what skh_keyset_load(.., default SD_PLAIN, incr 0) leaves there */
        free(plain);
    }
    if (rc != SK_OK) { fprintf(err, "strain_detect: device error: %s (%s)\n", sk_strerror(rc), sk_last_error(ctx)); return 1; }
    return sd_strain_flags(p, a, g, o);
}

/* --coverage-depth: where the table of strain p goes, and the accumulator that collects it */
static int sd_coverage_open(sd_prog *p, const char *explicit_path, int64_t min_hits)
{
    if (explicit_path && *explicit_path) p->cov_path = strdup(explicit_path);
    else {
        const size_t n = strlen(p->o_path);
        p->cov_path = (char *)malloc(n + 32);
        strcpy(p->cov_path, p->o_path);
        if (n >= 13 && !strcmp(p->cov_path + n - 13, ".kmer_hits.gz")) p->cov_path[n - 13] = 0;
        strcat(p->cov_path, ".coverage_depth");
    }
    p->cov = skc_create(min_hits);
    return p->cov ? 0 : 1;
}

static int sd_coverage_write(sd_prog *p)
{
    FILE *f;
    int rc;
    if (!p->cov) return 0;
    if (!(f = fopen(p->cov_path, "w"))) { fprintf(p->err, "strain_detect: could not write %s\n", p->cov_path); return 1; }
    rc = skc_report(p->cov, p->ctx, p->o_path, f, p->err);
    fclose(f);
    if (!rc && sd_rg.on) {
        if (!(f = fopen(p->rg_path, "w"))) { fprintf(p->err, "strain_detect: could not write %s\n", p->rg_path); return 1; }
        rc = skc_report_regions(p->cov, p->o_path, &p->rg, p->row_region, (uint32_t)p->ks.nrows, p->reg_inf, f, p->err);
        fclose(f);
    }
    if (!rc && sd_spec.on) {
        if (!(f = fopen(p->sp_path, "w"))) { fprintf(p->err, "strain_detect: could not write %s\n", p->sp_path); return 1; }
        rc = skc_report_spectrum(p->cov, p->o_path, sd_spec.max, f, p->err);
        fclose(f);
    }
    if (!rc && sd_thr.on) {
        if (!(f = fopen(p->th_path, "w"))) { fprintf(p->err, "strain_detect: could not write %s\n", p->th_path); return 1; }
        rc = skc_report_thresholds(p->cov, p->o_path, f, p->err);
        fclose(f);
    }
    if (!rc && sd_rar.on && p->ra_f) {
        if (fclose(p->ra_f)) rc = 1;
        p->ra_f = NULL;
        if (!rc && !(f = fopen(p->ra_path, "w"))) { fprintf(p->err, "strain_detect: could not write %s\n", p->ra_path); return 1; }
        if (!rc) { rc = fwrite(p->ra_buf, 1, p->ra_len, f) != p->ra_len; if (fclose(f)) rc = 1; }
        if (rc) fprintf(p->err, "strain_detect: error writing %s\n", p->ra_path);
    }
    if (!rc && sd_sw.on) {
        if (!(f = fopen(p->sw_path, "w"))) { fprintf(p->err, "strain_detect: could not write %s\n", p->sw_path); return 1; }
        rc = skc_report_classes(p->cov, p->o_path, p->row_class, (uint32_t)p->ks.nrows, f, p->err);
        fclose(f);
    }
    if (!rc && sd_rec.on) {
        FILE *fp = NULL;
        if (!(f = fopen(p->rc_path, "w"))) { fprintf(p->err, "strain_detect: could not write %s\n", p->rc_path); return 1; }
        if (sd_rec.pairs && !(fp = fopen(p->rp_path, "w"))) { fclose(f); fprintf(p->err, "strain_detect: could not write %s\n", p->rp_path); return 1; }
        rc = skc_report_recurrence(p->cov, p->o_path, f, fp, p->err);
        fclose(f);
        if (fp) fclose(fp);
    }
    return rc;
}

/* --coverage-recurrence, --recurrence-pairs: where the tables of strain p go */
static char *sd_table_path(const char *o_path, const char *explicit_path, const char *suffix)
{
    const size_t n = strlen(o_path);
    char *t;
    if (explicit_path && *explicit_path) return strdup(explicit_path);
    if (!(t = (char *)malloc(n + strlen(suffix) + 1))) return NULL;
    strcpy(t, o_path);
    if (n >= 13 && !strcmp(t + n - 13, ".kmer_hits.gz")) t[n - 13] = 0;
    strcat(t, suffix);
    return t;
}

/* --coverage-background, --background-spectrum: the tables of strain p */
static int sd_background_write(sd_prog *p)
{
    char *name = sd_strain_name(p->o_path);
    FILE *f = name ? fopen(p->bg_path, "w") : NULL;
    int rc = f ? skb_write(p->bg, name, f) : -1;
    const char *bad = p->bg_path;
    if (f) fclose(f);
    if (!rc && p->bgs_path) {
        bad = p->bgs_path;
        rc = (f = fopen(p->bgs_path, "w")) ? skb_write_spectrum(p->bg, name, f) : -1;
        if (f) fclose(f);
    }
    free(name);
    if (rc) { fprintf(p->err, "strain_detect: could not write %s\n", bad); return 1; }
    return 0;
}

/* --coverage-support: every strain's table, and with --support-pairs the panel's one file */
static int sd_support_write(sd_prog *p, uint32_t ns)
{
    FILE *err = p[0].err, *f;
    char **name = NULL;
    uint32_t s;
    int bad = 0;
    for (s = 0; s < ns && !bad; s++) {
        if (!(f = fopen(p[s].su_path, "w"))) { fprintf(err, "strain_detect: could not write %s\n", p[s].su_path); return 1; }
        bad = sks_write_support(sd_sup.acc, s, f) != 0;
        if (fclose(f)) bad = 1;
        if (bad) fprintf(err, "strain_detect: error writing %s\n", p[s].su_path);
    }
    if (bad || !sd_sup.pairs_path) return bad;
    name = (char **)calloc(ns, sizeof *name);
    for (s = 0; name && s < ns; s++) if (!(name[s] = sd_strain_name(p[s].o_path))) break;
    if (!name || s < ns) { fprintf(err, "strain_detect: out of memory\n"); bad = 1; }
    else if (!(f = fopen(sd_sup.pairs_path, "w"))) { fprintf(err, "strain_detect: could not write %s\n", sd_sup.pairs_path); bad = 1; }
    else {
        bad = sks_write_pairs(sd_sup.acc, (const char *const *)name, f) != 0;
        if (fclose(f)) bad = 1;
        if (bad) fprintf(err, "strain_detect: error writing %s\n", sd_sup.pairs_path);
    }
    for (s = 0; name && s < ns; s++) free(name[s]);
    free(name);
    return bad;
}

static int sd_recurrence_open(sd_prog *p, const char *explicit_path, const char *explicit_pairs)
{
    p->rc_path = sd_table_path(p->o_path, explicit_path, ".coverage_recurrence");
    if (sd_rec.pairs) p->rp_path = sd_table_path(p->o_path, explicit_pairs, ".coverage_recurrence_pairs");
    if (!p->rc_path || (sd_rec.pairs && !p->rp_path)) { fprintf(p->err, "strain_detect: out of memory\n"); return 1; }
    return 0;
}

/* --coverage-thresholds: where the table of strain p goes, and the list to the strain's host accumulator */
static int sd_thresholds_open(sd_prog *p, const char *explicit_path)
{
    if (explicit_path && *explicit_path) p->th_path = strdup(explicit_path);
    else {
        const size_t n = strlen(p->o_path);
        p->th_path = (char *)malloc(n + 32);
        if (p->th_path) {
            strcpy(p->th_path, p->o_path);
            if (n >= 13 && !strcmp(p->th_path + n - 13, ".kmer_hits.gz")) p->th_path[n - 13] = 0;
            strcat(p->th_path, ".coverage_thresholds");
        }
    }
    if (!p->th_path || skc_set_thresholds(p->cov, sd_thr.t, sd_thr.n)) { fprintf(p->err, "strain_detect: out of memory\n"); return 1; }
    return 0;
}

/* --coverage-scrub-sweep, before a strain is opened or a file written: the class files of all strains read and held against their
 * informative lists -- a class file names exactly the list's k-mers, in its order, each with a class.  paths: four per strain as
 * sd_open_strains takes them (entry 1 the list, entry 3 a -g list, which is refused); explicit_classes: the one strain's class file. */
static int sd_sweep_load(skc_classes **out, uint32_t ns, char **paths, const char *explicit_classes, FILE *err)
{
    skc_classes *c = (skc_classes *)calloc(ns ? ns : 1u, sizeof *c);
    uint32_t s;
    if (!c) { fprintf(err, "strain_detect: out of memory\n"); return 1; }
    *out = c;
    for (s = 0; s < ns; s++)
        if (paths[4 * s + 3]) {
            fprintf(err, "strain_detect: --coverage-scrub-sweep does not go with a -g list (%s): its cut is sized by the number of informative k-mers, "
                         "so the fractions' sets would no longer be nested\n", paths[4 * s + 3]);
            return 1;
        }
    for (s = 0; s < ns; s++) {
        const char *a = paths[4 * s + 1];
        char *cp = explicit_classes ? strdup(explicit_classes) : (char *)malloc(strlen(a) + 16), why[240], line[100];
        gzFile g;
        uint64_t i = 0;
        int bad = 0;
        if (!cp) { fprintf(err, "strain_detect: out of memory\n"); return 1; }
        if (!explicit_classes) { strcpy(cp, a); strcat(cp, ".classes"); }
        if (skc_classes_read(cp, &c[s], why, sizeof why)) { fprintf(err, "strain_detect: --coverage-scrub-sweep: class file %s: %s\n", cp, why); free(cp); return 1; }
        if (!(g = gzopen(a, "r"))) { free(cp); continue; }           /* (an unreadable list: the strain's opening says so) */
        while (!bad && gzgets(g, line, 100)) {                       /* the list as sd_flag_informative reads it */
            char *nl;
            if (line[0] == '#') continue;
            if ((nl = strchr(line, '\n')) != NULL) *nl = '\0';
            if (i >= c[s].n || strcmp(line, c[s].arena + c[s].off[i])) bad = 1;
            i++;
        }
        gzclose(g);
        if (bad || i != c[s].n) {
            fprintf(err, "strain_detect: --coverage-scrub-sweep: class file %s does not name the k-mers of the informative list %s, each once and in its order "
                         "(they differ at k-mer %llu)\n", cp, a, (unsigned long long)(bad ? i : (i < c[s].n ? i : c[s].n) + 1u));
            free(cp);
            return 1;
        }
        free(cp);
    }
    return 0;
}

static void sd_sweep_drop(skc_classes *c, uint32_t ns)
{
    uint32_t s;
    for (s = 0; c && s < ns; s++) skc_classes_free(&c[s]);
    free(c);
}

/* ... and once the strain is open: where its table goes, its class file's k-mers to rows by one tally batch (as the -a list's are),
 * the header to the strain's host accumulator.  *c is taken over. */
static int sd_sweep_open(sd_prog *p, skc_classes *c, const char *explicit_path)
{
    const uint32_t nq = (uint32_t)c->n;
    uint8_t *stream = NULL; uint32_t *start = NULL, *tally = NULL; sk_hit *hits = NULL;
    uint64_t nh = 0, i, named = 0;
    int rc = SK_OK, bad = 0;
    p->sw_c = *c;
    memset(c, 0, sizeof *c);
    p->sw_path = sd_table_path(p->o_path, explicit_path, ".coverage_scrub_sweep");
    p->row_class = (uint8_t *)calloc(p->ks.nrows ? p->ks.nrows : 1, 1);
    p->sw_rows = (uint32_t *)malloc(((size_t)nq + 1) * sizeof *p->sw_rows);
    if (!p->sw_path || !p->row_class || !p->sw_rows || skc_set_classes(p->cov, &p->sw_c)) { fprintf(p->err, "strain_detect: out of memory\n"); return 1; }
    for (i = 0; i < nq; i++) p->sw_rows[i] = 0xFFFFFFFFu;
    if (nq) {
        stream = (uint8_t *)malloc((size_t)nq * 32);
        start = (uint32_t *)malloc((size_t)nq * 4);
        tally = (uint32_t *)calloc((size_t)nq * 2, 4);
        hits = (sk_hit *)malloc((size_t)nq * sizeof *hits);
        if (!stream || !start || !tally || !hits) { fprintf(p->err, "strain_detect: out of memory\n"); bad = 1; goto out; }
        for (i = 0; i < nq; i++) {
            const char *t = p->sw_c.arena + p->sw_c.off[i];
            if (strlen(t) != SK_K) { bad = 2; break; }                /* (held against the list already: a piece the list's reader also rejects) */
            start[i] = (uint32_t)i * 32;
            memcpy(stream + (size_t)i * 32, t, SK_K);
            stream[(size_t)i * 32 + SK_K] = '\n';
        }
        if (!bad) {
            rc = sk_tally_batch(p->ctx, stream, (uint64_t)nq * 32, start, nq, SD_TYPE, SD_INFORMATIVE, tally, hits, nq, &nh);
            if (rc) { fprintf(p->err, "strain_detect: device error: %s (%s)\n", sk_strerror(rc), sk_last_error(p->ctx)); bad = 1; goto out; }
        }
        for (i = 0; !bad && i < nh && i < nq; i++) {                  /* one informative hit per k-mer, on a row of its own */
            const uint32_t q = hits[i].pos / 32u, row = hits[i].row;
            if (q >= nq || row >= p->ks.nrows || p->row_class[row] || p->sw_rows[q] != 0xFFFFFFFFu) { bad = 2; break; }
            p->row_class[row] = p->sw_c.cls[q];
            p->sw_rows[q] = row;
            named++;
        }
    }
    if (!bad && (named != nq || (uint64_t)p->genome_inf != nq)) bad = 2;
    if (bad == 2)
        fprintf(p->err, "strain_detect: --coverage-scrub-sweep: the class file of %s does not name the strain's %u informative k-mers, each once\n",
                p->o_path, p->genome_inf);
out:
    free(stream); free(start); free(tally); free(hits);
    return bad ? 1 : 0;
}

/* --coverage-spectrum: where the table of strain p goes */
static int sd_spectrum_open(sd_prog *p, const char *explicit_path)
{
    if (explicit_path && *explicit_path) p->sp_path = strdup(explicit_path);
    else {
        const size_t n = strlen(p->o_path);
        p->sp_path = (char *)malloc(n + 32);
        if (p->sp_path) {
            strcpy(p->sp_path, p->o_path);
            if (n >= 13 && !strcmp(p->sp_path + n - 13, ".kmer_hits.gz")) p->sp_path[n - 13] = 0;
            strcat(p->sp_path, ".coverage_spectrum");
        }
    }
    if (!p->sp_path) { fprintf(p->err, "strain_detect: out of memory\n"); return 1; }
    return 0;
}

/* --coverage-regions: the region table of a strain file, before anything of the run is opened; more than SKH_REGIONS_MAX regions
 * are refused here */
static int sd_regions_load(skh_regions *rg, const char *genome, FILE *err)
{
    const int rc = skh_regions_from_file(genome, sd_rg.window, rg);
    if (rc == SK_OK) return 0;
    if (rg->too_many) fprintf(err, "strain_detect: --coverage-regions: %s has more than %u regions of %llu bases: choose a larger --region-window\n",
                              genome, SKH_REGIONS_MAX, (unsigned long long)sd_rg.window);
    else if (rc == SK_E_OPEN) fprintf(err, "strain_detect: --coverage-regions: could not read %s\n", genome);
    else fprintf(err, "strain_detect: --coverage-regions: %s: %s\n", genome, sk_strerror(rc));
    return 1;
}

/* ... and of an open strain: where the table goes (takes over *rg) */
static int sd_regions_open(sd_prog *p, skh_regions *rg, const char *explicit_path)
{
    p->rg = *rg;
    memset(rg, 0, sizeof *rg);
    if (explicit_path && *explicit_path) p->rg_path = strdup(explicit_path);
    else {
        const size_t n = strlen(p->o_path);
        p->rg_path = (char *)malloc(n + 32);
        if (p->rg_path) {
            strcpy(p->rg_path, p->o_path);
            if (n >= 13 && !strcmp(p->rg_path + n - 13, ".kmer_hits.gz")) p->rg_path[n - 13] = 0;
            strcat(p->rg_path, ".coverage_regions");
        }
    }
    p->reg_inf = (uint64_t *)calloc((size_t)p->rg.n + 1, sizeof *p->reg_inf);
    if (!p->rg_path || !p->reg_inf) { fprintf(p->err, "strain_detect: out of memory\n"); return 1; }
    return 0;
}

/* Every row's region and the informative rows per region ON THE HOST: what skc_report_regions needs to fold the host accumulator's
 * (sample, row) list -- --coverage-depth, and --coverage-only where it counts on the host.  Where the accumulators on the device
 * fold, they know both (sk_covacc_set_regions, sk_covacc_region_rows) and this walk over all rows is left out. */
static int sd_regions_rows(sd_prog *p)
{
    const uint32_t nrows = (uint32_t)p->ks.nrows;
    uint32_t *own = NULL, i;
    const uint32_t *fp = p->ks.first_pos;
    if (p->row_region) return 0;
    p->row_region = (uint32_t *)malloc(((size_t)nrows + 1) * sizeof *p->row_region);
    if (!p->row_region) { fprintf(p->err, "strain_detect: out of memory\n"); return 1; }
    memset(p->reg_inf, 0, ((size_t)p->rg.n + 1) * sizeof *p->reg_inf);
    if (!fp && nrows) {                                  /* a key set built on the device: the table knows the positions */
        int rc = SK_E_STATE;
        own = (uint32_t *)malloc((size_t)nrows * sizeof *own);
        if (own && sk_table_first_pos) rc = sk_table_first_pos(p->ctx, own);
        if (!own || rc != SK_OK) { fprintf(p->err, "strain_detect: --coverage-regions: %s (%s)\n", sk_strerror(own ? rc : SK_E_NOMEM), sk_last_error(p->ctx)); free(own); return 1; }
        fp = own;
    }
    for (i = 0; i < nrows; i++) {
        uint32_t r = p->rg.n;
        if (fp[i] != 0xFFFFFFFFu && p->rg.n && p->rg.text_off[0] <= fp[i]) {
            uint32_t lo = 0, hi = p->rg.n;
            while (hi - lo > 1u) { const uint32_t mid = lo + ((hi - lo) >> 1); if (p->rg.text_off[mid] <= fp[i]) lo = mid; else hi = mid; }
            r = lo;
        }
        p->row_region[i] = r;
        if (p->type[i] == SD_INFORMATIVE) p->reg_inf[r]++;
    }
    free(own);
    return 0;
}

static int sd_strain_open(sd_prog *p, const char *r, const char *a, const char *g, const char *o, int device, FILE *out, FILE *err)
{
    sk_ctxjob cj;
    int ks_rc;
    memset(p, 0, sizeof *p);
    p->out = out;
    p->err = err;
    sk_ctxjob_start(&cj, device);                        /* (the HIP runtime comes up on a helper thread) */
    p->ctx_rc = sk_ctxjob_join(&cj, &p->ctx);
    ks_rc = sd_keyset(p, r, device);
    return sd_strain_finish(p, ks_rc, r, a, g, o, device);
}

static void sd_strain_close(sd_prog *p)
{
    if (p->zo && skzo_close(p->zo)) fprintf(stderr, "strain_detect: error writing the -o file\n");
    /* SK_LEAK_AT_EXIT=1 (set by bin/strain_detect, whose process ends right after): the result file is complete; taking 32
     * device contexts and key sets apart one hipFree at a time (0.3-0.7 s for 32 strains) is left to the end of the process */
    if (getenv("SK_LEAK_AT_EXIT") && strcmp(getenv("SK_LEAK_AT_EXIT"), "0")) { memset(p, 0, sizeof *p); return; }
    if (p->ctx) { skh_pack_cache_set(p->ctx, NULL, NULL); sk_ctx_destroy(p->ctx); }
    skh_keyset_free(&p->ks);
    free(p->type); free(p->copy_rows); free(p->hitbuf); free(p->tallybuf); free(p->cov_path); free(p->o_path); free(p->co_rows); free(p->co_tot);
    if (p->ra_f) fclose(p->ra_f);
    free(p->ra_path); free(p->ra_buf); free(p->co_pair); free(p->rar_best);
    skc_destroy(p->cov);
    if (skh_regions_free) skh_regions_free(&p->rg);
    free(p->row_region); free(p->reg_inf); free(p->rg_path); free(p->sp_path); free(p->th_path); free(p->su_path); free(p->rc_path); free(p->rp_path);
    free(p->sw_path); free(p->sw_rows); free(p->row_class);
    free(p->bg_path); free(p->bgs_path);
    if (p->bg && skb_destroy) skb_destroy(p->bg);
    skc_classes_free(&p->sw_c);
    memset(p, 0, sizeof *p);
}

static void close_one(void *arg, uint32_t s) { sd_strain_close(&((sd_prog *)arg)[s]); }

/* one line of a -B list, cut in place: <type> TAB <file> [TAB <second file>] (src/strain_detect.c:300-340) */
enum { SD_LL_TARGET, SD_LL_EMPTY, SD_LL_UNKNOWN, SD_LL_NO_FIRST, SD_LL_NO_SECOND };
static int sd_list_line(char *line, int *m, char **tok, char **f1, char **f2)
{
    char *nl = strchr(line, '\n');
    if (nl) *nl = '\0';
    *f1 = *f2 = NULL;
    if (!(*tok = strtok(line, "\t"))) return SD_LL_EMPTY;
    if ((*m = file_type(*tok)) == SD_UNKNOWN) return SD_LL_UNKNOWN;
    if (!(*f1 = strtok(NULL, "\t"))) return SD_LL_NO_FIRST;
    if (*m == SD_PE && !(*f2 = strtok(NULL, "\t"))) return SD_LL_NO_SECOND;
    return SD_LL_TARGET;
}

/* the run's recurrence tables, once per unit, from the planes to each strain's accumulator */
static int sd_recurrence_finish(sd_prog *p, FILE *err)
{
    const uint32_t T = sd_rec.T;
    uint32_t k, m;
    if (sd_rec.next != T) { fprintf(err, "strain_detect: --coverage-recurrence: %u of %u targets were counted\n", sd_rec.next, T); return 1; }
    for (k = 0; k < sd_rec.nr; k++) {
        const uint32_t a = co_unit_first(k), n = co_unit_members(k);
        uint64_t *hist = (uint64_t *)malloc((size_t)n * (T + 1u) * sizeof *hist);
        uint64_t *pairs = sd_rec.pairs ? (uint64_t *)malloc((size_t)n * T * T * sizeof *pairs) : NULL;
        int rc = !hist || (sd_rec.pairs && !pairs) ? SK_E_NOMEM : SK_OK;
        if (rc == SK_OK) {
            pthread_mutex_lock(&sd_dev_mu);
            rc = sk_recur_finish(sd_rec.r[k], hist, pairs);
            pthread_mutex_unlock(&sd_dev_mu);
        }
        for (m = 0; m < n && rc == SK_OK; m++)
            if (skc_add_recurrence_counts(p[a + m].cov, (const char *const *)sd_rec.name, T, hist + (size_t)m * (T + 1u),
                                          pairs ? pairs + (size_t)m * T * T : NULL)) rc = SK_E_NOMEM;
        free(hist); free(pairs);
        if (rc != SK_OK) { fprintf(err, "strain_detect: --coverage-recurrence: %s (%s)\n", sk_strerror(rc), sk_last_error(p[a].ctx)); return 1; }
    }
    return 0;
}

/* the metagenome side of main (src/strain_detect.c:263-384), for ns strains at once */
static int sd_run(sd_prog *p, uint32_t ns, const char *B, const char *b, const char *b2, int mode, FILE *out, FILE *err)
{
    sk_batch *batch = NULL;                          /* (every stream has its own pair of device batches: stream_fill) */
    sd_pool pool;
    int bad = 0;
    sd_pin_open(p[0].ctx, sd_chunk_bytes());
    sd_all_p = p; sd_all_ns = ns;
    sd_unions_open(p, ns);
    if (sd_ps.path && sd_panel_share(p, ns)) { sd_unions_close(); return 1; }      /* (before any target is read) */
    if (sd_sup.on) {                                     /* a group = the strains of one union table; without unions every strain is alone */
        if (sd_sup.pairs_path && ns > 1 && sd_un.n != (ns + sd_group - 1) / sd_group) {
            fprintf(err, "strain_detect: --support-pairs: the strains cannot all be held in union tables (a strain with byte-string keys or "
                         "without a text stage, or a union that could not be built): no pairs of the panel\n");
            sd_unions_close();
            return 1;
        }
        sd_sup.failed = 0;
        if (!(sd_sup.acc = sks_create(ns, sd_un.n ? sd_group : 1u))) { fprintf(err, "strain_detect: out of memory\n"); sd_unions_close(); return 1; }
    }
    sd_co.host = 0;
    if (sd_co.on && B) {                                 /* the script keys its samples by basename: two targets that share one are one sample */
        FILE *fp = fopen(B, "r");
        char *line = NULL, **seen = NULL;
        size_t cap = 0;
        uint32_t nseen = 0, k;
        int nomem = 0;
        while (fp && !nomem && getline(&line, &cap, fp) != -1) {
            char *tok, *f1, *f2, **grown, *copy;
            int m;
            if (sd_list_line(line, &m, &tok, &f1, &f2) != SD_LL_TARGET) continue;       /* (the lines the loop below quantifies, and no others) */
            if (strrchr(f1, '/')) f1 = strrchr(f1, '/') + 1;
            for (k = 0; k < nseen; k++) if (!strcmp(seen[k], f1)) sd_co.host = 1;
            grown = (char **)realloc(seen, ((size_t)nseen + 1) * sizeof *seen);
            copy = grown ? strdup(f1) : NULL;
            if (grown) seen = grown;
            if (!copy) { nomem = 1; break; }
            seen[nseen++] = copy;
        }
        for (k = 0; k < nseen; k++) free(seen[k]);
        free(seen); free(line);
        if (fp) fclose(fp);
        if (nomem) { fprintf(err, "strain_detect: out of memory\n"); sd_unions_close(); return 1; }
        if (sd_co.host) fprintf(err, "strain_detect: --coverage-only: two targets of %s share a file name, the script counts them as one sample: "
                                     "this run is counted on the host\n", B);
    }
    {
        const int crc = co_open(p, ns);
        if (crc != SK_OK) { fprintf(err, "strain_detect: device error: %s (%s)\n", sk_strerror(crc), sk_last_error(p[0].ctx)); sd_unions_close(); return 1; }
    }
    if (sd_rg.on && !sd_co.acc) {                        /* (no accumulator on the device folds by region: the host will) */
        uint32_t s;
        for (s = 0; s < ns; s++) if (sd_regions_rows(&p[s])) { co_close(); sd_unions_close(); return 1; }
    }
    pool_start(&pool, ns);
    lanes_start(p, ns);
    if (B) {
        FILE *fp = fopen(B, "r");
        char *line = NULL, *tok, *f1, *f2;
        size_t cap = 0;
        if (!fp) { fprintf(err, "could not read file file_of_filenames %s in quantify_hits_all_files()\n", B); lanes_stop(); pool_stop(&pool); co_close(); sd_unions_close(); return 1; }
        while (!bad && getline(&line, &cap, fp) != -1) {
            int m;
            const int what = sd_list_line(line, &m, &tok, &f1, &f2);
            if (what == SD_LL_EMPTY) { fprintf(err, "strain_detect: empty line in %s (the original program crashes here)\n", B); bad = 1; break; }
            if (what == SD_LL_UNKNOWN) { fprintf(out, "unknown file type skipping line (%s)\n", tok); continue; }
            if (what == SD_LL_NO_FIRST) { fprintf(out, "ERROR: no first file specified for %s\n", line); continue; }
            if (what == SD_LL_NO_SECOND) { fprintf(out, "ERROR: no second file specified for PE: %s\n", line); continue; }
            bad = sd_quantify(p, ns, batch, &pool, f1, m == SD_PE ? f2 : NULL, m);
        }
        free(line);
        fclose(fp);
    } else bad = sd_quantify(p, ns, batch, &pool, b, b2, mode);
    lanes_stop();
    pool_stop(&pool);
    sd_unmap_wait();
    sd_batch_cache_close();
    if (getenv("SK_SD_SCAN_TIMING") && sk_scan_timing && sk_union_scan_timing) {   /* (opt-in: what --coverage-background's count scans add is read off two runs) */
        double ms = 0, one;
        uint64_t n = 0, k;
        uint32_t g, s;
        for (g = 0; g < sd_un.n; g++) if (sk_union_scan_timing(sd_un.u[g], &one, &k, 0) == SK_OK) { ms += one; n += k; }
        for (s = 0; !sd_un.n && s < ns; s++) if (sk_scan_timing(p[s].ctx, &one, &k, 0) == SK_OK) { ms += one; n += k; }
        fprintf(err, "strain_detect timing: scan kernels on the device: %.3f ms in %llu launches (TALLY%s)\n", ms, (unsigned long long)n,
                sd_bg.on ? " and the background's COUNT scans" : "");
    }
    if (!bad && sd_rec.r) bad = sd_recurrence_finish(p, err);
    co_close();
    if (getenv("SK_LEAK_AT_EXIT") && strcmp(getenv("SK_LEAK_AT_EXIT"), "0")) return bad;     /* (the process is about to end: see sd_strain_close) */
    { const double t0 = now_s(); sd_unions_close(); t_uclose = now_s() - t0; }
    return bad;
}

/* strains that are already resident (kmer_scrub_count ... --scrub f --detect ...): n contexts and key sets, taken over */
typedef struct {
    uint32_t n;
    sk_ctx **ctx;
    skh_keyset *ks;
    const char *const *a, *const *o, *const *g;      /* o == NULL: ONE strain whose -o and -g are on the command line */
} sd_adoption;

static int sd_main_impl(int argc, char **argv, FILE *out, FILE *err, const sd_adoption *ad);

int skh_strain_detect_main(int argc, char **argv, FILE *out, FILE *err) { return sd_main_impl(argc, argv, out, err, NULL); }

/* strain_detect on a strain that is already resident: ctx holds its table (>= 6 columns), *ks its key set -- both are
 * taken over and released here -- and informative_path names the informative k-mer list (what -a would name).  argv: the
 * rest of a strain_detect command line (-B/-b/-c/-t/-g/-o, --coverage-depth ...), argv[0] ignored; -r and -a are implied.
 * The n = 1 case of skh_strain_detect_resident_many, with -o and -g taken from argv. */
int skh_strain_detect_resident(sk_ctx *ctx, skh_keyset *ks, const char *informative_path, int argc, char **argv, FILE *out, FILE *err)
{
    return skh_strain_detect_resident_many(1, &ctx, ks, &informative_path, NULL, NULL, argc, argv, out, err);
}

/* strain_detect -S on n strains that are already resident: ctx[s] holds strain s's table (>= 6 columns), ks[s] its key set --
 * all are taken over and released here, whatever happens -- informative[s] names its informative k-mer list (-a), hits[s]
 * its outfile (-o) and glist[s] (NULL, or glist itself NULL) its -g list.  argv: strain_detect's command line without -r, -a,
 * -o, -S, -g (-B/-b/-c/-t, --coverage-depth, --min-kmer-hits), argv[0] ignored.  The strains share the -S machinery: one decode
 * of the targets, union tables of SK_SD_GROUP strains, each --coverage-depth table at its strain's default path.  hits == NULL:
 * n must be 1, and -o (and -g) come from argv, as in skh_strain_detect_resident. */
int skh_strain_detect_resident_many(uint32_t n, sk_ctx **ctx, skh_keyset *ks, const char *const *informative, const char *const *hits,
                                    const char *const *glist, int argc, char **argv, FILE *out, FILE *err)
{
    sd_adoption ad;
    uint32_t s;
    int bad = !ctx || !ks || !informative || n == 0 || (!hits && n != 1);
    for (s = 0; !bad && s < n; s++) bad = !ctx[s] || !informative[s] || (hits && !hits[s]);
    if (bad) {
        for (s = 0; ctx && ks && s < n; s++) {           /* (taken over all the same: nothing is left to the caller) */
            if (ctx[s]) { skh_pack_cache_set(ctx[s], NULL, NULL); sk_ctx_destroy(ctx[s]); }
            ctx[s] = NULL;
            skh_keyset_free(&ks[s]);
        }
        fprintf(err, "strain_detect: no resident strains to adopt\n");
        return 1;
    }
    ad.n = n; ad.ctx = ctx; ad.ks = ks; ad.a = informative; ad.o = hits; ad.g = glist;
    return sd_main_impl(argc, argv, out, err, &ad);
}

/* the strains of a -S list (or the adopted ones), opened by worker threads, each strain start to finish on one of them;
 * their messages are replayed here in list order, up to the first failure (SK_THREADS, default: the usable CPUs, at most
 * 16).  paths: r, a, o, g of every strain.  Returns non-zero when a strain failed. */
static int sd_open_strains(sd_prog *p, uint32_t ns, char **paths, int adopted, FILE *out, FILE *err)
{
    long ncpu = sk_cpu_budget();
    int nth = getenv("SK_THREADS") ? atoi(getenv("SK_THREADS")) : (int)(ncpu < 1 ? 1 : ncpu > 16 ? 16 : ncpu), t;
    ks_pool kp;
    pthread_t th[16];
    uint32_t k, failed = 0;
    sk_ctxjob cj;
    /* the HIP runtime comes up (0.25-3 s) while the first key sets are built: the context opened here becomes the first
     * strain's -- every other sk_ctx_create then finds the runtime ready instead of all workers queueing up behind it */
    if (ns && !adopted) sk_ctxjob_start(&cj, sd_dev.phys[0]);
    memset(&kp, 0, sizeof kp);
    kp.jobs = (ks_job *)calloc(ns ? ns : 1, sizeof *kp.jobs);
    kp.njobs = ns;
    pthread_mutex_init(&kp.mu, NULL);
    pthread_cond_init(&kp.cv, NULL);
    for (k = 0; k < ns; k++) {
        ks_job *j = &kp.jobs[k];
        j->p = &p[k]; j->r = paths[4 * k]; j->a = paths[4 * k + 1]; j->o = paths[4 * k + 2]; j->g = paths[4 * k + 3];
        j->device = sd_dev.phys[sd_dev_of_strain(k)];
        j->cj = k == 0 && !adopted ? &cj : NULL;
        j->adopted = adopted;
    }
    if (nth > 16) nth = 16;
    if (nth < 1) nth = 1;
    if ((uint32_t)nth > ns) nth = (int)ns;
    for (t = 0; t < nth; t++) if (pthread_create(&th[t], NULL, sd_keyset_pool_thread, &kp)) break;
    nth = t;
    if (nth == 0) sd_keyset_pool_thread(&kp);     /* no thread could be started: open them here */
    for (k = 0; k < ns; k++) {
        ks_job *j = &kp.jobs[k];
        pthread_mutex_lock(&kp.mu);
        while (!j->done) pthread_cond_wait(&kp.cv, &kp.mu);
        pthread_mutex_unlock(&kp.mu);
        if (!failed) {
            if (j->out_buf && j->out_len) fwrite(j->out_buf, 1, j->out_len, out);
            if (j->err_buf && j->err_len) fwrite(j->err_buf, 1, j->err_len, err);
            failed = (uint32_t)j->failed;
        }
        free(j->out_buf); free(j->err_buf);
    }
    for (t = 0; t < nth; t++) pthread_join(th[t], NULL);
    pthread_mutex_destroy(&kp.mu);
    pthread_cond_destroy(&kp.cv);
    free(kp.jobs);
    return failed != 0;
}

/* a run that ends before its strains were opened: the adopted ones are released all the same */
static int sd_drop(sd_prog *p, uint32_t ns)
{
    uint32_t s;
    for (s = 0; p && s < ns; s++) sd_strain_close(&p[s]);
    free(p);
    return 1;
}

static int sd_main_impl(int argc, char **argv, FILE *out, FILE *err, const sd_adoption *ad)
{
    const char *a = NULL, *r = NULL, *b = NULL, *b2 = NULL, *B = NULL, *tt = NULL, *g = NULL, *o = NULL, *S = NULL, *env;
    int c, j, mode = SD_SE, status = 1, device = 0, n_S = 0, want_cov = 0, cov_only = 0;
    skzo_pool zpool;
    const char *cov_file = NULL, *tc_dir = NULL, *rg_file = NULL, *rg_window = NULL;
    const char *const *rg_genomes = sd_rg.genomes;       /* (adopted strains: theirs for this call only) */
    const uint32_t rg_ngenomes = sd_rg.ngenomes;
    skh_regions *rgs = NULL;
    int want_rg = 0, want_sp = 0, want_ps = 0, want_rc = 0, want_rp = 0;
    const char *rc_file = NULL, *rp_file = NULL;
    const char *sp_file = NULL, *sp_max = NULL, *ps_file = NULL, *th_file = NULL, *th_list = NULL;
    int want_th = 0, want_sw = 0, want_su = 0, want_sq = 0;
    const char *ra_file = NULL, *ra_list = NULL, *ra_seed = NULL;
    int want_ra = 0;
    const char *su_file = NULL, *sq_file = NULL;
    int want_bg = 0, want_bgs = 0;
    const char *bg_file = NULL, *bgs_file = NULL, *bg_max = NULL;
    const char *sw_file = NULL, *sw_classes = NULL;
    skc_classes *swc = NULL;
    uint32_t nswc = 0;
    long long cov_min = 1;
    double t_begin = 0;
    sd_prog *p = NULL;
    char **paths = NULL;
    uint32_t ns = 0, s, nrgs = 0;

    if (ad) {                                            /* the resident strains are ours from here, whatever happens */
        p = (sd_prog *)calloc(ad->n, sizeof *p);
        if (!p) { fprintf(err, "strain_detect: out of memory\n"); return 1; }
        for (s = 0; s < ad->n; s++) sd_strain_adopt(&p[s], ad->ctx[s], &ad->ks[s], out, err);
        for (s = 0; s < ad->n; s++) ad->ctx[s] = NULL;
        ns = ad->n;
    }

    /* Extension (not in the reference): "--coverage-depth[=FILE]" also writes the table that
     * scripts/coverage_depth.py -k <outfile> [-m N] would print (step 4 of the workflow), collected while the
     * hits are emitted; default FILE = outfile with ".kmer_hits.gz" replaced by ".coverage_depth".
     * "--min-kmer-hits N" is that script's -m.  Taken out of argv before getopt. */
    for (c = 1, j = 1; c < argc; c++) {
        if (!strncmp(argv[c], "--coverage-depth", 16) && (argv[c][16] == 0 || argv[c][16] == '=')) {
            want_cov = 1;
            cov_file = argv[c][16] ? argv[c] + 17 : NULL;
            continue;
        }
        /* "--coverage-only[=FILE]": that table and NO hit list -- -o only names the strain and the table's default path; the counts
         * stay on the device (sk_covacc) wherever the reads allow it */
        if (!strncmp(argv[c], "--coverage-only", 15) && (argv[c][15] == 0 || argv[c][15] == '=')) {
            cov_only = 1;
            cov_file = argv[c][15] ? argv[c] + 16 : NULL;
            continue;
        }
        /* "--coverage-regions[=FILE] [--region-window W]": next to either table, the same numbers per window of W bases of the
         * strain's records (default 100000; 0: per record), default FILE = outfile with ".kmer_hits.gz" replaced by ".coverage_regions" */
        if (!strncmp(argv[c], "--coverage-regions", 18) && (argv[c][18] == 0 || argv[c][18] == '=')) {
            want_rg = 1;
            rg_file = argv[c][18] ? argv[c] + 19 : NULL;
            continue;
        }
        if (!strcmp(argv[c], "--region-window") && c + 1 < argc) { rg_window = argv[++c]; continue; }
        if (!strncmp(argv[c], "--region-window=", 16)) { rg_window = argv[c] + 16; continue; }
        /* "--coverage-spectrum[=FILE] [--spectrum-max D]": next to either table, how many informative k-mers were seen 0, 1, ..., D and
         * more than D times (default D 255, at most 1023), default FILE = outfile with ".kmer_hits.gz" replaced by ".coverage_spectrum" */
        if (!strncmp(argv[c], "--coverage-spectrum", 19) && (argv[c][19] == 0 || argv[c][19] == '=')) {
            want_sp = 1;
            sp_file = argv[c][19] ? argv[c] + 20 : NULL;
            continue;
        }
        if (!strcmp(argv[c], "--spectrum-max") && c + 1 < argc) { sp_max = argv[++c]; continue; }
        if (!strncmp(argv[c], "--spectrum-max=", 15)) { sp_max = argv[c] + 15; continue; }
        /* "--coverage-thresholds[=FILE] [--threshold-list t1,t2,...]": next to either table, its two numbers at each of up to 16
         * --min-kmer-hits from the one pass (default list 0,1,2,3,5,10,20,50), default FILE = outfile with ".kmer_hits.gz" replaced
         * by ".coverage_thresholds" */
        if (!strncmp(argv[c], "--coverage-thresholds", 21) && (argv[c][21] == 0 || argv[c][21] == '=')) {
            want_th = 1;
            th_file = argv[c][21] ? argv[c] + 22 : NULL;
            continue;
        }
        /* "--coverage-rarefaction[=FILE] [--rarefaction-list f0,f1,...] [--rarefaction-seed S]": next to either table, the target's pairs
         * and its two numbers over nested subsamples of its read pairs, from the one pass (default list 1,0.5,0.25,0.125,0.0625,0.03125,
         * default seed 0), default FILE = outfile with ".kmer_hits.gz" replaced by ".coverage_rarefaction" */
        if (!strncmp(argv[c], "--coverage-rarefaction", 22) && (argv[c][22] == 0 || argv[c][22] == '=')) {
            want_ra = 1;
            ra_file = argv[c][22] ? argv[c] + 23 : NULL;
            continue;
        }
        if (!strcmp(argv[c], "--rarefaction-list") && c + 1 < argc) { ra_list = argv[++c]; continue; }
        if (!strncmp(argv[c], "--rarefaction-list=", 19)) { ra_list = argv[c] + 19; continue; }
        if (!strcmp(argv[c], "--rarefaction-seed") && c + 1 < argc) { ra_seed = argv[++c]; continue; }
        if (!strncmp(argv[c], "--rarefaction-seed=", 19)) { ra_seed = argv[c] + 19; continue; }
        if (!strcmp(argv[c], "--threshold-list") && c + 1 < argc) { th_list = argv[++c]; continue; }
        if (!strncmp(argv[c], "--threshold-list=", 17)) { th_list = argv[c] + 17; continue; }
        /* "--coverage-scrub-sweep[=FILE] [--scrub-classes FILE]": next to either table, its numbers at every min_fraction of the strain's
         * class file (kmer_scrub_filter --min_fraction_list; default the -a path plus ".classes") from the one pass, default FILE =
         * outfile with ".kmer_hits.gz" replaced by ".coverage_scrub_sweep" */
        if (!strncmp(argv[c], "--coverage-scrub-sweep", 22) && (argv[c][22] == 0 || argv[c][22] == '=')) {
            want_sw = 1;
            sw_file = argv[c][22] ? argv[c] + 23 : NULL;
            continue;
        }
        if (!strcmp(argv[c], "--scrub-classes") && c + 1 < argc) { sw_classes = argv[++c]; continue; }
        if (!strncmp(argv[c], "--scrub-classes=", 16)) { sw_classes = argv[c] + 16; continue; }
        /* "--coverage-recurrence[=FILE] [--recurrence-pairs[=FILE]]": next to either table, in how many of the run's samples each
         * informative k-mer was seen, and what every two samples share; default FILEs = outfile with ".kmer_hits.gz" replaced by
         * ".coverage_recurrence" and ".coverage_recurrence_pairs" */
        if (!strncmp(argv[c], "--coverage-recurrence", 21) && (argv[c][21] == 0 || argv[c][21] == '=')) {
            want_rc = 1;
            rc_file = argv[c][21] ? argv[c] + 22 : NULL;
            continue;
        }
        if (!strncmp(argv[c], "--recurrence-pairs", 18) && (argv[c][18] == 0 || argv[c][18] == '=')) {
            want_rp = 1;
            rp_file = argv[c][18] ? argv[c] + 19 : NULL;
            continue;
        }
        /* "--panel-share=FILE" (-S only): before the first target, the k-mers every ordered pair of the panel's strains share, one
         * table for the whole panel (sd_panel_share) */
        if (!strncmp(argv[c], "--panel-share", 13) && (argv[c][13] == 0 || argv[c][13] == '=')) {
            want_ps = 1;
            ps_file = argv[c][13] ? argv[c] + 14 : NULL;
            continue;
        }
        /* "--coverage-support[=FILE] [--support-pairs=FILE]": next to either table, the read pairs behind its numbers -- supporting pairs,
         * those with both mates, their lines -- default FILE = outfile with ".kmer_hits.gz" replaced by ".coverage_support"; with -S,
         * --support-pairs=FILE is one file for the panel: the pairs every two strains of a group share */
        if (!strncmp(argv[c], "--coverage-support", 18) && (argv[c][18] == 0 || argv[c][18] == '=')) {
            want_su = 1;
            su_file = argv[c][18] ? argv[c] + 19 : NULL;
            continue;
        }
        if (!strncmp(argv[c], "--support-pairs", 15) && (argv[c][15] == 0 || argv[c][15] == '=')) {
            want_sq = 1;
            sq_file = argv[c][15] ? argv[c] + 16 : NULL;
            continue;
        }
        /* "--coverage-background[=FILE] [--background-spectrum[=FILE]] [--background-max D]": next to either table, how much of ALL the
         * strain's k-mers each target holds and how deep, per class (informative, background); with the spectrum, per depth 0..D and
         * above (default D 63, at most 255); default FILEs = outfile with ".kmer_hits.gz" replaced by ".coverage_background" and
         * ".coverage_background_spectrum" */
        if (!strncmp(argv[c], "--coverage-background", 21) && (argv[c][21] == 0 || argv[c][21] == '=')) {
            want_bg = 1;
            bg_file = argv[c][21] ? argv[c] + 22 : NULL;
            continue;
        }
        if (!strncmp(argv[c], "--background-spectrum", 21) && (argv[c][21] == 0 || argv[c][21] == '=')) {
            want_bgs = 1;
            bgs_file = argv[c][21] ? argv[c] + 22 : NULL;
            continue;
        }
        if (!strcmp(argv[c], "--background-max") && c + 1 < argc) { bg_max = argv[++c]; continue; }
        if (!strncmp(argv[c], "--background-max=", 17)) { bg_max = argv[c] + 17; continue; }
        if (!strcmp(argv[c], "--min-kmer-hits") && c + 1 < argc) { cov_min = atoll(argv[++c]); continue; }
        if (!strcmp(argv[c], "--target-cache") && c + 1 < argc) { tc_dir = argv[++c]; continue; }       /* (extension: the target cache, see sd_tc) */
        if (!strncmp(argv[c], "--target-cache=", 15)) { tc_dir = argv[c] + 15; continue; }
        argv[j++] = argv[c];
    }
    argc = j;
    sd_rg.on = 0; sd_rg.genomes = NULL; sd_rg.ngenomes = 0;
    sd_spec.on = 0;
    sd_thr.on = 0;
    sd_rar.on = 0;
    sd_sw.on = 0;
    sd_rec.on = 0;
    sd_co.on = 0;
    sd_ps.path = NULL;
    sd_sup.on = 0; sd_sup.pairs_path = NULL;
    memset(&sd_bg, 0, sizeof sd_bg);
    if (cov_only && want_cov) { fputs("strain_detect: --coverage-only and --coverage-depth exclude each other (the table is the same; only one writes the hit list)\n", err); return sd_drop(p, ns); }

    optind = 1;
    while ((c = getopt(argc, argv, "g:r:a:A:b:c:B:S:M:o:t:Hhuspn")) != -1) {
        switch (c) {
        case 'a': a = optarg; break;
        case 'A': break;
        case 'b': b = optarg; break;
        case 'c': b2 = optarg; break;
        case 'B': B = optarg; break;
        case 'r': r = optarg; break;
        case 'g': g = optarg; break;
        case 'o': o = optarg; break;
        case 'n': mode = SD_SE; break;
        case 't': tt = optarg; break;
        case 'S': S = optarg; n_S++; break;              /* the reference prints its usage for -S and carries on; see below */
        default:  usage(err); break;
        }
    }
    /* Extension: "-S <file>" with NO -r/-a/-o runs several strains in one pass over the metagenomes.  Each
     * line of the file is  <reference genome> TAB <informative k-mer file> TAB <outfile> [TAB <-g list>];
     * every outfile gets exactly what a separate run with that line's -r/-a/-o[/-g] would write.  All
     * tables stay resident on the device; each metagenome is decoded and uploaded once. */
    if (ad && ad->o) {                                   /* many strains: their -r/-a/-o/-g are not on the command line */
        if (r || a || o || S || g) { fputs("strain_detect: the resident strains bring their own -r, -a, -o and -g\n", err); return sd_drop(p, ns); }
        if (cov_file) { fputs("strain_detect: --coverage-depth=FILE names one file; the resident strains each have their own\n", err); return sd_drop(p, ns); }
        o = ad->o[0];
    }
    if (cov_only) {
        if (cov_file && ((S && !a && !o && !r) || (ad && ad->o))) { fputs("strain_detect: --coverage-only=FILE names one file; with several strains each table goes to its default path\n", err); return sd_drop(p, ns); }
        if (!o && !S && !(ad && ad->o)) { fputs("strain_detect: --coverage-only needs -o: it names the strain and the table's default path (no hit list is written)\n", err); return sd_drop(p, ns); }
        want_cov = 1;
    }
    if (want_rg || rg_window) {
        long long w = 100000;
        char *end = NULL;
        if (!want_rg) { fputs("strain_detect: --region-window goes with --coverage-regions\n", err); return sd_drop(p, ns); }
        if (!want_cov) { fputs("strain_detect: --coverage-regions goes with --coverage-depth or --coverage-only: it folds their table's numbers by region\n", err); return sd_drop(p, ns); }
        if (rg_file && ((S && !a && !o && !r) || (ad && ad->o))) { fputs("strain_detect: --coverage-regions=FILE names one file; with several strains each table goes to its default path\n", err); return sd_drop(p, ns); }
        if (rg_window) {
            errno = 0;
            w = strtoll(rg_window, &end, 10);
            if (end == rg_window || *end || errno || w < 0) { fprintf(err, "strain_detect: --region-window %s: a number of bases, 0 or more (0: one region per record)\n", rg_window); return sd_drop(p, ns); }
        }
        if (!skh_regions_from_file || !skh_regions_free) { fputs("strain_detect: --coverage-regions: this build has no region table\n", err); return sd_drop(p, ns); }
        if (ad && (!rg_genomes || rg_ngenomes != ad->n)) { fputs("strain_detect: --coverage-regions: the resident strains' genome files are not known\n", err); return sd_drop(p, ns); }
        sd_rg.window = (uint64_t)w;
    }
    if (want_sp || sp_max) {
        long long d = 255;
        char *end = NULL;
        if (!want_sp) { fputs("strain_detect: --spectrum-max goes with --coverage-spectrum\n", err); return sd_drop(p, ns); }
        if (!want_cov) { fputs("strain_detect: --coverage-spectrum goes with --coverage-depth or --coverage-only: it bins their table's hits by depth\n", err); return sd_drop(p, ns); }
        if (sp_file && ((S && !a && !o && !r) || (ad && ad->o))) { fputs("strain_detect: --coverage-spectrum=FILE names one file; with several strains each table goes to its default path\n", err); return sd_drop(p, ns); }
        if (sp_max) {
            errno = 0;
            d = strtoll(sp_max, &end, 10);
            if (end == sp_max || *end || errno || d < 1 || d > (long long)SK_COVACC_SPECTRUM_MAX) { fprintf(err, "strain_detect: --spectrum-max %s: a depth from 1 to %u\n", sp_max, SK_COVACC_SPECTRUM_MAX); return sd_drop(p, ns); }
        }
        sd_spec.max = (uint32_t)d;
    }
    if (want_ra || ra_list || ra_seed) {
        unsigned long long seed = 0;
        char *end = NULL;
        if (!want_ra) { fprintf(err, "strain_detect: %s goes with --coverage-rarefaction\n", ra_list ? "--rarefaction-list" : "--rarefaction-seed"); return sd_drop(p, ns); }
        if (!want_cov) { fputs("strain_detect: --coverage-rarefaction goes with --coverage-depth or --coverage-only: it gives their table's two numbers over nested subsamples of the read pairs\n", err); return sd_drop(p, ns); }
        if (ra_file && ((S && !a && !o && !r) || (ad && ad->o))) { fputs("strain_detect: --coverage-rarefaction=FILE names one file; with several strains each table goes to its default path\n", err); return sd_drop(p, ns); }
        if (ad) { fputs("strain_detect: --coverage-rarefaction does not go behind kmer_scrub_count --detect\n", err); return sd_drop(p, ns); }
        if (!skh_rarefaction_parse || !skh_rarefaction_class || !skh_rarefaction_write) { fputs("strain_detect: --coverage-rarefaction: this build has no rarefaction table\n", err); return sd_drop(p, ns); }
        if (ra_seed) {
            errno = 0;
            seed = strtoull(ra_seed, &end, 10);
            if (end == ra_seed || *end || errno || seed > 0xFFFFFFFFull || ra_seed[0] == '-' || ra_seed[0] == '+' || ra_seed[0] == ' ') { fprintf(err, "strain_detect: --rarefaction-seed %s: an integer from 0 to 4294967295\n", ra_seed); return sd_drop(p, ns); }
        }
        if (skh_rarefaction_parse(ra_list, (uint32_t)seed, &sd_rar.r) != SK_OK) {
            fprintf(err, "strain_detect: --rarefaction-list %s: 1 to %u decimal fractions, 0 < f <= 1, strictly descending, no two of them equal in 32 bits\n", ra_list, SK_COVACC_RAREFACTION_MAX);
            return sd_drop(p, ns);
        }
    }
    if (want_th || th_list) {
        static const int64_t dflt[8] = { 0, 1, 2, 3, 5, 10, 20, 50 };
        char why[160];
        if (!want_th) { fputs("strain_detect: --threshold-list goes with --coverage-thresholds\n", err); return sd_drop(p, ns); }
        if (!want_cov) { fputs("strain_detect: --coverage-thresholds goes with --coverage-depth or --coverage-only: it gives their table's two numbers at several --min-kmer-hits\n", err); return sd_drop(p, ns); }
        if (th_file && ((S && !a && !o && !r) || (ad && ad->o))) { fputs("strain_detect: --coverage-thresholds=FILE names one file; with several strains each table goes to its default path\n", err); return sd_drop(p, ns); }
        memset(sd_thr.t, 0, sizeof sd_thr.t);
        memcpy(sd_thr.t, dflt, sizeof dflt);
        sd_thr.n = 8;
        if (th_list && skc_parse_threshold_list(th_list, sd_thr.t, &sd_thr.n, why, sizeof why)) { fprintf(err, "strain_detect: --threshold-list %s: %s\n", th_list, why); return sd_drop(p, ns); }
    }
    if (want_sw || sw_classes) {
        const int several = (S && !a && !o && !r) || (ad && ad->o);
        if (!want_sw) { fputs("strain_detect: --scrub-classes goes with --coverage-scrub-sweep\n", err); return sd_drop(p, ns); }
        if (!want_cov) { fputs("strain_detect: --coverage-scrub-sweep goes with --coverage-depth or --coverage-only: it gives their table's numbers at several min_fraction\n", err); return sd_drop(p, ns); }
        if ((sw_file || sw_classes) && several) { fputs("strain_detect: --coverage-scrub-sweep=FILE and --scrub-classes name one file; with several strains each table and class file is at its default path\n", err); return sd_drop(p, ns); }
        if (sw_classes && !*sw_classes) { fputs("strain_detect: --scrub-classes needs a file name\n", err); return sd_drop(p, ns); }
        if (g) { fprintf(err, "strain_detect: --coverage-scrub-sweep does not go with a -g list (%s): its cut is sized by the number of informative k-mers, so the fractions' sets would no longer be nested\n", g); return sd_drop(p, ns); }
    }
    if (want_rc || want_rp) {
        uint32_t T = 1;
        if (!want_rc) { fputs("strain_detect: --recurrence-pairs goes with --coverage-recurrence\n", err); return sd_drop(p, ns); }
        if (!want_cov) { fputs("strain_detect: --coverage-recurrence goes with --coverage-depth or --coverage-only: it follows their table's k-mers over the samples\n", err); return sd_drop(p, ns); }
        if ((rc_file || rp_file) && ((S && !a && !o && !r) || (ad && ad->o))) { fputs("strain_detect: --coverage-recurrence=FILE names one file; with several strains each table goes to its default path\n", err); return sd_drop(p, ns); }
        if (!sk_recur_create || !sk_recur_destroy || !sk_recur_finish || !sk_covacc_set_recurrence || !sk_covacc_mark_target) { fputs("strain_detect: --coverage-recurrence: this build has no recurrence engine\n", err); return sd_drop(p, ns); }
        if (B) {                                             /* the target lines of the run: its samples */
            FILE *fp = fopen(B, "r");
            char *line = NULL, *tok, *f1, *f2;
            size_t cap = 0;
            int m;
            for (T = 0; fp && getline(&line, &cap, fp) != -1; )
                if (sd_list_line(line, &m, &tok, &f1, &f2) == SD_LL_TARGET) T++;
            free(line);
            if (fp) fclose(fp);
            else T = 1;                                      /* (unreadable: the run says so) */
        }
        if (T > SK_RECUR_SAMPLES_MAX) { fprintf(err, "strain_detect: --coverage-recurrence: %s names %u targets, at most %u\n", B, T, SK_RECUR_SAMPLES_MAX); return sd_drop(p, ns); }
        if (want_rp && T > SK_RECUR_PAIRS_MAX) { fprintf(err, "strain_detect: --recurrence-pairs: %s names %u targets, at most %u\n", B, T, SK_RECUR_PAIRS_MAX); return sd_drop(p, ns); }
        sd_rec.T = T ? T : 1u;
    }
    if (want_su || want_sq) {
        const int several = (S && !a && !o && !r) || (ad && ad->o);
        const char *ws = getenv("SK_WORLD_SIZE") ? getenv("SK_WORLD_SIZE") : getenv("WORLD_SIZE");
        if (!want_su) { fputs("strain_detect: --support-pairs goes with --coverage-support\n", err); return sd_drop(p, ns); }
        if (!want_cov) { fputs("strain_detect: --coverage-support goes with --coverage-depth or --coverage-only: it counts the read pairs behind their table's numbers\n", err); return sd_drop(p, ns); }
        if (su_file && several) { fputs("strain_detect: --coverage-support=FILE names one file; with several strains each table goes to its default path\n", err); return sd_drop(p, ns); }
        if (!sks_create || !sks_merge || !sks_write_support || !sks_write_pairs) { fputs("strain_detect: --coverage-support: this build has no support accumulator\n", err); return sd_drop(p, ns); }
        if (want_sq) {
            if (!sq_file || !*sq_file) { fputs("strain_detect: --support-pairs=FILE needs a file name: the table is one file for the whole panel\n", err); return sd_drop(p, ns); }
            if (!several) { fputs("strain_detect: --support-pairs goes with -S: it compares the strains of a panel\n", err); return sd_drop(p, ns); }
            if (ws && atoi(ws) > 1) { fprintf(err, "strain_detect: --support-pairs is for ONE process: with WORLD_SIZE %d each rank holds only its own strains\n", atoi(ws)); return sd_drop(p, ns); }
            if (getenv("SK_SD_NO_UNION")) { fputs("strain_detect: --support-pairs compares the strains of a union table and SK_SD_NO_UNION is set: no pairs of the panel\n", err); return sd_drop(p, ns); }
        }
    }
    if (want_bg || want_bgs || bg_max) {
        const int several = (S && !a && !o && !r) || (ad && ad->o);
        long long d = 63;
        char *end = NULL;
        if (!want_bg) { fprintf(err, "strain_detect: %s goes with --coverage-background\n", want_bgs ? "--background-spectrum" : "--background-max"); return sd_drop(p, ns); }
        if (!want_cov) { fputs("strain_detect: --coverage-background goes with --coverage-depth or --coverage-only: it is the denominator their table's numbers are read against\n", err); return sd_drop(p, ns); }
        if ((bg_file || bgs_file) && several) { fputs("strain_detect: --coverage-background=FILE names one file; with several strains each table goes to its default path\n", err); return sd_drop(p, ns); }
        if (bg_max) {
            errno = 0;
            d = strtoll(bg_max, &end, 10);
            if (end == bg_max || *end || errno || d < 1 || d > (long long)SK_BACKGROUND_MAX_DEPTH) { fprintf(err, "strain_detect: --background-max %s: a depth from 1 to %u\n", bg_max, SK_BACKGROUND_MAX_DEPTH); return sd_drop(p, ns); }
        }
        if (ad) { fputs("strain_detect: --coverage-background does not go behind kmer_scrub_count --detect: the resident tables were loaded without its count column\n", err); return sd_drop(p, ns); }
        if (!sk_scan_batch || !sk_background_finish || !sk_union_background_finish || !sk_union_count_enable || !sk_union_context || !skb_create || !skb_destroy ||
            !skb_add || !skb_write || !skb_write_spectrum) { fputs("strain_detect: --coverage-background: this build has no background sweep\n", err); return sd_drop(p, ns); }
        if (B) {                                             /* breadth is not additive, and the device column is swept per target */
            FILE *fp = fopen(B, "r");
            char *line = NULL, **seen = NULL;
            size_t cap = 0;
            uint32_t nseen = 0, k;
            int shared = 0;
            while (fp && !shared && getline(&line, &cap, fp) != -1) {
                char *tok, *f1, *f2, **grown;
                int m;
                if (sd_list_line(line, &m, &tok, &f1, &f2) != SD_LL_TARGET) continue;
                if (strrchr(f1, '/')) f1 = strrchr(f1, '/') + 1;
                for (k = 0; k < nseen; k++) if (!strcmp(seen[k], f1)) shared = 1;
                if (!(grown = (char **)realloc(seen, ((size_t)nseen + 1) * sizeof *seen))) break;
                seen = grown;
                if (!(seen[nseen] = strdup(f1))) break;
                nseen++;
            }
            for (k = 0; k < nseen; k++) free(seen[k]);
            free(seen); free(line);
            if (fp) fclose(fp);
            if (shared) {
                fprintf(err, "strain_detect: --coverage-background: two targets of %s share a file name, the tables count them as one sample, and the "
                             "k-mers two files cover do not add up: run them apart\n", B);
                return sd_drop(p, ns);
            }
        }
        sd_bg.max = (uint32_t)d;
    }
    if (want_ps) {
        const char *ws = getenv("SK_WORLD_SIZE") ? getenv("SK_WORLD_SIZE") : getenv("WORLD_SIZE");
        if (!ps_file || !*ps_file) { fputs("strain_detect: --panel-share=FILE needs a file name: the table is one file for the whole panel\n", err); return sd_drop(p, ns); }
        if (!((S && !a && !o && !r) || (ad && ad->o))) { fputs("strain_detect: --panel-share goes with -S: it compares the strains of a panel\n", err); return sd_drop(p, ns); }
        if (!sk_union_share) { fputs("strain_detect: --panel-share: this build has no sk_union_share\n", err); return sd_drop(p, ns); }
        if (ws && atoi(ws) > 1) { fprintf(err, "strain_detect: --panel-share is for ONE process: with WORLD_SIZE %d each rank holds only its own strains\n", atoi(ws)); return sd_drop(p, ns); }
        if (!ad && (env = getenv("SK_DEVICES")) != NULL && *env) {     /* (several logical devices on ONE card are fine: SK_DEVICES=0,0) */
            int several = !strchr(env, ',') && atoi(env) > 1;
            const char *q = strchr(env, ',');
            for (; q && !several; q = strchr(q + 1, ',')) several = atoi(q + 1) != atoi(env);
            if (several) {
                fprintf(err, "strain_detect: --panel-share compares strains on ONE device and SK_DEVICES=%s names several: the table depends on the strains "
                             "only, take it in a one-device run\n", env);
                return sd_drop(p, ns);
            }
        }
    }
    if (ad) { a = ad->a[0]; r = "(resident)"; S = NULL; }
    if (S && !a && !o && !r) {
        if (!b && !B) { usage(err); return sd_drop(p, ns); }
    } else {
        S = NULL;
        while (n_S-- > 0) usage(err);
        if (!a || !o || !r) { usage(err); return sd_drop(p, ns); }
        if (!b && !B) { usage(err); return sd_drop(p, ns); }
    }
    if (tt) {
        mode = file_type(tt);
        if (mode == SD_UNKNOWN) { fputs("unknown filetype specification. allowed are SE, PE, PEI\n\n", out); usage(err); return sd_drop(p, ns); }
    }
    if (b && mode == SD_PE && !b2) {
        fputs("commandline PE mapping requires two files (-b [file1] and -c [file2])\n\n", out); usage(err); return sd_drop(p, ns);
    }
    if (b && B) {
        fputs("cannot have -B flag and -b flag\nEither have a file with metagenomics files to be detect the strain in or "
              "specify one metagenomic file to detect the strain in\n", out);
        usage(err); return sd_drop(p, ns);
    }
    if ((env = getenv("SK_DEVICE")) != NULL) device = atoi(env);
    sd_dev.n = 1; sd_dev.phys[0] = device;
    sd_group = SK_UNION_MAX;
    if ((env = getenv("SK_SD_GROUP")) != NULL && atoi(env) >= 1 && atoi(env) <= SK_UNION_MAX) sd_group = (uint32_t)atoi(env);
    memset(sd_dev.ctx, 0, sizeof sd_dev.ctx);
    t_begin = now_s();
    sd_co.on = cov_only; sd_co.min = cov_min;
    sd_co_ms_fold = sd_co_ms_sweep = 0;
    sd_rg.on = want_rg;
    sd_spec.on = want_sp;
    sd_thr.on = want_th; sd_thr.ms_finish = 0;
    sd_rar.on = want_ra; sd_rar.named = S != NULL; sd_rar.min = cov_min; sd_rar.ms_class = sd_rar.ms_finish = 0;
    sd_sw.on = want_sw; sd_sw.ms_cls = 0;
    sd_rec.on = want_rc; sd_rec.pairs = want_rp; sd_rec.next = 0;
    sd_rec.ms_mark = sd_rec.ms_hist = sd_rec.ms_gram = 0;
    sd_ps.path = want_ps ? ps_file : NULL;
    sd_ps.ms = 0; sd_ps.calls = 0;
    sd_sup.on = want_su; sd_sup.pairs_path = want_sq ? sq_file : NULL; sd_sup.acc = NULL; sd_sup.ms_take = sd_sup.ms_finish = 0;
    sd_bg.on = want_bg;
    sd_co.flush_rows = (env = getenv("SK_SD_CO_FLUSH_ROWS")) != NULL && atoll(env) >= 1 ? (uint64_t)atoll(env) : 1u << 20;
    sd_res_bytes = 0;
    sd_tc_open(tc_dir, err);
    n_text_taken = n_text_declined = 0;                  /* (per run: the library entry points may be called again in one process) */
    {
        const long ncpu = sk_cpu_budget();
        skzo_pool_start(&zpool, getenv("SK_THREADS") ? atoi(getenv("SK_THREADS")) : (int)(ncpu > 16 ? 16 : ncpu < 1 ? 1 : ncpu));
        sd_zpool = &zpool;
    }

    if (S) {
        FILE *fp = fopen(S, "r");
        char *line = NULL;
        size_t cap = 0;
        const int world = getenv("SK_WORLD_SIZE") ? atoi(getenv("SK_WORLD_SIZE")) : (getenv("WORLD_SIZE") ? atoi(getenv("WORLD_SIZE")) : 1);
        const int rank = getenv("SK_RANK") ? atoi(getenv("SK_RANK")) : (getenv("RANK") ? atoi(getenv("RANK")) : 0);
        unsigned lineno = 0;
        if (!fp) { fprintf(err, "strain_detect: could not read the strain list %s\n", S); goto done; }
        if (!getenv("SK_DEVICE") && (env = getenv("SK_LOCAL_RANK") ? getenv("SK_LOCAL_RANK") : getenv("LOCAL_RANK")) != NULL) device = atoi(env);
        sd_dev.phys[0] = device;
        if ((env = getenv("SK_DEVICES")) != NULL && *env) {      /* one process, several devices: see sd_dev */
            if (world > 1) { fprintf(err, "strain_detect: SK_DEVICES is for ONE process that drives several devices (WORLD_SIZE is %d)\n", world); fclose(fp); goto done; }
            if (strchr(env, ',')) {                               /* the devices as listed (several logical devices may share a card) */
                const char *q = env;
                sd_dev.n = 0;
                while (*q && sd_dev.n < SD_MAX_DEV) {
                    sd_dev.phys[sd_dev.n++] = atoi(q);
                    while (*q && *q != ',') q++;
                    if (*q == ',') q++;
                }
            } else {
                int k;
                sd_dev.n = atoi(env);
                if (sd_dev.n < 1 || sd_dev.n > SD_MAX_DEV) { fprintf(err, "strain_detect: SK_DEVICES must be 1..%d or a list of devices\n", SD_MAX_DEV); fclose(fp); goto done; }
                for (k = 0; k < sd_dev.n; k++) sd_dev.phys[k] = device + k;
            }
        }
        while (getline(&line, &cap, fp) != -1) {
            char *nl, *fr, *fa, *fo, *fg;
            if ((nl = strchr(line, '\n')) != NULL) *nl = '\0';
            if (line[0] == '#' || line[0] == '\0') continue;
            if (world > 1 && (int)(lineno++ % (unsigned)world) != rank) continue;     /* strains are dealt to the ranks; no collective */
            fr = strtok(line, "\t"); fa = strtok(NULL, "\t"); fo = strtok(NULL, "\t"); fg = strtok(NULL, "\t");
            if (!fr || !fa || !fo) { fprintf(err, "strain_detect: %s: a line needs <genome> TAB <informative k-mers> TAB <outfile>\n", S); free(line); fclose(fp); goto done; }
            p = (sd_prog *)realloc(p, ((size_t)ns + 1) * sizeof *p);
            paths = (char **)realloc(paths, ((size_t)ns + 1) * 4 * sizeof *paths);
            memset(&p[ns], 0, sizeof *p);
            p[ns].out = out; p[ns].err = err;
            paths[4 * ns] = strdup(fr); paths[4 * ns + 1] = strdup(fa); paths[4 * ns + 2] = strdup(fo); paths[4 * ns + 3] = fg ? strdup(fg) : NULL;
            ns++;
        }
        free(line);
        fclose(fp);
        {   /* no more devices than there are groups of strains */
            const uint32_t ng = (ns + sd_group - 1) / sd_group;
            if ((uint32_t)sd_dev.n > ng) sd_dev.n = ng ? (int)ng : 1;
        }
        if (want_rg && ns) {                             /* (before any strain or target is opened: a refusal leaves nothing behind) */
            if (!(rgs = (skh_regions *)calloc(ns, sizeof *rgs))) { fprintf(err, "strain_detect: out of memory\n"); goto done; }
            for (nrgs = 0; nrgs < ns; nrgs++) if (sd_regions_load(&rgs[nrgs], paths[4 * nrgs], err)) goto done;
        }
        if (want_sw && ns) { nswc = ns; if (sd_sweep_load(&swc, ns, paths, NULL, err)) goto done; }
        if (sd_open_strains(p, ns, paths, 0, out, err)) goto done;
        if (ns == 0) { status = 0; goto done; }          /* nothing dealt to this rank */
    } else if (ad) {                                     /* (sd_dev: one device, the one the strains are on) */
        paths = (char **)calloc((size_t)ns * 4, sizeof *paths);
        for (s = 0; s < ns; s++) {
            paths[4 * s + 1] = strdup(ad->a[s]);
            paths[4 * s + 2] = strdup(ad->o ? ad->o[s] : o);
            paths[4 * s + 3] = ad->o ? (ad->g && ad->g[s] ? strdup(ad->g[s]) : NULL) : (g ? strdup(g) : NULL);
        }
        if (want_rg) {
            if (!(rgs = (skh_regions *)calloc(ns, sizeof *rgs))) { fprintf(err, "strain_detect: out of memory\n"); goto done; }
            for (nrgs = 0; nrgs < ns; nrgs++) if (sd_regions_load(&rgs[nrgs], rg_genomes[nrgs], err)) goto done;
        }
        if (want_sw) { nswc = ns; if (sd_sweep_load(&swc, ns, paths, ad->o ? NULL : sw_classes, err)) goto done; }
        if (sd_open_strains(p, ns, paths, 1, out, err)) goto done;
    } else {
        if (want_rg) {
            if (!(rgs = (skh_regions *)calloc(1, sizeof *rgs))) { fprintf(err, "strain_detect: out of memory\n"); goto done; }
            if (sd_regions_load(&rgs[0], r, err)) goto done;
            nrgs = 1;
        }
        if (want_sw) {                                   /* (before the strain is opened: a refusal leaves nothing behind) */
            char *one[4] = { NULL, (char *)a, NULL, NULL };
            nswc = 1;
            if (sd_sweep_load(&swc, 1, one, sw_classes, err)) goto done;
        }
        p = (sd_prog *)malloc(sizeof *p);
        ns = 1;
        if (sd_strain_open(&p[0], r, a, g, o, device, out, err)) goto done;
    }
    t_setup = now_s() - t_begin;
    for (s = ns; s-- > 0; ) sd_dev.ctx[sd_dev_of_strain(s)] = p[s].ctx;       /* a context on every device (its first strain's): owner of the device's batches */
    if (getenv("SK_SD_TIMING") && sd_dev.n > 1) fprintf(err, "strain_detect timing: %u strains on %d devices, one decode pipeline\n", ns, sd_dev.n);
    for (s = 0; want_cov && s < ns; s++)
        if (sd_coverage_open(&p[s], S ? NULL : cov_file, cov_min)) goto done;
    for (s = 0; want_rg && s < ns; s++)
        if (sd_regions_open(&p[s], &rgs[s], S || (ad && ad->o) ? NULL : rg_file)) goto done;
    for (s = 0; want_sp && s < ns; s++)
        if (sd_spectrum_open(&p[s], S || (ad && ad->o) ? NULL : sp_file)) goto done;
    for (s = 0; want_th && s < ns; s++)
        if (sd_thresholds_open(&p[s], S || (ad && ad->o) ? NULL : th_file)) goto done;
    for (s = 0; want_ra && s < ns; s++) {
        p[s].ra_path = sd_table_path(p[s].o_path, S || (ad && ad->o) ? NULL : ra_file, ".coverage_rarefaction");
        p[s].ra_f = p[s].ra_path ? open_memstream(&p[s].ra_buf, &p[s].ra_len) : NULL;
        if (!p[s].ra_f || skh_rarefaction_write(p[s].ra_f, &sd_rar.r, S ? "" : NULL, NULL, NULL, NULL, NULL) != SK_OK) { fprintf(err, "strain_detect: out of memory\n"); goto done; }
    }
    for (s = 0; want_sw && s < ns; s++)
        if (sd_sweep_open(&p[s], &swc[s], S || (ad && ad->o) ? NULL : sw_file)) goto done;
    for (s = 0; want_su && s < ns; s++)
        if (!(p[s].su_path = sd_table_path(p[s].o_path, S || (ad && ad->o) ? NULL : su_file, ".coverage_support"))) { fprintf(err, "strain_detect: out of memory\n"); goto done; }
    for (s = 0; want_rc && s < ns; s++)
        if (sd_recurrence_open(&p[s], S || (ad && ad->o) ? NULL : rc_file, S || (ad && ad->o) ? NULL : rp_file)) goto done;
    for (s = 0; want_bg && s < ns; s++) {
        const int own = S || (ad && ad->o);
        p[s].bg_path = sd_table_path(p[s].o_path, own ? NULL : bg_file, ".coverage_background");
        p[s].bgs_path = want_bgs ? sd_table_path(p[s].o_path, own ? NULL : bgs_file, ".coverage_background_spectrum") : NULL;
        p[s].bg = skb_create(sd_bg.max);
        if (!p[s].bg_path || (want_bgs && !p[s].bgs_path) || !p[s].bg) { fprintf(err, "strain_detect: out of memory\n"); goto done; }
    }
    if ((c = sd_run(p, ns, B, b, b2, mode, out, err)) != 0) { if (c == SK_E_CACHE) status = SK_E_CACHE; goto done; }
    for (s = 0; s < ns; s++)
        if (sd_coverage_write(&p[s])) goto done;
    for (s = 0; want_bg && s < ns; s++)
        if (sd_background_write(&p[s])) goto done;
    if (sd_sup.acc && sd_support_write(p, ns)) goto done;
    status = 0;
done:
    if (getenv("SK_SD_TIMING") && ns > 1)
        fprintf(err, "strain_detect timing: opening the strains, thread time summed: context %.2f s, table load %.2f s, -a/-g flags + outfile %.2f s\n",
                t_open_ctx, t_open_load, t_open_flags);
    if (getenv("SK_SD_TIMING"))
        fprintf(err, "strain_detect timing: setup %.2f s, waiting for the decode thread %.2f s, tally %.2f s (upload %.2f, launch + collect %.2f, "
                     "posting to the lanes %.2f), read lengths %.2f s, posting the runs %.2f s, waiting for the lanes at the files' ends %.2f s "
                     "(and %.2f s for room in a lane's ring), chunks freed %.2f s, files opened %.2f s and closed %.2f s, union tables freed %.2f s, "
                     "total before close %.2f s; lanes' busy time, summed: %.2f s (sort + spread + replay + compression hand-over)\n",
                t_setup, t_wait, t_tally, t_fill, t_launch, t_post, t_lens, t_replay, t_lane_drain, t_lane_backpressure, t_cfree, t_sopen, t_sclose,
                t_uclose, now_s() - t_begin, t_lane_busy);
    if (getenv("SK_SD_TIMING")) {                        /* who used the CPUs: the process as a whole against the threads this file starts */
        struct rusage ru;
        if (getrusage(RUSAGE_SELF, &ru) == 0)
            fprintf(err, "strain_detect timing: CPU time of the process: user %.1f s + system %.1f s; of it parser threads %.1f s, reader threads %.1f s, "
                         "lanes %.1f s, this (main) thread %.1f s -- the rest is the output compressors, the HIP runtime's own threads and the strains' opening\n",
                    (double)ru.ru_utime.tv_sec + 1e-6 * (double)ru.ru_utime.tv_usec, (double)ru.ru_stime.tv_sec + 1e-6 * (double)ru.ru_stime.tv_usec,
                    cpu_parsers, cpu_readers, cpu_lanes, thread_cpu_s());
    }
    if (getenv("SK_SD_TIMING")) {                        /* ... and the threads that are still there (the runtime's, the compressors', the lanes'), by name */
        DIR *td = opendir("/proc/self/task");
        struct dirent *de;
        const double tick = 1.0 / (double)sysconf(_SC_CLK_TCK);
        while (td && (de = readdir(td)) != NULL) {
            char path[300], buf[1024], *rp;
            FILE *tf;
            unsigned long ut = 0, stt = 0;
            if (de->d_name[0] == '.') continue;
            snprintf(path, sizeof path, "/proc/self/task/%s/stat", de->d_name);
            if (!(tf = fopen(path, "r"))) continue;
            if (fgets(buf, sizeof buf, tf) && (rp = strrchr(buf, ')')) != NULL &&
                sscanf(rp + 2, "%*c %*d %*d %*d %*d %*d %*u %*u %*u %*u %*u %lu %lu", &ut, &stt) == 2 && (double)(ut + stt) * tick >= 0.5) {
                *rp = 0;
                fprintf(err, "strain_detect timing: thread %s (%s: user %.1f s, system %.1f s\n", de->d_name, strchr(buf, '(') ? strchr(buf, '(') + 1 : "?",
                        (double)ut * tick, (double)stt * tick);
            }
            fclose(tf);
        }
        if (td) closedir(td);
    }
    if (getenv("SK_SD_TIMING")) {                        /* was the process held back by its CPU quota?  (cgroup v2: cpu.stat of the job's group) */
        FILE *cs = fopen("/sys/fs/cgroup/cpu.stat", "r");
        char ln[128];
        while (cs && fgets(ln, sizeof ln, cs))
            if (!strncmp(ln, "nr_throttled", 12) || !strncmp(ln, "throttled_usec", 14) || !strncmp(ln, "usage_usec", 10)) {
                ln[strcspn(ln, "\n")] = 0;
                fprintf(err, "strain_detect timing: cgroup cpu.stat %s (since the group began)\n", ln);
            }
        if (cs) fclose(cs);
    }
    if (getenv("SK_SD_TIMING"))
        fprintf(err, "strain_detect timing: page-locked chunk buffers: %d of at most %d made (%zu bytes each), %lu chunks had to do without one\n",
                sd_pin.total, SD_PIN_MAX, sd_pin.bytes, n_unpinned_chunks);
    if (getenv("SK_SD_TIMING") && (n_text_taken || n_text_declined || sd_text_wanted()))
        fprintf(err, "strain_detect timing: text pieces parsed on the device: %lu taken, %lu declined (the host parsed the rest of their files)\n", n_text_taken, n_text_declined);
    if (getenv("SK_SD_TIMING") && t_pw_parse > 0)
        fprintf(err, "strain_detect timing: parser threads, summed: parsing %.2f s, waiting for a segment %.2f s, for their turn to hand chunks on %.2f s, for room in the queue %.2f s\n",
                t_pw_parse, t_pw_seg, t_pw_turn, t_pw_push);
    if (getenv("SK_SD_TIMING") && cov_only)
        fprintf(err, "strain_detect timing: coverage accumulators on the device: folds %.3f ms, target sweeps %.3f ms%s\n", sd_co_ms_fold, sd_co_ms_sweep,
                want_rg && want_sp ? " (folded by region, binned by depth)" : want_rg ? " (folded by region)" : want_sp ? " (binned by depth)" : "");
    if (getenv("SK_SD_TIMING") && cov_only && want_th)
        fprintf(err, "strain_detect timing: thresholds on the device: %u thresholds, finishing passes %.3f ms (the folds above classify as well)\n",
                sd_thr.n, sd_thr.ms_finish);
    if (getenv("SK_SD_TIMING") && cov_only && want_ra)
        fprintf(err, "strain_detect timing: rarefaction on the device: %u fractions, classifying passes %.3f ms (inside the folds above), finishing passes %.3f ms\n",
                sd_rar.r.n, sd_rar.ms_class, sd_rar.ms_finish);
    if (getenv("SK_SD_TIMING") && cov_only && want_sw)
        fprintf(err, "strain_detect timing: scrub sweep on the device: class passes %.3f ms\n", sd_sw.ms_cls);
    if (getenv("SK_SD_TIMING") && cov_only && want_rc)
        fprintf(err, "strain_detect timing: recurrence on the device: marks %.3f ms (%u targets), finish: histogram %.3f ms, pairs %.3f ms\n",
                sd_rec.ms_mark, sd_rec.T, sd_rec.ms_hist, sd_rec.ms_gram);
    if (getenv("SK_SD_TIMING") && cov_only && want_su)
        fprintf(err, "strain_detect timing: support on the device: takes %.3f ms (inside the folds above), finishes %.3f ms\n", sd_sup.ms_take, sd_sup.ms_finish);
    if (getenv("SK_SD_TIMING") && want_bg)
        fprintf(err, "strain_detect timing: background: %llu count scans beside the TALLY launches, finishing sweeps %.3f ms (wall time of the calls)\n",
                (unsigned long long)sd_bg.scans, sd_bg.ms_sweep);
    if (getenv("SK_SD_TIMING") && want_ps)
        fprintf(err, "strain_detect timing: panel share %.3f ms, %u call(s) of sk_union_share\n", sd_ps.ms, sd_ps.calls);
    if (getenv("SK_SD_RESULT_BYTES"))
        fprintf(err, "strain_detect: scan results copied from the device: %llu bytes; --coverage-only: %llu runs counted on the device, %llu replayed, "
                     "%llu targets on the host accumulator (the process's totals)\n", (unsigned long long)sd_res_bytes,
                (unsigned long long)sd_co_dev, (unsigned long long)sd_co_replayed, (unsigned long long)sd_co_hostacc);
    sd_tc_close(err);
    sd_pin_close();
    sd_co.on = 0;
    sd_rg.on = 0;
    sd_spec.on = 0;
    sd_thr.on = 0;
    sd_rar.on = 0;
    sd_sw.on = 0;
    sd_rec.on = 0;
    sd_ps.path = NULL;
    sd_bg.on = 0;
    if (sd_sup.acc) sks_destroy(sd_sup.acc);
    sd_sup.acc = NULL; sd_sup.on = 0; sd_sup.pairs_path = NULL;
    sd_sweep_drop(swc, nswc);
    for (s = 0; rgs && s < nrgs; s++) skh_regions_free(&rgs[s]);
    free(rgs);
    {   /* closing a strain = finishing its gz output, freeing its device context and tables: strain by strain on threads */
        sd_pool cp;
        const double t0 = now_s();
        pool_start(&cp, ns);
        pool_run(&cp, ns, close_one, p);
        pool_stop(&cp);
        t_close = now_s() - t0;
        if (getenv("SK_SD_TIMING")) fprintf(err, "strain_detect timing: closing the strains %.2f s\n", t_close);
    }
    skzo_pool_stop(&zpool);
    sd_zpool = NULL;
    for (s = 0; paths && s < 4 * ns; s++) free(paths[s]);
    free(paths);
    free(p);
    return status;
}
