/* sk_input.h -- getting an input file's text to the record parser (internal; header-only like sk_parser.h): SK_READ_BLOCK, the exact
 * pread, a span of a plain file fed by one of three ways under ONE rule for a way that fails, and the cutter of inflated text.  Shared by
 * the list scan (sk_host.c) and strain_detect (sk_host_sd.c); tests/native/input_check.c checks it on its own. */
#ifndef SK_INPUT_H
#define SK_INPUT_H
#include <errno.h>
#include <sys/mman.h>
#include <unistd.h>
#include "sk_parser.h"

/* SK_READ_BLOCK: 64 bytes (tests) .. 32 MiB; anything else, or unset: the caller's default */
static inline size_t ski_read_block(size_t dflt)
{
    const char *e = getenv("SK_READ_BLOCK");
    const long long v = e ? atoll(e) : 0;
    return v >= 64 && v <= (32 << 20) ? (size_t)v : dflt;
}

/* bytes [off, off + n) of fd into buf: how many were got -- fewer than n at the file's end or after an error */
static inline size_t ski_pread_exact(int fd, void *buf, size_t n, uint64_t off)
{
    size_t have = 0;
    while (have < n) {
        const ssize_t r = pread(fd, (unsigned char *)buf + have, n - have, (off_t)(off + have));
        if (r < 0 && errno == EINTR) continue;
        if (r <= 0) break;
        have += (size_t)r;
    }
    return have;
}

/* ---- a span of a plain file into the parser ---------------------------------------------------------------------------------
 * Three ways to get at the bytes, measured in round 4 with many threads at once (sixteen decode threads of the list scan on 1,670 plain
 * files, BASELINE configs[2]; twelve parser threads of strain_detect on the segments of one file, configs[4]'s share pass):
 *   SKI_POPULATE (default)  the span's pages are put into the address space by ONE call (MADV_POPULATE_READ: no trap per 64 KiB of
 *       text), parsed where they lie in the file's mapping, and taken out again by one call (MADV_DONTNEED).  No copy, the address
 *       space's lock is only ever taken for READING, and the file's munmap finds nothing to tear down.  strain_detect: 3.5-3.6 s,
 *       40 CPU-seconds (profiles/r04_cfg5_populate.json); list scan: 2.38-2.66 s against 2.69-2.80 s with read(), 31-34 CPU-seconds
 *       against 35-37.
 *   SKI_PREAD   copied into a block of the thread's own, small enough to stay in the core's cache between the copy and the parse:
 *       3.9-4.1 s, 48 CPU-seconds (profiles/r04_cfg5_pread.json, r04_cfg5_read_blocks.json).  A sampling of the program counter has
 *       59 % of a strain_detect parser thread's time, and 56 % of a list-scan decode thread's, inside the kernel's copy
 *       (tools/probes/sigprof_preload.c, profiles/r04_sigprof.txt).
 *   SKI_MAPPED  parsed out of the mapping, every page faulted in where it is first touched: 5.1-6.7 s; in the list scan the threads
 *       spend 31 s on a core and 37 s asleep in page faults (profiles/r04_cfg3_where.txt: scans 4.6 s against 3.4 s).  Not the faults
 *       themselves: a file's munmap tears its page-table entries down (2.7 M of them) under the address space's lock for WRITING, and
 *       the other threads' faults wait a third of a second for it, file after file.
 * The rule, the same for every caller (*mode is shared between threads: relaxed atomics only):
 *   POPULATE  populate the span rounded OUT to pages, feed it in place, drop the whole pages INSIDE it only (a neighbour thread may
 *             still be reading those at its ends).  A populate that fails sends THIS span the PREAD way, whatever the reason; EINVAL
 *             (no such advice before 5.14) also latches *mode to SKI_PREAD.  Built without MADV_POPULATE_READ, POPULATE is PREAD.
 *   PREAD     blocks of `block` bytes into rb (made here when first needed; the thread's own, freed by the caller).  A block that
 *             cannot be read whole is fed out of the mapping; without one (map == NULL: always PREAD) what was read is fed and
 *             SKI_SHORT ends the span.
 *   MAPPED    fed out of the mapping.
 * Between blocks (POPULATE and MAPPED: the span is one block) a stopped parser or a set *cancel (may be NULL) ends the span. */
enum { SKI_POPULATE = 0, SKI_PREAD = 1, SKI_MAPPED = 2 };
enum { SKI_FED = 0, SKI_SHORT = 1, SKI_NOMEM = -1 };      /* (NOMEM: no block and no mapping -- nothing was fed) */
typedef struct { unsigned char *buf; size_t cap; } ski_rbuf;

static inline int ski_feed_span(parser *ps, const unsigned char *map, int fd, uint64_t off, size_t n, int *mode,
                                ski_rbuf *rb, size_t block, const volatile int *cancel)
{
    int m = map ? __atomic_load_n(mode, __ATOMIC_RELAXED) : SKI_PREAD;
    size_t done = 0;
    if (!n || ps->state == P_STOP || (cancel && *cancel)) return SKI_FED;
    if (m == SKI_POPULATE) {
#ifdef MADV_POPULATE_READ
        const uintptr_t a = (uintptr_t)(map + off), pg = 4095u;
        if (madvise((void *)(a & ~pg), (size_t)(((a + n + pg) & ~pg) - (a & ~pg)), MADV_POPULATE_READ) == 0) {
            const uintptr_t da = (a + pg) & ~pg, de = (a + n) & ~pg;
            parser_feed(ps, map + off, n);
            if (de > da) (void)madvise((void *)da, (size_t)(de - da), MADV_DONTNEED);
            return SKI_FED;
        }
        if (errno == EINVAL) __atomic_store_n(mode, SKI_PREAD, __ATOMIC_RELAXED);
#endif
        m = SKI_PREAD;
    }
    if (m == SKI_PREAD && fd >= 0) {
        if (!rb->buf && (rb->buf = (unsigned char *)malloc(block)) != NULL) rb->cap = block;
        if (!rb->buf && !map) return SKI_NOMEM;
        while (done < n && ps->state != P_STOP && !(cancel && *cancel)) {
            const size_t want = !rb->buf || n - done < rb->cap ? n - done : rb->cap;
            const size_t have = rb->buf ? ski_pread_exact(fd, rb->buf, want, off + done) : 0;
            if (have == want) parser_feed(ps, rb->buf, want);
            else if (map) parser_feed(ps, map + off + done, want);               /* (a failed read: out of the mapping) */
            else { if (have) parser_feed(ps, rb->buf, have); return SKI_SHORT; }
            done += want;
        }
        return SKI_FED;
    }
    if (!map) return SKI_SHORT;
    parser_feed(ps, map + off, n);
    return SKI_FED;
}

/* ---- inflated text cut into segments -------------------------------------------------------------------------------------------
 * The text of a .gz file comes in deliveries of any size.  The cutter gathers it and hands out segments of about `want` bytes, each
 * ending at the first line start behind `want` bytes that looks like a record start (parser_guess_start; the guess wants two more
 * lines of text behind it, hence `tail` bytes of look-behind before a cut is looked for).  None so far -- very long records -- and
 * it keeps gathering, looking only at what it has not looked at yet.  A segment is a malloc'ed buffer that the consumer frees; what
 * lies behind the cut is carried into a fresh one.  Nothing is trusted from the guess: whoever parses a segment checks that it ends
 * between two records (parser_between_records). */
typedef struct { unsigned char *buf; size_t n, cap, want, tail, scan_from; } ski_cutter;

/* a fresh gathering buffer with room for `keep` carried bytes */
static inline void ski_cutter_fresh(ski_cutter *c, size_t keep)
{
    c->cap = c->want + (c->want >> 2) + ((size_t)1 << 20);          /* (a segment, the look-behind, one delivery of the inflate) */
    if (c->cap < keep) c->cap = keep * 2;
    c->buf = (unsigned char *)malloc(c->cap);
    c->n = 0;
    c->scan_from = c->want;
}

/* text wanted behind `want` bytes before a cut is looked for (also by who cuts a mapped file, where nothing is gathered) */
static inline size_t ski_cut_tail(size_t want) { return want / 2 < (64u << 10) ? (want / 2 < 256 ? 256 : want / 2) : (64u << 10); }

static inline void ski_cutter_init(ski_cutter *c, size_t want)
{
    c->want = want;
    c->tail = ski_cut_tail(want);
    ski_cutter_fresh(c, 0);
}

static inline void ski_cutter_add(ski_cutter *c, const unsigned char *data, size_t n)
{
    if (c->n + n > c->cap) { c->cap = (c->n + n) * 2; c->buf = (unsigned char *)realloc(c->buf, c->cap); }
    memcpy(c->buf + c->n, data, n);
    c->n += n;
}

/* 1: *buf, *n is a finished segment (a delivery may hold several: call again); 0: none yet */
static inline int ski_cutter_take(ski_cutter *c, unsigned char **buf, size_t *n)
{
    unsigned char *const old = c->buf;
    size_t cut, rest;
    if (c->n < c->want + c->tail) return 0;
    cut = (size_t)parser_guess_start(old, c->n, c->scan_from, 0);
    if (cut >= c->n) { c->scan_from = c->n - c->tail; return 0; }
    rest = c->n - cut;
    ski_cutter_fresh(c, rest);
    memcpy(c->buf, old + cut, rest);
    c->n = rest;
    *buf = old;
    *n = cut;
    return 1;
}

/* the text is over: what is left is the last segment (the cutter holds nothing afterwards) */
static inline void ski_cutter_rest(ski_cutter *c, unsigned char **buf, size_t *n) { *buf = c->buf; *n = c->n; c->buf = NULL; c->n = c->cap = 0; }

#endif
