/* input_check.c -- strainer2_amd/csrc/sk_input.h on its own (built under ASan/UBSan and run by tests/test_input_host.py).
 *   input_check span FILE   ski_feed_span: the whole file and a fixed list of spans whose ends lie on, one before and one behind page
 *                           boundaries, by each of the three ways and three read blocks, must hand the parser what ONE parser_feed of
 *                           the same bytes out of a plain memory copy hands it -- records and end state; then the short read without a
 *                           mapping, and a cancel set beforehand
 *   input_check cut FILE    ski_cutter with want = 300: the text delivered in pieces of six sizes, segments taken in a `while` (the
 *                           list scan) and once per delivery (strain_detect)
 * Prints MISMATCH and exits non-zero on any difference. */
#define _GNU_SOURCE
#include <fcntl.h>
#include <stdio.h>
#include <sys/stat.h>
#include "../../strainer2_amd/csrc/sk_parser.h"
#include "../../strainer2_amd/csrc/sk_input.h"

static int bad;
#define CHECK(cond, ...) do { if (!(cond)) { printf("MISMATCH: " __VA_ARGS__); printf("  [%s]\n", #cond); bad++; } } while (0)

/* what a parser handed out: every record's length and bytes, in order */
typedef struct { unsigned char *p; size_t n, cap, count; } rec_log;
static int log_record(void *user, char *seq, size_t len)
{
    rec_log *l = (rec_log *)user;
    if (l->n + len + sizeof len > l->cap) { l->cap = (l->n + len + sizeof len) * 2 + 4096; l->p = (unsigned char *)realloc(l->p, l->cap); }
    memcpy(l->p + l->n, &len, sizeof len);
    memcpy(l->p + l->n + sizeof len, seq, len);
    l->n += sizeof len + len;
    l->count++;
    return 0;
}
static int log_equal(const rec_log *a, const rec_log *b) { return a->count == b->count && a->n == b->n && (a->n == 0 || !memcmp(a->p, b->p, a->n)); }

/* two parsers stand at the same place: state, counters, the text gathered for the record under way */
static int parser_equal(const parser *a, const parser *b)
{
    /* (between records the lengths still stand but the whole-record shortcut has copied no text: the bytes count inside a record only) */
    const int in_seq = a->state == P_LINE_START || a->state == P_SEQ || a->state == P_PLUS || a->state == P_QUAL;
    /* (and each of the three flags where parser_eof reads it: elsewhere it is left over from whichever way the last record went) */
    return a->state == b->state && (a->state != P_NAME || a->name_any == b->name_any) && (a->state != P_SEQ || a->line_any == b->line_any) &&
           (a->state != P_QUAL || a->qual_any == b->qual_any) &&
           a->seq_len == b->seq_len && a->qual_len == b->qual_len && a->nrecords == b->nrecords && a->sink_rc == b->sink_rc &&
           a->end_kind == b->end_kind && a->end_len == b->end_len && a->last_len == b->last_len &&
           (!in_seq || a->seq_len == 0 || !memcmp(a->seq, b->seq, a->seq_len)) &&
           (a->state != P_QUAL || a->qual_len == 0 || !memcmp(a->qual, b->qual, a->qual_len));
}

static unsigned char *read_file(const char *path, size_t *n)
{
    struct stat sb;
    const int fd = open(path, O_RDONLY);
    unsigned char *p;
    if (fd < 0 || fstat(fd, &sb) != 0) { perror(path); exit(2); }
    *n = (size_t)sb.st_size;
    p = (unsigned char *)malloc(*n ? *n : 1);                        /* (exactly the file: a read past it is the sanitizer's to see) */
    if (ski_pread_exact(fd, p, *n, 0) != *n) { perror(path); exit(2); }
    close(fd);
    return p;
}

/* the reference: bytes [a, b) out of a memory copy of their own, one parser_feed; the parser is left before its eof */
static void feed_copy(const unsigned char *text, size_t a, size_t b, parser *ps, rec_log *log)
{
    unsigned char *copy = (unsigned char *)malloc(b - a ? b - a : 1);
    memcpy(copy, text + a, b - a);
    memset(log, 0, sizeof *log);
    parser_init(ps, log_record, log);
    parser_feed(ps, copy, b - a);
    free(copy);
}

static void compare_and_end(parser *ps, rec_log *log, parser *ref, rec_log *rlog, const char *what, size_t a, size_t b, int mode, size_t block)
{
    CHECK(parser_equal(ps, ref), "%s [%zu, %zu) mode %d block %zu: the parser stands elsewhere\n", what, a, b, mode, block);
    parser_eof(ps);
    parser_eof(ref);
    CHECK(parser_equal(ps, ref), "%s [%zu, %zu) mode %d block %zu: another ending\n", what, a, b, mode, block);
    CHECK(log_equal(log, rlog), "%s [%zu, %zu) mode %d block %zu: other records (%zu against %zu)\n", what, a, b, mode, block, log->count, rlog->count);
    parser_free(ps); parser_free(ref);
    free(log->p); free(rlog->p);
}

static int check_spans(const char *path)
{
    static const size_t blocks[3] = { 64, 257, 4096 }, starts[5] = { 0, 1, 4095, 4096, 4097 };
    size_t n, ends[7], spans[64][2], nspans = 0, i, j, populated = 0;
    unsigned char *text = read_file(path, &n);
    const int fd = open(path, O_RDONLY);
    const unsigned char *map = (const unsigned char *)mmap(NULL, n, PROT_READ, MAP_PRIVATE, fd, 0);
    const size_t last_page = n & ~(size_t)4095;
    int mode, bi;
    if (fd < 0 || map == MAP_FAILED || n < 3 * 4096 + 2 || last_page == n) { printf("MISMATCH: %s cannot be mapped or has an unfit size\n", path); return 1; }
    ends[0] = 8191; ends[1] = 8192; ends[2] = 8193; ends[3] = last_page - 1; ends[4] = last_page; ends[5] = last_page + 1; ends[6] = n;
    spans[nspans][0] = 0; spans[nspans++][1] = n;                    /* the whole file ... */
    for (i = 0; i < 5; i++) for (j = 0; j < 7; j++)                  /* ... and every start with every end */
        if (!(starts[i] == 0 && ends[j] == n)) { spans[nspans][0] = starts[i]; spans[nspans++][1] = ends[j]; }
    for (i = 0; i < nspans; i++) for (mode = SKI_POPULATE; mode <= SKI_MAPPED; mode++) for (bi = 0; bi < 3; bi++) {
        const size_t a = spans[i][0], b = spans[i][1];
        parser ps, ref;
        rec_log log, rlog;
        ski_rbuf rb = { NULL, 0 };
        int m = mode, fr;
        feed_copy(text, a, b, &ref, &rlog);
        memset(&log, 0, sizeof log);
        parser_init(&ps, log_record, &log);
        fr = ski_feed_span(&ps, map, fd, a, b - a, &m, &rb, blocks[bi], NULL);
        CHECK(fr == SKI_FED, "span [%zu, %zu) mode %d: returned %d\n", a, b, mode, fr);
        CHECK(m == mode || (mode == SKI_POPULATE && m == SKI_PREAD), "span [%zu, %zu): mode %d became %d\n", a, b, mode, m);
        CHECK(rb.buf == NULL || (rb.cap == blocks[bi] && mode != SKI_MAPPED), "span [%zu, %zu) mode %d: a block of %zu bytes\n", a, b, mode, rb.cap);
        if (mode == SKI_POPULATE && !rb.buf) {                       /* pages were dropped: what lies next to the span, and the span, still read as the file */
            populated++;
            CHECK(!memcmp(map, text, n), "span [%zu, %zu): the mapping no longer reads as the file\n", a, b);
        }
        compare_and_end(&ps, &log, &ref, &rlog, "span", a, b, mode, blocks[bi]);
        free(rb.buf);
    }
    /* no mapping, a span that reaches past the file's end: told so, fed exactly what exists, and nothing else touched */
    for (bi = 0; bi < 3; bi++) for (i = 0; i < 3; i++) {
        const size_t a = i == 0 ? 4097 : i == 1 ? n - 1 : n, past = 5000;
        parser ps, ref;
        rec_log log, rlog;
        ski_rbuf rb = { NULL, 0 };
        int m = SKI_PREAD, fr;
        feed_copy(text, a, n, &ref, &rlog);
        memset(&log, 0, sizeof log);
        parser_init(&ps, log_record, &log);
        fr = ski_feed_span(&ps, NULL, fd, a, n - a + past, &m, &rb, blocks[bi], NULL);
        CHECK(fr == SKI_SHORT, "short span from %zu: returned %d\n", a, fr);
        CHECK(m == SKI_PREAD && rb.buf && rb.cap == blocks[bi], "short span from %zu: mode %d, a block of %zu bytes\n", a, m, rb.cap);
        compare_and_end(&ps, &log, &ref, &rlog, "short span", a, n, SKI_PREAD, blocks[bi]);
        free(rb.buf);
    }
    {   /* within the file and without a mapping: fed whole, whatever *mode says */
        parser ps, ref;
        rec_log log, rlog;
        ski_rbuf rb = { NULL, 0 };
        int m = SKI_POPULATE, fr;
        feed_copy(text, 1, 8193, &ref, &rlog);
        memset(&log, 0, sizeof log);
        parser_init(&ps, log_record, &log);
        fr = ski_feed_span(&ps, NULL, fd, 1, 8192, &m, &rb, 257, NULL);
        CHECK(fr == SKI_FED && m == SKI_POPULATE, "no mapping: returned %d, mode %d\n", fr, m);
        compare_and_end(&ps, &log, &ref, &rlog, "no mapping", 1, 8193, SKI_PREAD, 257);
        free(rb.buf);
    }
    /* a cancel that is set beforehand: nothing is fed, nothing is made */
    for (mode = SKI_POPULATE; mode <= SKI_MAPPED; mode++) {
        parser ps, fresh;
        rec_log log;
        ski_rbuf rb = { NULL, 0 };
        volatile int cancel = 1;
        int m = mode, fr;
        memset(&log, 0, sizeof log);
        parser_init(&ps, log_record, &log);
        parser_init(&fresh, log_record, &log);
        fr = ski_feed_span(&ps, map, fd, 1, n - 1, &m, &rb, 257, &cancel);
        CHECK(fr == SKI_FED && m == mode && !rb.buf && !log.count && parser_equal(&ps, &fresh), "cancelled, mode %d: something was fed\n", mode);
        parser_free(&ps);
        free(log.p); free(rb.buf);
    }
    printf("%s: %zu spans x 3 ways x 3 blocks, %zu of them populated\n", path, nspans, populated);
    munmap((void *)map, n);
    close(fd);
    free(text);
    return bad != 0;
}

typedef struct { unsigned char *buf; size_t n; } seg;

static int check_cutter(const char *path)
{
    enum { WANT = 300 };
    size_t n, sizes[6] = { 1, 7, 299, 300, 905, 0 }, si, gathered_on = 0;
    unsigned char *text = read_file(path, &n);
    parser whole;
    rec_log wlog;
    int in_while;
    sizes[5] = n;
    feed_copy(text, 0, n, &whole, &wlog);
    parser_eof(&whole);
    for (si = 0; si < 6; si++) for (in_while = 0; in_while < 2; in_while++) {
        ski_cutter c;
        seg *segs = NULL;
        size_t nsegs = 0, cap = 0, at, pos = 0, i;
        rec_log log;
        unsigned char *buf;
        size_t len;
        ski_cutter_init(&c, WANT);
        CHECK(c.tail == 256 && c.want == WANT && c.scan_from == WANT, "cutter: want %zu tail %zu\n", c.want, c.tail);
        for (at = 0; at < n; at += sizes[si]) {
            int took = 0;
            ski_cutter_add(&c, text + at, n - at < sizes[si] ? n - at : sizes[si]);
            while ((in_while || !took) && ski_cutter_take(&c, &buf, &len)) {
                if (nsegs == cap) { cap = cap ? cap * 2 : 64; segs = (seg *)realloc(segs, cap * sizeof *segs); }
                segs[nsegs].buf = buf; segs[nsegs++].n = len;
                took = 1;
            }
            if (!took && c.n >= c.want + c.tail) gathered_on++;        /* no record start yet: it keeps gathering */
        }
        ski_cutter_rest(&c, &buf, &len);
        CHECK(c.buf == NULL && c.n == 0, "cutter: something is left behind the last segment\n");
        if (nsegs == cap) { cap = cap ? cap * 2 : 64; segs = (seg *)realloc(segs, cap * sizeof *segs); }
        segs[nsegs].buf = buf; segs[nsegs++].n = len;
        memset(&log, 0, sizeof log);
        for (i = 0; i < nsegs; i++) {
            parser ps;
            const int last = i + 1 == nsegs;
            CHECK(pos + segs[i].n <= n && !memcmp(segs[i].buf, text + pos, segs[i].n), "delivery %zu, segment %zu: not the text at %zu\n", sizes[si], i, pos);
            if (!last) {
                CHECK(segs[i].n >= WANT, "delivery %zu, segment %zu: %zu bytes, fewer than wanted\n", sizes[si], i, segs[i].n);
                CHECK(pos + segs[i].n < n && parser_guess_start(text + pos, n - pos, segs[i].n, 1) == segs[i].n,
                      "delivery %zu, segment %zu: ends at %zu, where no record start is guessed\n", sizes[si], i, pos + segs[i].n);
            }
            parser_init(&ps, log_record, &log);                      /* a file of its own */
            parser_feed(&ps, segs[i].buf, segs[i].n);
            if (!last) CHECK(ps.state != P_STOP && parser_between_records(&ps), "delivery %zu, segment %zu: ends inside a record (state %d)\n", sizes[si], i, ps.state);
            parser_eof(&ps);
            if (last) CHECK(ps.end_kind == whole.end_kind, "delivery %zu: the last segment ends as %d, the text as %d\n", sizes[si], ps.end_kind, whole.end_kind);
            parser_free(&ps);
            pos += segs[i].n;
            free(segs[i].buf);
        }
        CHECK(pos == n, "delivery %zu: the segments hold %zu bytes of %zu\n", sizes[si], pos, n);
        CHECK(log_equal(&log, &wlog), "delivery %zu, %s: the segments' records are not the text's (%zu against %zu)\n", sizes[si], in_while ? "while" : "once", log.count, wlog.count);
        if (si == 5) CHECK(in_while ? nsegs > 2 : nsegs == 2, "whole text in one delivery, %s: %zu segments\n", in_while ? "while" : "once", nsegs);
        free(log.p);
        free(segs);
    }
    printf("%s: %zu records; kept gathering %zu times\n", path, wlog.count, gathered_on);
    parser_free(&whole);
    free(wlog.p);
    free(text);
    return bad != 0;
}

int main(int argc, char **argv)
{
    if (argc == 3 && !strcmp(argv[1], "span")) return check_spans(argv[2]);
    if (argc == 3 && !strcmp(argv[1], "cut")) return check_cutter(argv[2]);
    fprintf(stderr, "usage: input_check span|cut FILE\n");
    return 2;
}
