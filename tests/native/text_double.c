/* text_double.c -- a CPU double of the device's text parser (sk_scan_text_pinned_many, sk_text_enabled) for the host layer's piece
 * walk (sk_host.c: text_scan), built from the host parser itself (sk_parser.h).  It honours the contract of
 * include/strainer_kmer.h: the piece starts at a record boundary; `consumed` ends the last record whose end the piece itself
 * shows (FASTQ: all four lines with their '\n'; FASTA: the next header's character at a line start); with is_eof every byte is
 * consumed; a piece that does not start with a header character, and a FASTQ record whose quality has the wrong length, DECLINE.
 * TEXT_DOUBLE_DECLINE_AT=<n>|last forces a decline at piece n (counted over the run) or at every file's last piece.
 * TEST CODE only, linked with device_double.c by tests/test_text_parse_host.py. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../include/strainer_kmer.h"
#include "../../strainer2_amd/csrc/sk_parser.h"

static unsigned long long g_pieces, g_declined, g_grown;
void text_double_stats(unsigned long long *pieces, unsigned long long *declined, unsigned long long *grown)
{
    *pieces = __atomic_load_n(&g_pieces, __ATOMIC_RELAXED);
    *declined = __atomic_load_n(&g_declined, __ATOMIC_RELAXED);
    *grown = __atomic_load_n(&g_grown, __ATOMIC_RELAXED);
}

int sk_text_enabled(sk_ctx *ctx) { const char *e = getenv("SK_DEVICE_PARSE"); (void)ctx; return e && e[0] == '1'; }

typedef struct { uint8_t *p; size_t len, cap; uint64_t bases; } td_out;
static int td_record(void *user, char *seq, size_t len)
{
    td_out *o = (td_out *)user;
    if (o->len + len + 1 > o->cap) { o->cap = (o->len + len + 1) * 2; o->p = (uint8_t *)realloc(o->p, o->cap); }
    memcpy(o->p + o->len, seq, len);
    o->len += len;
    o->p[o->len++] = '\n';
    o->bases += len;
    return 0;
}

int sk_scan_text_pinned_many(sk_ctx *const *ctx, uint32_t n, const uint8_t *text, uint64_t nbytes, int is_eof, uint32_t col, sk_text_info *info)
{
    const char *force = getenv("TEXT_DOUBLE_DECLINE_AT"), *pb = getenv("SK_TEXT_PIECE_BYTES");
    const unsigned long long piece = __atomic_fetch_add(&g_pieces, 1, __ATOMIC_RELAXED);
    td_out out = {NULL, 0, 0, 0};
    parser ps;
    uint64_t i, c_consumed = 0, c_len = 0, c_bases = 0, c_nrec = 0;
    int decline = 0;
    uint32_t k;
    memset(info, 0, sizeof *info);
    if (pb && nbytes > (uint64_t)atoll(pb)) __atomic_fetch_add(&g_grown, 1, __ATOMIC_RELAXED);
    if (force && (!strcmp(force, "last") ? is_eof != 0 : piece == (unsigned long long)atoll(force))) decline = 1;
    if (!nbytes || (text[0] != '>' && text[0] != '@')) decline = 1;
    parser_init(&ps, td_record, &out);
    for (i = 0; i < nbytes && !decline && ps.state != P_STOP; i++) {
        const int64_t before = ps.nrecords;
        parser_feed(&ps, text + i, 1);
        if (ps.nrecords != before) {                       /* a record ended: at this header character (FASTA), behind this '\n' (FASTQ) */
            c_consumed = ps.state == P_NAME ? i : i + 1;
            c_len = out.len; c_bases = out.bases; c_nrec = (uint64_t)ps.nrecords;
        }
    }
    if (!decline && ps.state != P_STOP && is_eof) {
        parser_eof(&ps);
        c_consumed = nbytes; c_len = out.len; c_bases = out.bases; c_nrec = (uint64_t)ps.nrecords;
    }
    if (ps.end_kind == SKP_END_TRUNC) decline = 1;         /* (the host parser stops where the reference stops) */
    parser_free(&ps);
    if (decline) {
        __atomic_fetch_add(&g_declined, 1, __ATOMIC_RELAXED);
        info->status = SK_TEXT_DECLINED;
        free(out.p);
        return SK_OK;
    }
    info->status = SK_TEXT_OK;
    info->form = SK_TEXT_FASTA;
    info->consumed = c_consumed; info->stream_bytes = c_len; info->nrecords = c_nrec; info->bases = c_bases;
    for (k = 0; k < n; k++) { const int rc = sk_scan_stream(ctx[k], out.p, c_len, col); if (rc) { free(out.p); return rc; } }
    free(out.p);
    return SK_OK;
}
