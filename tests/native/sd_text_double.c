/* sd_text_double.c -- a CPU double of the device's text-fed batch (sk_batch_fill_text, sk_batch_text_finish, sk_text_enabled) for
 * strain_detect's host layer (sk_host_sd.c: sd_text_read, sd_text_resolve), built from the host parser itself (sk_parser.h) on top of
 * device_double.c's public sk_batch_fill.  It honours the contract of include/strainer_kmer.h: the piece starts at a record boundary;
 * `consumed` ends the last record whose end the piece itself shows (FASTQ: all four lines with their '\n'; FASTA: the next header's
 * character at a line start); with is_eof every byte is consumed; the batch holds EVERY record, short and empty ones included; a
 * piece that does not start with a header character, and a FASTQ record whose quality has the wrong length, DECLINE.
 * SD_TEXT_DOUBLE_DECLINE_AT=<n>|last forces a decline at piece n (counted over the run) or at every file's last piece.
 * TEST CODE only, linked with device_double.c by tests/test_sd_text_host.py. */
#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../include/strainer_kmer.h"
#include "../../strainer2_amd/csrc/sk_parser.h"

int sk_text_enabled(sk_ctx *ctx) { const char *e = getenv("SK_DEVICE_PARSE"); (void)ctx; return e && e[0] == '1'; }

/* what a batch's parse left, until its finish (the batch itself is device_double.c's) */
typedef struct { sk_batch *b; uint8_t *p; size_t len, cap; uint32_t *start; size_t nrec, rcap; sk_text_info info; int pending; } sdt_slot;
#define SDT_SLOTS 64
static sdt_slot g_slot[SDT_SLOTS];
static pthread_mutex_t g_mu = PTHREAD_MUTEX_INITIALIZER;
static unsigned long long g_pieces;

static sdt_slot *slot_of(sk_batch *b)
{
    int i;
    sdt_slot *s = NULL;
    pthread_mutex_lock(&g_mu);
    for (i = 0; i < SDT_SLOTS && !s; i++) if (g_slot[i].b == b) s = &g_slot[i];
    for (i = 0; i < SDT_SLOTS && !s; i++) if (!g_slot[i].b) { s = &g_slot[i]; s->b = b; }
    pthread_mutex_unlock(&g_mu);
    return s;
}

static int sdt_record(void *user, char *seq, size_t len)
{
    sdt_slot *o = (sdt_slot *)user;
    if (o->len + len + 1 > o->cap) { o->cap = (o->len + len + 1) * 2; o->p = (uint8_t *)realloc(o->p, o->cap); }
    if (o->nrec == o->rcap) { o->rcap = o->rcap ? o->rcap * 2 : 64; o->start = (uint32_t *)realloc(o->start, o->rcap * sizeof *o->start); }
    o->start[o->nrec++] = (uint32_t)o->len;
    memcpy(o->p + o->len, seq, len);
    o->len += len;
    o->p[o->len++] = '\n';
    return 0;
}

int sk_batch_fill_text(sk_batch *b, const uint8_t *text, uint64_t nbytes, int is_eof)
{
    const char *force = getenv("SD_TEXT_DOUBLE_DECLINE_AT");
    const unsigned long long piece = __atomic_fetch_add(&g_pieces, 1, __ATOMIC_RELAXED);
    sdt_slot *s = slot_of(b);
    parser ps;
    uint64_t i, c_consumed = 0;
    size_t c_len = 0, c_nrec = 0;
    int decline = 0, at_seek = 0;
    if (!s || !text || !nbytes) return SK_E_ARG;
    s->len = s->nrec = 0;
    memset(&s->info, 0, sizeof s->info);
    if (force && (!strcmp(force, "last") ? is_eof != 0 : piece == (unsigned long long)atoll(force))) decline = 1;
    if (text[0] != '>' && text[0] != '@') decline = 1;
    parser_init(&ps, sdt_record, s);
    for (i = 0; i < nbytes && !decline && ps.state != P_STOP; i++) {
        const int64_t before = ps.nrecords;
        parser_feed(&ps, text + i, 1);
        if (ps.nrecords != before) {                       /* a record ended: at this header character (FASTA), behind this '\n' (FASTQ) */
            c_consumed = ps.state == P_NAME ? i : i + 1;
            c_len = s->len; c_nrec = s->nrec;
        }
    }
    if (!decline && ps.state != P_STOP && is_eof) {
        at_seek = ps.state == P_SEEK;                      /* (behind a whole FASTQ record: the form whose ending is END_STALE) */
        parser_eof(&ps);
        c_consumed = nbytes; c_len = s->len; c_nrec = s->nrec;
    }
    if (ps.end_kind == SKP_END_TRUNC) decline = 1;         /* (the host parser stops where the reference stops) */
    s->info.form = (is_eof ? at_seek : ps.qual_cap != 0) ? SK_TEXT_FASTQ4 : SK_TEXT_FASTA;
    parser_free(&ps);
    if (decline || c_nrec > (1u << 22)) s->info.status = SK_TEXT_DECLINED;
    else {
        uint64_t bases = c_len - c_nrec;
        s->info.status = SK_TEXT_OK;
        s->info.consumed = c_consumed; s->info.stream_bytes = c_len; s->info.nrecords = c_nrec; s->info.bases = bases;
        s->len = c_len; s->nrec = c_nrec;
    }
    s->pending = 1;
    return SK_OK;
}

int sk_batch_text_finish(sk_batch *b, sk_text_info *info, const uint32_t **rec_start)
{
    sdt_slot *s = slot_of(b);
    if (!s || !s->pending || !info) return SK_E_STATE;
    s->pending = 0;
    *info = s->info;
    if (rec_start) *rec_start = s->start;
    if (info->status == SK_TEXT_OK && info->nrecords) return sk_batch_fill(b, s->p, s->len, s->start, (uint32_t)s->nrec);
    return SK_OK;
}
