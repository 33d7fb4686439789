/* sk_host_regions.c -- the region table of a strain (strain_detect --coverage-regions): where along the strain's text every window
 * of every record lies, so that a table row's first position names a region of the genome.
 *
 * The text is the one both key-set builders make (sk_host.c: builder_record, dk_record): the records of the strain file with at
 * least k - 1 bases, in file order, end to end.  The file is read with the record grammar every other reader here uses
 * (sk_parser.h); this is the one translation unit that compiles the parser's name sink in, for the records' names.
 */
#define _GNU_SOURCE
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <zlib.h>
#include "../../include/strainer_kmer.h"
#include "sk_common.h"
#define SKP_NAME_SINK
#include "sk_parser.h"

typedef struct {
    skh_regions *r;
    uint64_t window, cap, ncap;
    uint64_t record;            /* records seen so far, short ones included */
    char *pending;              /* the name of the record whose bases come next */
    int rc;
} rg_state;

static int rg_name(void *user, const char *name, size_t len)
{
    rg_state *s = (rg_state *)user;
    free(s->pending);
    s->pending = (char *)malloc(len + 1);
    if (!s->pending) { s->rc = SK_E_NOMEM; return 1; }
    memcpy(s->pending, name, len);
    s->pending[len] = 0;
    return 0;
}

static int rg_record(void *user, char *seq, size_t len)
{
    rg_state *s = (rg_state *)user;
    skh_regions *r = s->r;
    const uint64_t w = s->window ? s->window : (len ? len : 1);
    const uint64_t nwin = len ? (len + w - 1) / w : 1;
    uint64_t j;
    (void)seq;
    s->record++;
    if (len + 1 < SK_K) return 0;                        /* not part of the text (builder_record, dk_record) */
    if ((uint64_t)r->n + nwin > SKH_REGIONS_MAX) { s->rc = SK_E_ARG; r->too_many = 1; return 1; }
    if (r->nnames == s->ncap) {
        const uint64_t cap = s->ncap ? s->ncap * 2 : 64;
        char **nn = (char **)realloc(r->names, cap * sizeof *nn);
        if (!nn) { s->rc = SK_E_NOMEM; return 1; }
        r->names = nn; s->ncap = cap;
    }
    r->names[r->nnames++] = s->pending ? s->pending : strdup("");
    s->pending = NULL;
    if (!r->names[r->nnames - 1]) { r->nnames--; s->rc = SK_E_NOMEM; return 1; }
    if ((uint64_t)r->n + nwin > s->cap) {
        uint64_t cap = s->cap ? s->cap * 2 : 64;
        while (cap < (uint64_t)r->n + nwin) cap *= 2;
#define RG_GROW(field) do { void *p_ = realloc(r->field, cap * sizeof *r->field); if (!p_) { s->rc = SK_E_NOMEM; return 1; } r->field = p_; } while (0)
        RG_GROW(text_off); RG_GROW(record); RG_GROW(rec_off); RG_GROW(len); RG_GROW(name);
#undef RG_GROW
        s->cap = cap;
    }
    for (j = 0; j < nwin; j++) {
        const uint64_t a = j * w, e = a + w < len ? a + w : len;
        r->text_off[r->n] = r->text_bases + a;
        r->record[r->n] = (uint32_t)(s->record > 0xFFFFFFFFu ? 0xFFFFFFFFu : s->record);
        r->rec_off[r->n] = a;
        r->len[r->n] = e - a;
        r->name[r->n] = r->names[r->nnames - 1];
        r->n++;
    }
    r->text_bases += len;
    return 0;
}

void skh_regions_free(skh_regions *r)
{
    uint32_t i;
    if (!r) return;
    for (i = 0; i < r->nnames; i++) free(r->names[i]);
    free(r->names); free(r->text_off); free(r->record); free(r->rec_off); free(r->len); free(r->name);
    memset(r, 0, sizeof *r);
}

int skh_regions_from_file(const char *path, uint64_t window, skh_regions *out)
{
    enum { BLK = 1 << 20 };
    rg_state s;
    parser ps;
    gzFile g;
    unsigned char *blk;
    int got;
    if (!path || !out) return SK_E_ARG;
    memset(out, 0, sizeof *out);
    memset(&s, 0, sizeof s);
    s.r = out; s.window = window;
    if (!(g = gzopen(path, "rb"))) return SK_E_OPEN;     /* (plain text passes through) */
    gzbuffer(g, BLK);
    if (!(blk = (unsigned char *)malloc(BLK))) { gzclose(g); return SK_E_NOMEM; }
    parser_init(&ps, rg_record, &s);
    parser_set_name_sink(&ps, rg_name);
    while (ps.state != P_STOP && (got = gzread(g, blk, BLK)) > 0) parser_feed(&ps, blk, (size_t)got);
    parser_eof(&ps);
    parser_free(&ps);
    free(blk);
    gzclose(g);
    free(s.pending);
    if (s.rc != SK_OK) {
        const int too_many = out->too_many;
        skh_regions_free(out);
        out->too_many = too_many;
        return s.rc;
    }
    return SK_OK;
}
