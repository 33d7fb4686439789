/* sk_host_background.c -- strain_detect --coverage-background / --background-spectrum on the host: one strain's blocks, target after
 * target as the device's sweeps returned them (sk_background_finish's layout; include/strainer_kmer.h has the rule), and the two
 * tables written from them at the end of the run.  Both are integer TSV with one header line; strain_name and metagenome are formed
 * as in the other coverage tables (the -o file's basename without a trailing ".kmer_hits.gz"; the target's basename); targets come
 * in run order.
 *   strain_name<TAB>metagenome<TAB>class<TAB>kmers<TAB>covered_kmers<TAB>total_hits      class: informative, then background
 *   strain_name<TAB>metagenome<TAB>class<TAB>depth<TAB>kmers<TAB>hits                    depth 0..D, then ">D": every line is written
 * No device call in here: tests/native drives it as a stand-alone program. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "sk_internal.h"

struct skb_table {
    uint32_t max_depth, words;       /* D, SK_BACKGROUND_WORDS(D) */
    uint32_t n, cap;                 /* targets */
    char **name;                     /* [n] the targets' basenames */
    uint64_t *blk;                   /* [n * words] */
};

skb_table *skb_create(uint32_t max_depth)
{
    skb_table *t;
    if (max_depth > SK_BACKGROUND_MAX_DEPTH) return NULL;
    if (!(t = (skb_table *)calloc(1, sizeof *t))) return NULL;
    t->max_depth = max_depth;
    t->words = SK_BACKGROUND_WORDS(max_depth);
    return t;
}

void skb_destroy(skb_table *t)
{
    uint32_t i;
    if (!t) return;
    for (i = 0; i < t->n; i++) free(t->name[i]);
    free(t->name); free(t->blk); free(t);
}

int skb_add(skb_table *t, const char *metagenome, const uint64_t *block)
{
    const char *b;
    if (!t || !metagenome || !block) return -1;
    if (t->n == t->cap) {
        const uint32_t cap = t->cap ? t->cap * 2u : 8u;
        char **name = (char **)realloc(t->name, (size_t)cap * sizeof *name);
        uint64_t *blk;
        if (!name) return -1;
        t->name = name;
        if (!(blk = (uint64_t *)realloc(t->blk, (size_t)cap * t->words * sizeof *blk))) return -1;
        t->blk = blk;
        t->cap = cap;
    }
    b = strrchr(metagenome, '/');
    if (!(t->name[t->n] = strdup(b ? b + 1 : metagenome))) return -1;
    memcpy(t->blk + (size_t)t->n * t->words, block, (size_t)t->words * sizeof *block);
    t->n++;
    return 0;
}

uint32_t skb_targets(const skb_table *t) { return t ? t->n : 0u; }

static const char *const skb_class[2] = { "informative", "background" };

int skb_write(const skb_table *t, const char *strain_name, FILE *f)
{
    uint32_t i, c;
    if (!t || !strain_name || !f) return -1;
    fputs("strain_name\tmetagenome\tclass\tkmers\tcovered_kmers\ttotal_hits\n", f);
    for (i = 0; i < t->n; i++)
        for (c = 0; c < 2u; c++) {
            const uint64_t *o = t->blk + (size_t)i * t->words + (size_t)c * SK_BACKGROUND_CLASS_WORDS(t->max_depth);
            fprintf(f, "%s\t%s\t%s\t%llu\t%llu\t%llu\n", strain_name, t->name[i], skb_class[c], (unsigned long long)o[0], (unsigned long long)o[1],
                    (unsigned long long)o[2]);
        }
    return fflush(f) || ferror(f) ? -1 : 0;
}

int skb_write_spectrum(const skb_table *t, const char *strain_name, FILE *f)
{
    uint32_t i, c, d;
    if (!t || !strain_name || !f) return -1;
    fputs("strain_name\tmetagenome\tclass\tdepth\tkmers\thits\n", f);
    for (i = 0; i < t->n; i++)
        for (c = 0; c < 2u; c++) {
            const uint64_t *o = t->blk + (size_t)i * t->words + (size_t)c * SK_BACKGROUND_CLASS_WORDS(t->max_depth);
            for (d = 0; d <= t->max_depth; d++)
                fprintf(f, "%s\t%s\t%s\t%u\t%llu\t%llu\n", strain_name, t->name[i], skb_class[c], d, (unsigned long long)o[SK_BACKGROUND_HEAD + d],
                        (unsigned long long)(o[SK_BACKGROUND_HEAD + d] * d));
            fprintf(f, "%s\t%s\t%s\t>%u\t%llu\t%llu\n", strain_name, t->name[i], skb_class[c], t->max_depth, (unsigned long long)o[3], (unsigned long long)o[4]);
        }
    return fflush(f) || ferror(f) ? -1 : 0;
}
