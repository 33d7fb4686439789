/* sk_host_support.c -- strain_detect --coverage-support / --support-pairs on the host: the run's numbers per sample and strain, the merge
 * of a replayed run's emission lists across the strains of a group, and the two files (include/strainer_kmer.h has the rule and the
 * formats).  No device call and nothing of the scan: tests/native/support_check.c drives this file on its own. */
#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "sk_internal.h"

typedef struct sks_smp {
    char     *name;                 /* the targets' basename */
    uint64_t *mem;                  /* [nstrains x 3] supporting_pairs, lines, both_mates */
    uint64_t *mat;                  /* [nstrains x group x 2] row a, column b - first strain of a's group: shared pairs, lines of a */
    uint32_t *first;                /* [nstrains] the ordinal of the target that gave the strain its first emission here, 0: none yet */
} sks_smp;

struct sks_acc {
    uint32_t ns, group;
    sks_smp *smp; uint32_t n, cap;
    uint32_t targets;               /* sks_sample calls so far */
    pthread_mutex_t mu;
};

sks_acc *sks_create(uint32_t nstrains, uint32_t group)
{
    sks_acc *a;
    if (!nstrains || !group) return NULL;
    if (!(a = (sks_acc *)calloc(1, sizeof *a))) return NULL;
    a->ns = nstrains; a->group = group;
    pthread_mutex_init(&a->mu, NULL);
    return a;
}

void sks_destroy(sks_acc *a)
{
    uint32_t i;
    if (!a) return;
    for (i = 0; i < a->n; i++) { free(a->smp[i].name); free(a->smp[i].mem); free(a->smp[i].mat); free(a->smp[i].first); }
    free(a->smp);
    pthread_mutex_destroy(&a->mu);
    free(a);
}

/* the sample of a target (two targets with one basename are one sample), made at first sight; every call is one more target */
int sks_sample(sks_acc *a, const char *metagenome)
{
    const char *b = strrchr(metagenome, '/');
    uint32_t i;
    b = b ? b + 1 : metagenome;
    a->targets++;
    for (i = 0; i < a->n; i++) if (!strcmp(a->smp[i].name, b)) return (int)i;
    if (a->n == a->cap) {
        const uint32_t c2 = a->cap ? a->cap * 2 : 16;
        sks_smp *s2 = (sks_smp *)realloc(a->smp, (size_t)c2 * sizeof *s2);
        if (!s2) return -1;
        a->smp = s2; a->cap = c2;
    }
    {
        sks_smp *s = &a->smp[a->n];
        s->name = strdup(b);
        s->mem = (uint64_t *)calloc((size_t)a->ns * 3, sizeof *s->mem);
        s->mat = (uint64_t *)calloc((size_t)a->ns * a->group * 2, sizeof *s->mat);
        s->first = (uint32_t *)calloc(a->ns, sizeof *s->first);
        if (!s->name || !s->mem || !s->mat || !s->first) { free(s->name); free(s->mem); free(s->mat); free(s->first); return -1; }
    }
    return (int)a->n++;
}

int sks_list_push(sks_list *l, uint32_t pair, uint32_t lines, uint32_t parts)
{
    if (l->n == l->cap) {
        const uint32_t c2 = l->cap ? l->cap * 2 : 64;
        sks_em *e2 = (sks_em *)realloc(l->e, (size_t)c2 * sizeof *e2);
        if (!e2) return -1;
        l->e = e2; l->cap = c2;
    }
    l->e[l->n].pair = pair; l->e[l->n].lines = lines; l->e[l->n].parts = parts;
    l->n++;
    return 0;
}

void sks_list_free(sks_list *l) { free(l->e); l->e = NULL; l->n = l->cap = 0; }

static void sks_add_cell(sks_acc *a, sks_smp *s, uint32_t x, uint32_t y, uint64_t pairs, uint64_t lines)
{
    uint64_t *c = s->mat + ((size_t)x * a->group + (y - x / a->group * a->group)) * 2;
    c[0] += pairs; c[1] += lines;
}

static void sks_add_member(sks_acc *a, sks_smp *s, uint32_t x, uint64_t pairs, uint64_t lines, uint64_t both)
{
    s->mem[3 * (size_t)x] += pairs; s->mem[3 * (size_t)x + 1] += lines; s->mem[3 * (size_t)x + 2] += both;
    if (pairs && !s->first[x]) s->first[x] = a->targets;
}

/* One replayed run's emissions, a list per strain with the run's pair numbers ascending: the per-strain sums, and for every group
 * its lists merged by pair -- a walk over the lists' heads, so the cost goes with the emissions (times the group's size at most),
 * never with pairs x strains.  Any thread; the sums are added under the accumulator's lock. */
int sks_merge(sks_acc *a, uint32_t sample, const sks_list *lists)
{
    uint32_t g0;
    if (sample >= a->n) return -1;
    pthread_mutex_lock(&a->mu);
    {
        sks_smp *s = &a->smp[sample];
        for (g0 = 0; g0 < a->ns; g0 += a->group) {
            const uint32_t n = a->ns - g0 < a->group ? a->ns - g0 : a->group;
            uint32_t at[SK_UNION_MAX], who[SK_UNION_MAX], k;
            if (n > SK_UNION_MAX) { pthread_mutex_unlock(&a->mu); return -1; }
            for (k = 0; k < n; k++) at[k] = 0;
            for (;;) {
                uint32_t lo = 0xFFFFFFFFu, nw = 0, x, y;
                int any = 0;
                for (k = 0; k < n; k++)
                    if (at[k] < lists[g0 + k].n) { const uint32_t pr = lists[g0 + k].e[at[k]].pair; if (!any || pr < lo) lo = pr; any = 1; }
                if (!any) break;
                for (k = 0; k < n; k++)
                    if (at[k] < lists[g0 + k].n && lists[g0 + k].e[at[k]].pair == lo) who[nw++] = k;
                for (x = 0; x < nw; x++) {
                    const sks_em *e = &lists[g0 + who[x]].e[at[who[x]]];
                    sks_add_member(a, s, g0 + who[x], 1, e->lines, e->parts == 3u);
                    if (nw == 1) sks_add_cell(a, s, g0 + who[x], g0 + who[x], 1, e->lines);
                    else for (y = 0; y < nw; y++) if (y != x) sks_add_cell(a, s, g0 + who[x], g0 + who[y], 1, e->lines);
                }
                for (x = 0; x < nw; x++) at[who[x]]++;
            }
        }
    }
    pthread_mutex_unlock(&a->mu);
    return 0;
}

/* what the device counted for the n strains from `first` on (one launch's members, inside one group): sk_covacc_finish_target_support's
 * arrays, the matrices n x n */
int sks_add_device(sks_acc *a, uint32_t sample, uint32_t first, uint32_t n, const uint64_t *pairs, const uint64_t *lines, const uint64_t *both,
                   const uint64_t *shared, const uint64_t *lines_a)
{
    uint32_t x, y;
    if (sample >= a->n || first >= a->ns || n > a->ns - first || first / a->group != (first + n - 1) / a->group) return -1;
    pthread_mutex_lock(&a->mu);
    for (x = 0; x < n; x++) {
        sks_add_member(a, &a->smp[sample], first + x, pairs[x], lines[x], both[x]);
        for (y = 0; y < n; y++) sks_add_cell(a, &a->smp[sample], first + x, first + y, shared[(size_t)x * n + y], lines_a[(size_t)x * n + y]);
    }
    pthread_mutex_unlock(&a->mu);
    return 0;
}

/* a strain's .coverage_support: the samples in the order of the strain's main table -- those with an emission by the target that gave
 * the first, then the others by first sight */
int sks_write_support(const sks_acc *a, uint32_t strain, FILE *f)
{
    uint32_t i, k, done = 0;
    if (strain >= a->ns) return -1;
    fputs("metagenome\tsupporting_pairs\tboth_mates\tlines\n", f);
    for (k = 0; done < a->n && k <= a->targets; k++)             /* (k = the ordinal of a first emission; few samples: no sort) */
        for (i = 0; i < a->n; i++)
            if (a->smp[i].first[strain] == k + 1u) {
                const uint64_t *m = a->smp[i].mem + 3 * (size_t)strain;
                fprintf(f, "%s\t%llu\t%llu\t%llu\n", a->smp[i].name, (unsigned long long)m[0], (unsigned long long)m[2], (unsigned long long)m[1]);
                done++;
            }
    for (i = 0; i < a->n; i++)
        if (!a->smp[i].first[strain]) fprintf(f, "%s\t0\t0\t0\n", a->smp[i].name);
    return ferror(f) ? -1 : 0;
}

/* the panel's pairs file: the groups, then per sample (by first sight), strain a and strain b of a's group the shared pairs and a's
 * lines in them -- every a = a row (the exclusive numbers), the others only where pairs > 0 */
int sks_write_pairs(const sks_acc *a, const char *const *names, FILE *f)
{
    uint32_t i, x, y, g;
    for (g = 0; g * a->group < a->ns; g++) {
        fprintf(f, "#group\t%u", g);
        for (x = g * a->group; x < a->ns && x < (g + 1) * a->group; x++) fprintf(f, "\t%s", names[x]);
        fputc('\n', f);
    }
    fputs("metagenome\tstrain_a\tstrain_b\tpairs\tlines_a\n", f);
    for (i = 0; i < a->n; i++)
        for (x = 0; x < a->ns; x++) {
            const uint32_t g0 = x / a->group * a->group;
            for (y = g0; y < a->ns && y < g0 + a->group; y++) {
                const uint64_t *c = a->smp[i].mat + ((size_t)x * a->group + (y - g0)) * 2;
                if (x == y || c[0])
                    fprintf(f, "%s\t%s\t%s\t%llu\t%llu\n", a->smp[i].name, names[x], names[y], (unsigned long long)c[0], (unsigned long long)c[1]);
            }
        }
    return ferror(f) ? -1 : 0;
}
