/* sk_sweep.h -- the scrub sweep's fraction list, for the host programs that take one (kmer_scrub_filter --min_fraction_list,
 * kmer_scrub_count --scrub f0,f1,...) and those that read a class file's header.  include/strainer_kmer.h has the rule: 1 to
 * SK_SCRUB_SWEEP_MAX numbers in [0, 1], strictly descending, each kept as the text it was given. */
#ifndef SK_SWEEP_H
#define SK_SWEEP_H
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "sk_internal.h"                         /* (SKW_TEXT_MAX, and the public header) */

typedef struct {
    uint32_t n;
    double   f[SK_SCRUB_SWEEP_MAX];
    char     text[SK_SCRUB_SWEEP_MAX][SKW_TEXT_MAX];
} skw_list;

/* "f0,f1,...": 0 on success; otherwise 1 and `why` says what is wrong with the list */
static inline int skw_parse_list(const char *text, skw_list *l, char *why, size_t why_cap)
{
    const char *p = text;
    l->n = 0;
    for (;;) {
        const char *e = p;
        char buf[SKW_TEXT_MAX], *end;
        double v;
        while (*e && *e != ',') e++;
        if (e == p) { snprintf(why, why_cap, "an empty field"); return 1; }
        if (l->n == SK_SCRUB_SWEEP_MAX) { snprintf(why, why_cap, "more than %u fractions", SK_SCRUB_SWEEP_MAX); return 1; }
        if ((size_t)(e - p) >= sizeof buf) { snprintf(why, why_cap, "'%.40s...' is no number from 0 to 1", p); return 1; }
        memcpy(buf, p, (size_t)(e - p));
        buf[e - p] = 0;
        v = strtod(buf, &end);
        if (end == buf || *end || buf[0] == ' ' || buf[0] == '\t' || buf[0] == '\n' || !(v == v)) {
            snprintf(why, why_cap, "'%s' is no number from 0 to 1", buf);
            return 1;
        }
        if (v < 0.0 || v > 1.0) { snprintf(why, why_cap, "%s is out of range (0 to 1)", buf); return 1; }
        if (l->n && !(v < l->f[l->n - 1])) { snprintf(why, why_cap, "%s after %s: the list must descend strictly", buf, l->text[l->n - 1]); return 1; }
        l->f[l->n] = v;
        memcpy(l->text[l->n], buf, (size_t)(e - p) + 1);
        l->n++;
        if (!*e) return 0;
        p = e + 1;
    }
}
#endif /* SK_SWEEP_H */
