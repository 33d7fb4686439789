/* rarefaction_check.c -- drives the HOST side of rarefaction (strainer2_amd/csrc/sk_host_rarefaction.c: the list parser, the draw, a
 * pair's class, the host fold and the table writer) as a stand-alone program, so that it can run under AddressSanitizer + UBSan.  It
 * includes that file and nothing else of the library.  Built and run by tests/test_coverage_rarefaction_host.py.
 *   rarefaction_check parse LIST|- SEED        "T <n>" and one "<T> <text>" line per fraction ('-': the default list); exit 3: refused
 *   rarefaction_check draw SEED I...           one u(i) per line
 *   rarefaction_check fold LIST|- SEED MIN NROWS FIRST NPAIRS NLINES LCG OUT
 *       NLINES hit lines (pair, row, total) from a small generator of its own, folded by skh_rarefaction_fold and, beside it, by a table
 *       computed here line by line with sets per subsample (no classes, no suffix sums); both must agree (exit 4 otherwise).  The
 *       generated lines go to stdout as "pair row total", and the table, as skh_rarefaction_write prints it with and without a strain
 *       column, to OUT. */
#include "../../strainer2_amd/csrc/sk_host_rarefaction.c"

static uint64_t lcg(uint64_t *s) { *s = *s * 6364136223846793005ull + 1442695040888963407ull; return *s >> 11; }

int main(int argc, char **argv)
{
    skh_rarefaction r;
    uint32_t q;
    if (argc >= 4 && !strcmp(argv[1], "parse")) {
        if (skh_rarefaction_parse(strcmp(argv[2], "-") ? argv[2] : NULL, (uint32_t)strtoul(argv[3], NULL, 0), &r) != SK_OK) return 3;
        printf("T %u\n", r.n);
        for (q = 0; q < r.n; q++) printf("%llu %s\n", (unsigned long long)r.T[q], r.text[q]);
        return 0;
    }
    if (argc >= 3 && !strcmp(argv[1], "draw")) {
        int i;
        for (i = 3; i < argc; i++) printf("%u\n", skh_rarefaction_draw(strtoull(argv[i], NULL, 0), (uint32_t)strtoul(argv[2], NULL, 0)));
        return 0;
    }
    if (argc == 11 && !strcmp(argv[1], "fold")) {
        const int64_t min_hits = strtoll(argv[4], NULL, 0);
        const uint32_t nrows = (uint32_t)strtoul(argv[5], NULL, 0);
        const uint64_t first = strtoull(argv[6], NULL, 0), npairs = strtoull(argv[7], NULL, 0), n = strtoull(argv[8], NULL, 0);
        uint64_t seed = strtoull(argv[9], NULL, 0), i, *pair, gp[16], gu[16], gt[16];
        uint32_t *row, *tot;
        unsigned char *seen;
        FILE *f;
        int bad = 0;
        if (skh_rarefaction_parse(strcmp(argv[2], "-") ? argv[2] : NULL, (uint32_t)strtoul(argv[3], NULL, 0), &r) != SK_OK) return 3;
        pair = (uint64_t *)malloc((n ? n : 1) * sizeof *pair);
        row = (uint32_t *)malloc((n ? n : 1) * sizeof *row);
        tot = (uint32_t *)malloc((n ? n : 1) * sizeof *tot);
        seen = (unsigned char *)malloc(nrows ? nrows : 1);
        if (!pair || !row || !tot || !seen) return 2;
        for (i = 0; i < n; i++) {
            pair[i] = first + (npairs ? lcg(&seed) % npairs : 0);
            row[i] = nrows ? (uint32_t)(lcg(&seed) % nrows) : 0;
            tot[i] = (uint32_t)(lcg(&seed) % 7);
            printf("%llu %u %u\n", (unsigned long long)pair[i], row[i], tot[i]);
        }
        if (skh_rarefaction_fold(&r, min_hits, nrows, pair, row, tot, nrows ? n : 0, first, npairs, gp, gu, gt) != SK_OK) return 2;
        for (q = 0; q < r.n && !bad; q++) {                    /* the table of subsample q, from the keep rule alone */
            uint64_t p = 0, u = 0, t = 0;
            memset(seen, 0, nrows ? nrows : 1);
            for (i = 0; i < npairs; i++) p += (uint64_t)skh_rarefaction_draw(first + i, r.seed) < r.T[q];
            for (i = 0; nrows && i < n; i++) {
                if (!((int64_t)tot[i] > min_hits) || !((uint64_t)skh_rarefaction_draw(pair[i], r.seed) < r.T[q])) continue;
                t++;
                if (!seen[row[i]]) { seen[row[i]] = 1; u++; }
            }
            if (p != gp[q] || u != gu[q] || t != gt[q]) {
                fprintf(stderr, "fraction %u: fold %llu %llu %llu, the keep rule %llu %llu %llu\n", q, (unsigned long long)gp[q],
                        (unsigned long long)gu[q], (unsigned long long)gt[q], (unsigned long long)p, (unsigned long long)u, (unsigned long long)t);
                bad = 1;
            }
        }
        if (!bad && nrows && n) {                              /* a row the strain does not have is refused */
            uint64_t xp[16], xu[16], xt[16];
            const uint32_t keep = row[0];
            row[0] = nrows;
            if (skh_rarefaction_fold(&r, min_hits, nrows, pair, row, tot, n, first, npairs, xp, xu, xt) != SK_E_ARG) bad = 1;
            row[0] = keep;
        }
        if (!(f = fopen(argv[10], "w"))) return 2;
        if (skh_rarefaction_write(f, &r, NULL, NULL, NULL, NULL, NULL) != SK_OK || skh_rarefaction_write(f, &r, NULL, "m0.fq", gp, gu, gt) != SK_OK ||
            skh_rarefaction_write(f, &r, "Genus_species_s0", NULL, NULL, NULL, NULL) != SK_OK ||
            skh_rarefaction_write(f, &r, "Genus_species_s0", "m0.fq", gp, gu, gt) != SK_OK) bad = 1;
        fclose(f);
        free(pair); free(row); free(tot); free(seen);
        return bad ? 4 : 0;
    }
    fprintf(stderr, "usage: rarefaction_check parse|draw|fold ...\n");
    return 2;
}
