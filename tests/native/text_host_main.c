/* text_host_main.c -- stand-alone driver of the list scan for tests/test_text_parse_host.py: <strain file> <list file>.  Linked with
 * device_double.c (-DDOUBLE_NO_MAIN), the host sources and -- or not -- text_double.c; prints the bases seen, a digest and the sum of
 * the column, and what the text double counted.  TEST CODE only. */
#include <stdio.h>
#include <stdlib.h>
#include "../../include/strainer_kmer.h"

#pragma weak text_double_stats
void text_double_stats(unsigned long long *pieces, unsigned long long *declined, unsigned long long *grown);

int main(int argc, char **argv)
{
    skh_keyset ks;
    sk_ctx *ctx = NULL;
    uint64_t bases = 0, sum = 0, digest = 0xCBF29CE484222325ull;
    unsigned long long pieces = 0, declined = 0, grown = 0;
    uint32_t *col, i;
    int rc;
    if (argc != 3) return 2;
    if ((rc = skh_keyset_from_file(&ks, argv[1], 50, 1, 1)) != SK_OK || (rc = sk_ctx_create(&ctx, 0)) != SK_OK ||
        (rc = skh_keyset_load(ctx, &ks, 4)) != SK_OK) { fprintf(stderr, "set-up failed: %d\n", rc); return 1; }
    if ((rc = skh_scan_list(ctx, argv[2], NULL, 1, NULL, stderr, 0, 1, &bases)) != SK_OK) { fprintf(stderr, "scan failed: %d\n", rc); return 1; }
    col = (uint32_t *)calloc((size_t)ks.nrows + 1, sizeof *col);
    if (sk_counts_fetch(ctx, 1, col) != SK_OK) return 1;
    for (i = 0; i < ks.nrows; i++) { sum += col[i]; digest = (digest ^ col[i]) * 0x100000001B3ull; }
    if (text_double_stats) text_double_stats(&pieces, &declined, &grown);
    printf("bases=%llu digest=%016llx sum=%llu\n", (unsigned long long)bases, (unsigned long long)digest, (unsigned long long)sum);
    printf("pieces=%llu declined=%llu grown=%llu\n", pieces, declined, grown);
    free(col);
    skh_keyset_free(&ks);
    sk_ctx_destroy(ctx);
    return 0;
}
