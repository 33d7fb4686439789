/* background_check.c -- drives the HOST side of the background tables (strainer2_amd/csrc/sk_host_background.c: the targets' blocks and
 * the two tables' writers) as a stand-alone program, so that it can run under AddressSanitizer + UBSan without anything sanitized being
 * loaded into Python.  Built and run by tests/test_coverage_background_host.py.
 *   argv[1]  a script: first line "D <max_depth> <strain name>", then one line per target "T <path> <w0> <w1> ..." with the
 *            SK_BACKGROUND_WORDS(max_depth) u64 words of its block
 *   argv[2]  where the table goes, argv[3] where the spectrum goes */
#include <inttypes.h>
#include "../../strainer2_amd/csrc/sk_host_background.c"

int main(int argc, char **argv)
{
    FILE *in, *f;
    char strain[256], path[1024], tag[8];
    unsigned D = 0;
    uint32_t words, i;
    uint64_t *blk;
    skb_table *t;
    int rc = 0;
    if (argc != 4 || !(in = fopen(argv[1], "r"))) return 2;
    if (fscanf(in, "%7s %u %255s", tag, &D, strain) != 3 || strcmp(tag, "D")) return 2;
    if (skb_create(SK_BACKGROUND_MAX_DEPTH + 1u)) return 3;            /* a depth the tables do not take */
    if (!(t = skb_create(D))) return 3;
    words = SK_BACKGROUND_WORDS(D);
    if (!(blk = (uint64_t *)malloc((size_t)words * sizeof *blk))) return 3;
    while (fscanf(in, "%7s %1023s", tag, path) == 2) {
        if (strcmp(tag, "T")) return 2;
        for (i = 0; i < words; i++) if (fscanf(in, "%" SCNu64, &blk[i]) != 1) return 2;
        if (skb_add(t, path, blk)) return 3;
        memset(blk, 0xA5, (size_t)words * sizeof *blk);                 /* (the table keeps a copy) */
    }
    fclose(in);
    if (skb_add(t, NULL, blk) == 0 || skb_add(NULL, "x", blk) == 0) return 4;
    if (!(f = fopen(argv[2], "w"))) return 5;
    rc |= skb_write(t, strain, f);
    fclose(f);
    if (!(f = fopen(argv[3], "w"))) return 5;
    rc |= skb_write_spectrum(t, strain, f);
    fclose(f);
    printf("%u\n", skb_targets(t));
    free(blk);
    skb_destroy(t);
    skb_destroy(NULL);
    return rc ? 6 : 0;
}
