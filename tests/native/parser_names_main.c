/* The record parser (strainer2_amd/csrc/sk_parser.h) with and without its name sink compiled in: prints every record it hands
 * out and how the file ended, so that three builds of this file can be compared on one input --
 *   plain                      the parser as every reader but the region table compiles it
 *   -DSKP_NAME_SINK            the sink compiled in, none set
 *   -DSKP_NAME_SINK -DUSE_SINK a sink set: the names go to stderr, one per line
 * usage: parser_names_main FILE BLOCK_BYTES */
#include <stdio.h>
#include "../../strainer2_amd/csrc/sk_parser.h"

static int on_record(void *user, char *seq, size_t len)
{
    (void)user;
    printf("%zu\t", len);
    fwrite(seq, 1, len, stdout);
    putchar('\n');
    return 0;
}

#ifdef USE_SINK
static int on_name(void *user, const char *name, size_t len)
{
    (void)user;
    fwrite(name, 1, len, stderr);
    fputc('\n', stderr);
    return 0;
}
#endif

int main(int argc, char **argv)
{
    parser ps;
    FILE *f;
    unsigned char *blk;
    size_t n, bs;
    if (argc != 3 || !(f = fopen(argv[1], "rb"))) return 2;
    bs = (size_t)atol(argv[2]);
    if (bs < 1 || !(blk = (unsigned char *)malloc(bs))) return 2;
    parser_init(&ps, on_record, NULL);
#ifdef USE_SINK
    parser_set_name_sink(&ps, on_name);
#endif
    while (ps.state != P_STOP && (n = fread(blk, 1, bs, f)) > 0) parser_feed(&ps, blk, n);
    parser_eof(&ps);
    printf("records %lld end %d len %zu\n", (long long)ps.nrecords, ps.end_kind, ps.end_len);
    parser_free(&ps);
    free(blk);
    fclose(f);
    return 0;
}
