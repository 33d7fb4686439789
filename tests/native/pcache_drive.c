/* pcache_drive.c -- a stand-alone driver for the packed input cache, built with -fsanitize=address,undefined by
 * tests/test_pack_cache_host.py and linked with the CPU device double (pcache_double.c) and the host layer:
 *   part 1  the file format's writer and reader (strainer2_amd/csrc/sk_pcache.h) on their own: round trip over segment lengths around
 *           the 16-byte chunk, a file given up, files cut short, lengthened, with a flipped bit in header, segment header and payload,
 *           a source of another size or mtime, a chunk cap above the reader's buffers;
 *   part 2  skh_scan_file and skh_scan_list through skh_pack_cache_set over the double: fill, serve, off -- the same counters --
 *           and what skh_pack_cache_stats says.
 * usage: pcache_drive <empty work directory>; prints "ok" and exits 0, or says what failed and exits 1.  TEST CODE only. */
#define _GNU_SOURCE
#include <dirent.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>
#include <sys/wait.h>
#include <unistd.h>
#include "../../include/strainer_kmer.h"
#include "../../strainer2_amd/csrc/sk_pcache.h"

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "pcache_drive: line %d: %s\n", __LINE__, #c); exit(1); } } while (0)

static int count_files(const char *dir)
{
    DIR *d = opendir(dir);
    struct dirent *e;
    int n = 0;
    CHECK(d != NULL);
    while ((e = readdir(d)) != NULL) n += e->d_name[0] != '.';
    closedir(d);
    return n;
}

static uint8_t *slurp(const char *path, size_t *n)
{
    FILE *f = fopen(path, "rb");
    uint8_t *b;
    CHECK(f != NULL);
    fseek(f, 0, SEEK_END);
    *n = (size_t)ftell(f);
    fseek(f, 0, SEEK_SET);
    b = malloc(*n + 1);
    CHECK(fread(b, 1, *n, f) == *n);
    fclose(f);
    return b;
}

static void spit(const char *path, const uint8_t *b, size_t n)
{
    FILE *f = fopen(path, "wb");
    CHECK(f != NULL && fwrite(b, 1, n, f) == n);
    fclose(f);
}

static void format_checks(const char *dir)
{
    static const uint64_t lens[] = {1, 15, 16, 17, 31, 32, 33, 47, 4095, 4096};
    enum { NL = sizeof lens / sizeof lens[0] };
    char path[600], other[600];
    struct stat src;
    skpc_writer *w;
    skpc_reader r;
    skpc_seg sg;
    uint8_t *payload[NL], *buf = malloc(8192), *file;
    size_t fn;
    unsigned i;
    memset(&src, 0, sizeof src);
    src.st_size = 12345; src.st_mtim.tv_sec = 1700000000; src.st_mtim.tv_nsec = 123456789;
    snprintf(path, sizeof path, "%s/a.skp", dir);

    /* a file given up leaves nothing */
    CHECK((w = skpc_begin(path, &src, 4096)) != NULL);
    CHECK(count_files(dir) == 1);
    skpc_append(w, SKPC_BYTES, 5, "ACGTN");
    CHECK(skpc_end(w, 0, 0, 0) == 0);
    CHECK(count_files(dir) == 0);

    /* what a killed process left behind is removed by the next fill of the same item; a living process's temporary is not */
    {
        char dead[700], live[700], near[700];
        const pid_t child = fork();
        int st;
        CHECK(child >= 0);
        if (child == 0) _exit(0);
        CHECK(waitpid(child, &st, 0) == child);
        snprintf(dead, sizeof dead, "%s.tmp.%ld.7", path, (long)child);
        snprintf(live, sizeof live, "%s.tmp.%ld.7", path, (long)getppid());
        snprintf(near, sizeof near, "%s/aa.skp.tmp.%ld.7", dir, (long)child);      /* (another item's: not this fill's business) */
        spit(dead, (const uint8_t *)"x", 1); spit(live, (const uint8_t *)"x", 1); spit(near, (const uint8_t *)"x", 1);
        CHECK((w = skpc_begin(path, &src, 4096)) != NULL);
        CHECK(access(dead, F_OK) != 0 && access(live, F_OK) == 0 && access(near, F_OK) == 0);
        CHECK(skpc_end(w, 0, 0, 0) == 0);
        unlink(live); unlink(near);
        CHECK(count_files(dir) == 0);
    }

    /* round trip: packed and byte segments in turn */
    CHECK((w = skpc_begin(path, &src, 4096)) != NULL);
    for (i = 0; i < NL; i++) {
        const uint32_t kind = i & 1 ? SKPC_BYTES : SKPC_PACKED;
        const uint64_t plen = kind == SKPC_PACKED ? skpc_packed_bytes(lens[i]) : lens[i];
        uint64_t j;
        payload[i] = malloc(plen);
        for (j = 0; j < plen; j++) payload[i][j] = (uint8_t)(31 * i + 7 * j + (j >> 8));
        skpc_append(w, kind, lens[i], payload[i]);
    }
    CHECK(skpc_end(w, 1, 77, 9999) == 1);
    CHECK(count_files(dir) == 1);
    CHECK(skpc_open(&r, path, &src, 4096) == SKPC_OK);
    CHECK(r.h.records == 77 && r.h.bases == 9999 && r.h.segments == NL && r.h.chunk_cap == 4096);
    for (i = 0; i < NL; i++) {
        double t = 0;
        CHECK(skpc_next(&r, &sg) == SKPC_OK);
        CHECK(sg.kind == (i & 1 ? SKPC_BYTES : SKPC_PACKED) && sg.stream_len == lens[i]);
        CHECK(skpc_payload(&r, &sg, buf, &t) == SKPC_OK);
        CHECK(memcmp(buf, payload[i], sg.payload_len) == 0);
    }
    CHECK(skpc_next(&r, &sg) == SKPC_MISS);
    skpc_close(&r);

    /* no file; another source; buffers too small */
    snprintf(other, sizeof other, "%s/none.skp", dir);
    CHECK(skpc_open(&r, other, &src, 4096) == SKPC_MISS);
    src.st_size++;
    CHECK(skpc_open(&r, path, &src, 4096) == SKPC_INVALID);
    src.st_size--; src.st_mtim.tv_nsec++;
    CHECK(skpc_open(&r, path, &src, 4096) == SKPC_INVALID);
    src.st_mtim.tv_nsec--;
    CHECK(skpc_open(&r, path, &src, 4095) == SKPC_INVALID);

    /* cut short, lengthened, a bit flipped in the header */
    file = slurp(path, &fn);
    snprintf(other, sizeof other, "%s/b.skp", dir);
    spit(other, file, fn - 1);
    CHECK(skpc_open(&r, other, &src, 4096) == SKPC_INVALID);
    spit(other, file, SKPC_HEADER - 1);
    CHECK(skpc_open(&r, other, &src, 4096) == SKPC_INVALID);
    file[fn] = 0;
    spit(other, file, fn + 1);
    CHECK(skpc_open(&r, other, &src, 4096) == SKPC_INVALID);
    for (i = 0; i < SKPC_HEADER; i += 5) {
        file[i] ^= 0x10;
        spit(other, file, fn);
        CHECK(skpc_open(&r, other, &src, 4096) == SKPC_INVALID);
        file[i] ^= 0x10;
    }
    /* a bit flipped in every byte of the first segment's payload in turn, and in the second's */
    for (i = 0; i < 6 + 15; i++) {
        const size_t at = i < 6 ? SKPC_HEADER + SKPC_SEG_HEADER + i : SKPC_HEADER + 2 * SKPC_SEG_HEADER + 8 + (i - 6);
        file[at] ^= 1u << (i & 7);
        spit(other, file, fn);
        CHECK(skpc_open(&r, other, &src, 4096) == SKPC_OK);
        CHECK(skpc_next(&r, &sg) == SKPC_OK);
        if (i < 6) CHECK(skpc_payload(&r, &sg, buf, NULL) == SKPC_CORRUPT);
        else {
            CHECK(skpc_payload(&r, &sg, buf, NULL) == SKPC_OK);
            CHECK(skpc_next(&r, &sg) == SKPC_OK);
            CHECK(skpc_payload(&r, &sg, buf, NULL) == SKPC_CORRUPT);
        }
        skpc_close(&r);
        file[at] ^= 1u << (i & 7);
    }
    /* segment headers that cannot be: a stream longer than the cap, a payload of the wrong length, a kind that is none */
    for (i = 0; i < 3; i++) {
        const size_t at = SKPC_HEADER + (i == 0 ? 9 : i == 1 ? 16 : 0);
        const uint8_t was = file[at];
        file[at] = i == 0 ? 0x40 : i == 1 ? 7 : 3;
        spit(other, file, fn);
        CHECK(skpc_open(&r, other, &src, 4096) == SKPC_OK);
        CHECK(skpc_next(&r, &sg) == SKPC_CORRUPT);
        skpc_close(&r);
        file[at] = was;
    }
    unlink(other); unlink(path);
    for (i = 0; i < NL; i++) free(payload[i]);
    free(buf); free(file);
}

static void write_reads(const char *path, const char *strain, size_t sl, unsigned seed, int n, int crlf)
{
    FILE *f = fopen(path, "w");
    int i;
    CHECK(f != NULL);
    for (i = 0; i < n; i++) {
        size_t len, at, j;
        seed = seed * 1103515245u + 12345u;
        len = 31 + (seed >> 16) % 400;
        seed = seed * 1103515245u + 12345u;
        at = (seed >> 8) % (sl - len);
        fprintf(f, ">r%d%s\n", i, crlf ? "\r" : "");
        for (j = 0; j < len; j++) fputc(i % 7 == 3 && j == 40 ? 'R' : i % 5 == 1 && j == 33 ? 'N' : strain[at + j], f);
        fprintf(f, "%s\n", crlf ? "\r" : "");
    }
    fclose(f);
}

static void host_checks(const char *dir)
{
    enum { SL = 6000, NREADS = 300 };
    char strain[SL + 2], a[600], b[600], c[600], list[600], cache[600];
    skh_keyset ks;
    sk_ctx *ctx = NULL;
    uint32_t *want, *got, n;
    uint64_t served, written, stale, notc, bases_fill = 0, bases_serve = 0;
    unsigned seed = 99, i;
    int pass;
    FILE *f;
    for (i = 0; i < SL; i++) { seed = seed * 1103515245u + 12345u; strain[i] = "ACGT"[(seed >> 16) & 3]; }
    strain[SL] = '\n'; strain[SL + 1] = 0;
    snprintf(a, sizeof a, "%s/a.fa", dir); snprintf(b, sizeof b, "%s/b.fa", dir); snprintf(c, sizeof c, "%s/c_crlf.fa", dir);
    snprintf(list, sizeof list, "%s/list.txt", dir); snprintf(cache, sizeof cache, "%s/cache", dir);
    write_reads(a, strain, SL, 1, NREADS, 0);
    write_reads(b, strain, SL, 2, NREADS, 0);
    write_reads(c, strain, SL, 3, 40, 1);
    CHECK((f = fopen(list, "w")) != NULL);
    fprintf(f, "%s\n%s\n%s\n", a, b, c);
    fclose(f);
    setenv("SK_CHUNK_BYTES", "4096", 1);
    setenv("SK_THREADS", "3", 1);
    unsetenv("SK_PACK_CACHE");
    CHECK(skh_keyset_from_stream(&ks, strain, SL + 1, 1000, 1, 1) == SK_OK);
    CHECK(sk_ctx_create(&ctx, 0) == SK_OK);
    CHECK(skh_keyset_load(ctx, &ks, 4) == SK_OK);
    n = ks.nrows;
    want = malloc((size_t)n * 4); got = malloc((size_t)n * 4);

    /* the list, and one file alone, with the cache off */
    CHECK(skh_scan_list(ctx, list, NULL, 1, NULL, stderr, 0, 1, NULL) == SK_OK);
    CHECK(skh_scan_file(ctx, a, 1, NULL) == SK_OK);
    CHECK(sk_counts_fetch(ctx, 1, want) == SK_OK);
    for (i = 0, served = 0; i < n; i++) served += want[i];
    CHECK(served > 1000);                                        /* (the reads are the strain's: there is something to compare) */
    CHECK(skh_pack_cache_stats(ctx, &served, &written, &stale, &notc, 0) == SK_OK && served + written + stale + notc == 0);

    CHECK(skh_pack_cache_set(ctx, cache, "sometimes") == SK_E_ARG);
    for (pass = 0; pass < 3; pass++) {                           /* fill, serve, read-only serve */
        uint64_t bases = 0;
        CHECK(skh_pack_cache_set(ctx, cache, pass == 2 ? "ro" : "rw") == SK_OK);
        CHECK(sk_counts_zero(ctx, 1) == SK_OK);
        CHECK(skh_scan_list(ctx, list, NULL, 1, NULL, stderr, 0, 1, &bases) == SK_OK);
        CHECK(skh_scan_file(ctx, a, 1, &bases) == SK_OK);
        CHECK(sk_counts_fetch(ctx, 1, got) == SK_OK);
        CHECK(memcmp(want, got, (size_t)n * 4) == 0);
        CHECK(skh_pack_cache_stats(ctx, &served, &written, &stale, &notc, 1) == SK_OK);
        if (pass == 0) { CHECK(served == 1 && written == 3 && stale == 0 && notc == 0); bases_fill = bases; }
        else { CHECK(served == 4 && written == 0 && stale == 0 && notc == 0); bases_serve = bases; }
        CHECK(count_files(cache) == 3);
    }
    CHECK(bases_fill == bases_serve && bases_fill > 0);
    /* off for this context again: nothing is counted as served */
    CHECK(skh_pack_cache_set(ctx, "", NULL) == SK_OK);
    CHECK(sk_counts_zero(ctx, 1) == SK_OK);
    CHECK(skh_scan_list(ctx, list, NULL, 1, NULL, stderr, 0, 1, NULL) == SK_OK);
    CHECK(skh_scan_file(ctx, a, 1, NULL) == SK_OK);
    CHECK(sk_counts_fetch(ctx, 1, got) == SK_OK);
    CHECK(memcmp(want, got, (size_t)n * 4) == 0);
    CHECK(skh_pack_cache_stats(ctx, &served, &written, &stale, &notc, 0) == SK_OK && served + written + stale + notc == 0);
    CHECK(skh_pack_cache_set(ctx, NULL, NULL) == SK_OK);
    free(want); free(got);
    skh_keyset_free(&ks);
    sk_ctx_destroy(ctx);
}

int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: pcache_drive <empty work directory>\n"); return 2; }
    format_checks(argv[1]);
    host_checks(argv[1]);
    puts("ok");
    return 0;
}
