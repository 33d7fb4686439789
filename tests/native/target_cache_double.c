/* target_cache_double.c -- strain_detect's host layer with the target cache (sk_host_sd.c: the writer thread, the serving thread;
 * strainer2_amd/csrc/sk_pcache.h: the version-2 file) over the CPU device double, as a stand-alone program for
 * tests/test_target_cache_host.py (-fsanitize=address,undefined and again -fsanitize=thread).  It includes device_double.c and leaves
 * sk_batch_pack_home / sk_batch_pack_wait ABSENT: they are weak references in sk_host_sd.c, and without them the writer packs with
 * sk_pack_stream, so the whole flow -- off, filling, served -- runs on the CPU.
 *   target_cache_double <strain_detect's command line>     the program
 *   target_cache_double --format-drive <empty directory>   the version-2 reader and writer on their own; prints "ok"
 * TEST CODE only. */
#define _GNU_SOURCE
#define DOUBLE_NO_MAIN
#include "device_double.c"
#include <sys/stat.h>
#include <unistd.h>
#include "../../strainer2_amd/csrc/sk_pcache.h"

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "target_cache_double: line %d: %s\n", __LINE__, #c); exit(1); } } while (0)

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

/* a chunk as sd_on_record lays it down: records of the given lengths, those of k bases or more in the stream */
typedef struct { uint32_t kind, nrec, np; uint64_t stream_len; uint8_t *payload; uint64_t plen; } seg_made;

static seg_made make_seg(const uint32_t *len, uint32_t nrec, int as_bytes)
{
    seg_made m;
    uint8_t *stream;
    uint64_t at = 0, part;
    uint32_t i, j;
    int odd = 0;
    memset(&m, 0, sizeof m);
    m.nrec = nrec;
    for (i = 0; i < nrec; i++) if (len[i] >= SKPC_K) { m.stream_len += (uint64_t)len[i] + 1u; m.np++; }
    stream = malloc(m.stream_len + 16);
    for (i = 0; i < nrec; i++) {
        if (len[i] < SKPC_K) continue;
        for (j = 0; j < len[i]; j++) stream[at++] = (uint8_t)"ACGT"[(i * 7u + j * 3u + (j >> 2)) & 3u];
        stream[at++] = '\n';
    }
    if (as_bytes && m.stream_len) stream[0] = 'R';
    m.kind = as_bytes && m.stream_len ? SKPC_BYTES : SKPC_PACKED;
    part = skpt_stream_part(m.kind, m.stream_len);
    m.plen = skpt_payload_len(m.kind, m.stream_len, nrec);
    m.payload = calloc(1, m.plen + 8);
    if (m.kind == SKPC_BYTES) memcpy(m.payload, stream, m.stream_len);
    else if (m.stream_len) { CHECK(sk_pack_stream(stream, m.stream_len, m.payload, &odd) == SK_OK); CHECK(!odd); }
    for (i = 0; i < nrec; i++) skpc_put32(m.payload + part + 4u * i, len[i]);
    free(stream);
    return m;
}

static int walk(const char *path, const struct stat *src, const seg_made *want, unsigned nwant)
{
    skpc_reader r;
    skpt_seg sg;
    unsigned i = 0;
    int rc = skpt_open(&r, path, src);
    if (rc != SKPC_OK) return rc;
    for (;;) {
        uint8_t *buf;
        rc = skpt_next(&r, &sg);
        if (rc == SKPC_MISS) { rc = SKPC_OK; break; }
        if (rc != SKPC_OK) break;
        buf = malloc(sg.payload_len + 8);
        rc = skpt_payload(&r, &sg, buf, NULL, NULL);
        if (rc == SKPC_OK) rc = skpt_lengths(&sg, buf);
        if (rc == SKPC_OK && want) {
            CHECK(i < nwant && sg.kind == want[i].kind && sg.nrec == want[i].nrec && sg.np == want[i].np && sg.stream_len == want[i].stream_len);
            CHECK(sg.payload_len == want[i].plen && memcmp(buf, want[i].payload, want[i].plen) == 0);
            CHECK(((sg.flags & SKPT_LAST) != 0) == (i + 1 == nwant));
            if (i + 1 == nwant) CHECK(sg.end_kind == 2 && sg.end_len == 77);
        }
        free(buf);
        if (rc != SKPC_OK) break;
        i++;
    }
    if (rc == SKPC_OK && want) CHECK(i == nwant);
    skpc_close(&r);
    return rc;
}

static int format_drive(const char *dir)
{
    static const uint32_t l0[] = {31, 5, 0, 150, 30, 47}, l1[] = {33, 64}, l2[] = {0, 30, 7}, l3[] = {100};
    char path[700], other[700];
    struct stat src;
    seg_made m[4];
    skpc_writer *w;
    skpc_reader r;
    uint8_t *file, *bad;
    size_t fn, cut;
    uint64_t off[5];
    unsigned i;
    memset(&src, 0, sizeof src);
    src.st_size = 4242; src.st_mtim.tv_sec = 1700000000; src.st_mtim.tv_nsec = 5;
    snprintf(path, sizeof path, "%s/t.fq.0123456789abcdef.skt", dir);
    snprintf(other, sizeof other, "%s/other.skt", dir);
    m[0] = make_seg(l0, 6, 0);
    m[1] = make_seg(l1, 2, 1);                             /* kept as bytes */
    m[2] = make_seg(l2, 3, 0);                             /* every record shorter than k: an EMPTY stream */
    m[3] = make_seg(l3, 1, 0);
    CHECK(m[2].stream_len == 0 && m[2].np == 0 && m[2].plen == 12);

    /* a file given up leaves nothing; a committed one round-trips, the empty-stream segment included */
    CHECK((w = skpt_begin(path, &src)) != NULL);
    skpt_append(w, m[0].kind, m[0].stream_len, m[0].nrec, m[0].np, 0, 0, 0, m[0].payload);
    CHECK(skpc_end(w, 0, 0, 0) == 0 && access(path, F_OK) != 0);
    CHECK((w = skpt_begin(path, &src)) != NULL);
    off[0] = SKPC_HEADER;
    for (i = 0; i < 4; i++) {
        skpt_append(w, m[i].kind, m[i].stream_len, m[i].nrec, m[i].np, i == 3, 2, 77, m[i].payload);
        off[i + 1] = off[i] + SKPT_SEG_HEADER + skpc_pad8(m[i].plen);
    }
    CHECK(skpc_end(w, 1, 12, 537) == 1);
    CHECK(walk(path, &src, m, 4) == SKPC_OK);
    file = slurp(path, &fn);
    CHECK(fn == off[4]);
    CHECK(skpt_open(&r, path, &src) == SKPC_OK);
    CHECK(r.h.version == 2 && r.h.segments == 4 && r.h.records == 12 && r.h.bases == 537 && r.h.chunk_cap == m[0].stream_len);
    skpc_close(&r);

    /* another source size or mtime: not this target's cache */
    { struct stat s2 = src; s2.st_size++; CHECK(walk(path, &s2, NULL, 0) == SKPC_INVALID); }
    { struct stat s2 = src; s2.st_mtim.tv_nsec++; CHECK(walk(path, &s2, NULL, 0) == SKPC_INVALID); }
    /* a version-1 reader rejects a .skt */
    CHECK(skpc_open(&r, path, &src, 1u << 30) == SKPC_INVALID);

    /* cut at every segment boundary, inside a segment header and inside a payload; lengthened */
    for (i = 0; i < 4; i++) {
        spit(other, file, (size_t)off[i]);
        CHECK(walk(other, &src, NULL, 0) == SKPC_INVALID);
        spit(other, file, (size_t)off[i] + 17);
        CHECK(walk(other, &src, NULL, 0) == SKPC_INVALID);
        spit(other, file, (size_t)off[i] + SKPT_SEG_HEADER + (size_t)m[i].plen / 2);
        CHECK(walk(other, &src, NULL, 0) == SKPC_INVALID);
    }
    bad = malloc(fn + 8);
    memcpy(bad, file, fn); memset(bad + fn, 0, 8);
    spit(other, bad, fn + 8);
    CHECK(walk(other, &src, NULL, 0) == SKPC_INVALID);

    /* a wrong version under a header sum that holds */
    memcpy(bad, file, fn);
    skpc_put32(bad + 8, 3); skpc_put64(bad + 120, skpc_sum64(bad, 120));
    spit(other, bad, fn);
    CHECK(walk(other, &src, NULL, 0) == SKPC_INVALID);
    /* a segment count that the size does not bear (one segment dropped from the header, the sum made good) */
    memcpy(bad, file, fn);
    skpc_put64(bad + 56, 3); skpc_put64(bad + 120, skpc_sum64(bad, 120));
    spit(other, bad, fn);
    CHECK(walk(other, &src, NULL, 0) == SKPC_INVALID);

    /* one payload byte flipped in the second segment: the first is served, the second is CORRUPT */
    memcpy(bad, file, fn);
    bad[off[1] + SKPT_SEG_HEADER + 3] ^= 0x10;
    spit(other, bad, fn);
    CHECK(walk(other, &src, NULL, 0) == SKPC_CORRUPT);
    /* one length changed and the segment's sum recomputed: the structure check says so */
    for (cut = 0; cut < 2; cut++) {
        const uint64_t part = skpt_stream_part(m[0].kind, m[0].stream_len);
        uint8_t *pl = bad + off[0] + SKPT_SEG_HEADER;
        memcpy(bad, file, fn);
        skpc_put32(pl + part + 4u * (cut ? 1u : 3u), cut ? 31u : 149u);    /* a short record made long: np and the stream; a long one shortened: the stream */
        skpc_put64(bad + off[0] + 24, skpc_sum64(pl, m[0].plen));
        spit(other, bad, fn);
        CHECK(walk(other, &src, NULL, 0) == SKPC_CORRUPT);
    }
    /* segment headers that cannot be: the last flag early, an unknown kind, a record count the payload length does not bear */
    memcpy(bad, file, fn); skpc_put32(bad + off[0] + 4, SKPT_LAST); spit(other, bad, fn); CHECK(walk(other, &src, NULL, 0) == SKPC_CORRUPT);
    memcpy(bad, file, fn); skpc_put32(bad + off[3] + 4, 0); spit(other, bad, fn); CHECK(walk(other, &src, NULL, 0) == SKPC_CORRUPT);
    memcpy(bad, file, fn); skpc_put32(bad + off[1], 3); spit(other, bad, fn); CHECK(walk(other, &src, NULL, 0) == SKPC_CORRUPT);
    memcpy(bad, file, fn); skpc_put32(bad + off[2] + 32, 4); spit(other, bad, fn); CHECK(walk(other, &src, NULL, 0) == SKPC_CORRUPT);
    memcpy(bad, file, fn); skpc_put64(bad + off[2] + 8, 32); spit(other, bad, fn); CHECK(walk(other, &src, NULL, 0) == SKPC_CORRUPT);
    unlink(other);

    /* a .skp offered as a .skt */
    {
        skpc_writer *w1 = skpc_begin(other, &src, 4096);
        CHECK(w1 != NULL);
        skpc_append(w1, SKPC_BYTES, 5, "ACGTN");
        CHECK(skpc_end(w1, 1, 1, 5) == 1);
        CHECK(skpt_open(&r, other, &src) == SKPC_INVALID);
        CHECK(skpc_open(&r, other, &src, 4096) == SKPC_OK);
        skpc_close(&r);
        unlink(other);
    }
    /* the name */
    {
        char *a = skpc_path(dir, path), *b = skpt_path(dir, path);
        CHECK(a && b && strlen(a) == strlen(b) && !strncmp(a, b, strlen(a) - 1) && !strcmp(a + strlen(a) - 4, ".skp") && !strcmp(b + strlen(b) - 4, ".skt"));
        free(a); free(b);
    }
    CHECK(skpt_open(&r, other, &src) == SKPC_MISS);
    unlink(path);
    for (i = 0; i < 4; i++) free(m[i].payload);
    free(file); free(bad);
    puts("ok");
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 3 && !strcmp(argv[1], "--format-drive")) return format_drive(argv[2]);
    return skh_strain_detect_main(argc, argv, stdout, stderr);
}
