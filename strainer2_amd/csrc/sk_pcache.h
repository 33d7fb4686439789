/* sk_pcache.h -- the list scan's packed input cache (internal, header-only as sk_pack.h is: sk_host.c includes it, and so does the
 * stand-alone test driver tests/native/pcache_drive.c).
 *
 * The -A/-B lists are a background panel: the same genomes and metagenomes are scanned again for every new strain.  What a decode
 * thread hands to the device for one list item -- chunks of the record stream, whole records or pieces cut with the k-1 overlap --
 * is kept here in the form sk_pack_stream makes of it (6 bytes per 16 bases), one file per item, so that a later run reads 0.375
 * bytes per base out of the page cache and submits them: no inflate, no parse, no pack.
 *
 * File  DIR/<basename>.<16 hex digits of FNV-1a-64 of the item's realpath>.skp, little-endian:
 *   header, 128 bytes
 *       0  magic "SKPCACHE"            8  u32 version (1)            12  u32 k (31)
 *      16  u64 chunk cap (the largest stream length a segment may have: the writer's SK_CHUNK_BYTES)
 *      24  u64 source size            32  i64 source mtime, nanoseconds
 *      40  u64 records                48  u64 bases (sum of the records' lengths, short ones included)
 *      56  u64 segments               64  u64 payload bytes on disk (every payload padded to 8)
 *      72  zero                      120  u64 skpc_sum64 of bytes 0..119
 *   then per segment: 32 bytes {u32 kind (1 packed, 2 bytes), u32 zero, u64 stream length, u64 payload length, u64 skpc_sum64 of the
 *   payload}, the payload, zero padding to a multiple of 8.  A packed payload is sk_pack_stream's layout for the stream length (the
 *   code words, then the masks); a chunk with a byte for the byte-string kernel (IUPAC, U, CR: *odd) is kept as its bytes.
 *   The file's size is 128 + 32 * segments + payload bytes, exactly: anything else is not a cache file.
 * Version 1 holds chunks for the COUNT scan only; strain_detect's targets need every record's length: version 2, in files of their own
 * (.skt), at the end of this header.  The version-1 format, its reader and its writer are as they were.
 * A file is written under a temporary name (<name>.tmp.<pid>.<n>) and renamed once its item was parsed to the end; an item that fails
 * leaves nothing, and the temporary of a process that was killed is removed by the next fill of the same item. */
#ifndef SK_PCACHE_H
#define SK_PCACHE_H
#include <dirent.h>
#include <errno.h>
#include <fcntl.h>
#include <limits.h>
#include <pthread.h>
#include <signal.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>
#include <sys/uio.h>
#include <time.h>
#include <unistd.h>

#define SKPC_VERSION     1u
#define SKPC_K           31u
#define SKPC_HEADER      128u
#define SKPC_SEG_HEADER  32u
#define SKPC_PACKED      1u
#define SKPC_BYTES       2u
#define SKPC_RW          0
#define SKPC_RO          1

#define SKPC_OK          0
#define SKPC_MISS        1        /* no such file */
#define SKPC_INVALID     2        /* a file that is no valid cache of this source: stale, cut short, another version */
#define SKPC_IO          3        /* read or write failed */
#define SKPC_CORRUPT     4        /* a payload that does not match its checksum */

static inline uint64_t skpc_rotl(uint64_t x, unsigned r) { return (x << r) | (x >> (64u - r)); }
static inline uint64_t skpc_le64(const uint8_t *p)
{
    return (uint64_t)p[0] | (uint64_t)p[1] << 8 | (uint64_t)p[2] << 16 | (uint64_t)p[3] << 24 | (uint64_t)p[4] << 32 | (uint64_t)p[5] << 40 |
           (uint64_t)p[6] << 48 | (uint64_t)p[7] << 56;
}
static inline uint32_t skpc_le32(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }
static inline void skpc_put64(uint8_t *p, uint64_t v) { unsigned i; for (i = 0; i < 8; i++) p[i] = (uint8_t)(v >> (8 * i)); }
static inline void skpc_put32(uint8_t *p, uint32_t v) { unsigned i; for (i = 0; i < 4; i++) p[i] = (uint8_t)(v >> (8 * i)); }

/* The checksum: 64 bits, word by word -- four lanes of 8 bytes, each lane = rotl(lane ^ word, 31) * odd constant (a bijection of the
 * lane for every word, so one changed word always changes its lane), the lanes folded at the end with the length.  No byte table: a
 * table CRC walks a 12 MiB payload at 1-2 GB/s, this at the rate memory delivers it.  Bytes behind the last whole word count as a
 * word padded with zeros. */
static inline uint64_t skpc_word(const uint8_t *p)
{
#if defined(__BYTE_ORDER__) && __BYTE_ORDER__ == __ORDER_LITTLE_ENDIAN__
    uint64_t w;
    memcpy(&w, p, 8);
    return w;
#else
    return skpc_le64(p);
#endif
}
static inline uint64_t skpc_sum64(const void *data, uint64_t n)
{
    const uint8_t *b = (const uint8_t *)data;
    const uint64_t M = 0xFF51AFD7ED558CCDull;
    uint64_t a0 = 0x9E3779B97F4A7C15ull, a1 = 0xC2B2AE3D27D4EB4Full, a2 = 0x165667B19E3779F9ull, a3 = 0x27D4EB2F165667C5ull, left = n, h;
    while (left >= 32) {
        a0 = skpc_rotl(a0 ^ skpc_word(b), 31) * M;
        a1 = skpc_rotl(a1 ^ skpc_word(b + 8), 31) * M;
        a2 = skpc_rotl(a2 ^ skpc_word(b + 16), 31) * M;
        a3 = skpc_rotl(a3 ^ skpc_word(b + 24), 31) * M;
        b += 32; left -= 32;
    }
    while (left >= 8) { a0 = skpc_rotl(a0 ^ skpc_word(b), 31) * M; b += 8; left -= 8; }
    if (left) {
        uint8_t tail[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        memcpy(tail, b, (size_t)left);
        a1 = skpc_rotl(a1 ^ skpc_le64(tail), 31) * M;
    }
    h = a0 ^ skpc_rotl(a1, 17) ^ skpc_rotl(a2, 34) ^ skpc_rotl(a3, 51) ^ (n * M);
    h ^= h >> 33; h *= 0xC4CEB9FE1A85EC53ull; h ^= h >> 29;
    return h;
}

static inline double skpc_now(void) { struct timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec; }
static inline uint64_t skpc_packed_bytes(uint64_t n) { return ((n + 15u) >> 4) * 6u; }
static inline uint64_t skpc_pad8(uint64_t n) { return (n + 7u) & ~(uint64_t)7u; }

typedef struct {
    uint32_t version, k;
    uint64_t chunk_cap, src_size;
    int64_t  src_mtime;
    uint64_t records, bases, segments, payload_bytes;
} skpc_header;

static inline void skpc_header_put(const skpc_header *h, uint8_t out[SKPC_HEADER])
{
    memset(out, 0, SKPC_HEADER);
    memcpy(out, "SKPCACHE", 8);
    skpc_put32(out + 8, h->version); skpc_put32(out + 12, h->k);
    skpc_put64(out + 16, h->chunk_cap); skpc_put64(out + 24, h->src_size); skpc_put64(out + 32, (uint64_t)h->src_mtime);
    skpc_put64(out + 40, h->records); skpc_put64(out + 48, h->bases); skpc_put64(out + 56, h->segments); skpc_put64(out + 64, h->payload_bytes);
    skpc_put64(out + 120, skpc_sum64(out, 120));
}

/* 0: a header of this format whose checksum holds (version and k are the caller's to compare) */
static inline int skpc_header_get(const uint8_t in[SKPC_HEADER], skpc_header *h)
{
    if (memcmp(in, "SKPCACHE", 8) != 0 || skpc_le64(in + 120) != skpc_sum64(in, 120)) return -1;
    h->version = skpc_le32(in + 8); h->k = skpc_le32(in + 12);
    h->chunk_cap = skpc_le64(in + 16); h->src_size = skpc_le64(in + 24); h->src_mtime = (int64_t)skpc_le64(in + 32);
    h->records = skpc_le64(in + 40); h->bases = skpc_le64(in + 48); h->segments = skpc_le64(in + 56); h->payload_bytes = skpc_le64(in + 64);
    return 0;
}

static inline int64_t skpc_mtime_ns(const struct stat *st) { return (int64_t)st->st_mtim.tv_sec * 1000000000ll + (int64_t)st->st_mtim.tv_nsec; }

/* the cache file's name for a list item (malloc'd), or NULL: the item has no realpath (it does not exist) */
static inline char *skpc_path(const char *dir, const char *item)
{
    char real[PATH_MAX], *out;
    const char *base;
    uint64_t h = 0xCBF29CE484222325ull;
    size_t i, n;
    if (!realpath(item, real)) return NULL;
    for (i = 0; real[i]; i++) { h ^= (uint8_t)real[i]; h *= 0x100000001B3ull; }
    base = strrchr(real, '/');
    base = base ? base + 1 : real;
    n = strlen(dir) + strlen(base) + 32;
    if (!(out = (char *)malloc(n))) return NULL;
    snprintf(out, n, "%s/%s.%016llx.skp", dir, base, (unsigned long long)h);
    return out;
}

static inline int skpc_read_all(int fd, void *buf, uint64_t n, uint64_t off)
{
    uint8_t *p = (uint8_t *)buf;
    while (n) {
        const ssize_t r = pread(fd, p, (size_t)n, (off_t)off);
        if (r < 0 && errno == EINTR) continue;
        if (r <= 0) return -1;
        p += r; off += (uint64_t)r; n -= (uint64_t)r;
    }
    return 0;
}

/* ---- reader ---------------------------------------------------------------------------------------------------------------- */
typedef struct { int fd; skpc_header h; uint64_t seg, off, size; } skpc_reader;
typedef struct { uint32_t kind; uint64_t stream_len, payload_len, sum, payload_off; } skpc_seg;

/* Opens `path` and decides whether it is a cache of the source that `src` describes: SKPC_OK (the reader stands before segment 0),
 * SKPC_MISS (no file), SKPC_INVALID (not this format or version, another k, another source size or mtime, a file whose size is not
 * what its header implies, a chunk cap above max_chunk -- the caller's buffers). */
static inline int skpc_open(skpc_reader *r, const char *path, const struct stat *src, uint64_t max_chunk)
{
    uint8_t hb[SKPC_HEADER];
    struct stat st;
    memset(r, 0, sizeof *r);
    r->fd = open(path, O_RDONLY | O_CLOEXEC);
    if (r->fd < 0) return errno == ENOENT ? SKPC_MISS : SKPC_INVALID;
    if (fstat(r->fd, &st) != 0 || !S_ISREG(st.st_mode) || (uint64_t)st.st_size < SKPC_HEADER || skpc_read_all(r->fd, hb, SKPC_HEADER, 0) != 0 ||
        skpc_header_get(hb, &r->h) != 0 || r->h.version != SKPC_VERSION || r->h.k != SKPC_K ||
        r->h.src_size != (uint64_t)src->st_size || r->h.src_mtime != skpc_mtime_ns(src) || r->h.chunk_cap > max_chunk ||
        r->h.segments > ((uint64_t)st.st_size - SKPC_HEADER) / SKPC_SEG_HEADER ||
        (uint64_t)st.st_size != SKPC_HEADER + r->h.segments * SKPC_SEG_HEADER + r->h.payload_bytes) {
        close(r->fd);
        r->fd = -1;
        return SKPC_INVALID;
    }
    r->size = (uint64_t)st.st_size;
    r->off = SKPC_HEADER;
    return SKPC_OK;
}

static inline void skpc_close(skpc_reader *r) { if (r->fd >= 0) close(r->fd); r->fd = -1; }

/* the next segment's header: SKPC_OK, SKPC_MISS after the last one, SKPC_CORRUPT for a header that cannot be (a kind that is none, a
 * stream longer than the chunk cap, a payload of the wrong length for its stream, one that runs past the file's end), SKPC_IO */
static inline int skpc_next(skpc_reader *r, skpc_seg *s)
{
    uint8_t sb[SKPC_SEG_HEADER];
    if (r->seg >= r->h.segments) return r->off == r->size ? SKPC_MISS : SKPC_CORRUPT;
    if (r->off + SKPC_SEG_HEADER > r->size) return SKPC_CORRUPT;
    if (skpc_read_all(r->fd, sb, SKPC_SEG_HEADER, r->off) != 0) return SKPC_IO;
    s->kind = skpc_le32(sb); s->stream_len = skpc_le64(sb + 8); s->payload_len = skpc_le64(sb + 16); s->sum = skpc_le64(sb + 24);
    s->payload_off = r->off + SKPC_SEG_HEADER;
    if ((s->kind != SKPC_PACKED && s->kind != SKPC_BYTES) || skpc_le32(sb + 4) != 0 || s->stream_len == 0 || s->stream_len > r->h.chunk_cap ||
        s->payload_len != (s->kind == SKPC_PACKED ? skpc_packed_bytes(s->stream_len) : s->stream_len) ||
        skpc_pad8(s->payload_len) > r->size - s->payload_off)
        return SKPC_CORRUPT;
    r->off = s->payload_off + skpc_pad8(s->payload_len);
    r->seg++;
    return SKPC_OK;
}

/* the segment's payload into buf (room for payload_len): SKPC_OK, SKPC_IO, or SKPC_CORRUPT when it does not match its checksum;
 * *t_sum (may be NULL) grows by the seconds the checksum took */
static inline int skpc_payload(const skpc_reader *r, const skpc_seg *s, void *buf, double *t_sum)
{
    double t0;
    uint64_t sum;
    if (skpc_read_all(r->fd, buf, s->payload_len, s->payload_off) != 0) return SKPC_IO;
    t0 = t_sum ? skpc_now() : 0.0;
    sum = skpc_sum64(buf, s->payload_len);
    if (t_sum) *t_sum += skpc_now() - t0;
    return sum == s->sum ? SKPC_OK : SKPC_CORRUPT;
}

/* ---- writer ---------------------------------------------------------------------------------------------------------------- */
typedef struct {
    int             fd, err;
    char           *tmp, *final;
    skpc_header     h;
    pthread_mutex_t mu;             /* the helper threads of a split .gz item append to one file */
    double          t_sum, t_write;
} skpc_writer;

/* A process that was killed while it filled an item leaves <final>.tmp.<pid>.<n> behind (never a half .skp).  Whoever fills the same
 * item next removes those whose process is gone; a temporary of a process that lives (another run filling the same directory) stays. */
static inline void skpc_sweep_tmp(const char *final_path)
{
    const char *slash = strrchr(final_path, '/');
    const char *base = slash ? slash + 1 : final_path;
    const size_t bl = strlen(base), dl = slash ? (size_t)(slash - final_path) : 1;
    char *dir = (char *)malloc(dl + 1), *victim;
    DIR *d;
    struct dirent *e;
    if (!dir) return;
    memcpy(dir, slash ? final_path : ".", dl);
    dir[dl] = '\0';
    if ((d = opendir(dir)) != NULL) {
        while ((e = readdir(d)) != NULL) {
            long pid;
            char *end;
            if (strncmp(e->d_name, base, bl) != 0 || strncmp(e->d_name + bl, ".tmp.", 5) != 0) continue;
            pid = strtol(e->d_name + bl + 5, &end, 10);
            if (end == e->d_name + bl + 5 || *end != '.' || pid <= 0 || pid == (long)getpid()) continue;
            if (kill((pid_t)pid, 0) == 0 || errno != ESRCH) continue;
            if ((victim = (char *)malloc(dl + strlen(e->d_name) + 2)) != NULL) {
                sprintf(victim, "%s/%s", dir, e->d_name);
                unlink(victim);
                free(victim);
            }
        }
        closedir(d);
    }
    free(dir);
}

/* begins DIR's file for the item: the temporary file exists and holds room for the header.  NULL: it cannot be made (the caller
 * goes on uncached). */
static inline skpc_writer *skpc_begin(const char *final_path, const struct stat *src, uint64_t chunk_cap)
{
    static unsigned serial;
    skpc_writer *w = (skpc_writer *)calloc(1, sizeof *w);
    uint8_t zero[SKPC_HEADER];
    size_t n;
    if (!w) return NULL;
    n = strlen(final_path) + 48;
    w->final = strdup(final_path);
    w->tmp = (char *)malloc(n);
    if (!w->final || !w->tmp) { free(w->final); free(w->tmp); free(w); return NULL; }
    skpc_sweep_tmp(final_path);
    snprintf(w->tmp, n, "%s.tmp.%ld.%u", final_path, (long)getpid(), __atomic_add_fetch(&serial, 1, __ATOMIC_RELAXED));
    w->fd = open(w->tmp, O_WRONLY | O_CREAT | O_EXCL | O_CLOEXEC, 0666);
    memset(zero, 0, sizeof zero);
    if (w->fd < 0 || write(w->fd, zero, sizeof zero) != (ssize_t)sizeof zero) {
        if (w->fd >= 0) { close(w->fd); unlink(w->tmp); }
        free(w->final); free(w->tmp); free(w);
        return NULL;
    }
    w->h.version = SKPC_VERSION; w->h.k = SKPC_K; w->h.chunk_cap = chunk_cap;
    w->h.src_size = (uint64_t)src->st_size; w->h.src_mtime = skpc_mtime_ns(src);
    pthread_mutex_init(&w->mu, NULL);
    return w;
}

/* one chunk as it went to the device.  May be called from several threads; a failed write is remembered and ends the file at
 * skpc_end. */
static inline void skpc_append(skpc_writer *w, uint32_t kind, uint64_t stream_len, const void *payload)
{
    static const uint8_t pad[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const uint64_t plen = kind == SKPC_PACKED ? skpc_packed_bytes(stream_len) : stream_len, padded = skpc_pad8(plen);
    uint8_t sb[SKPC_SEG_HEADER];
    struct iovec iov[3];
    double t0 = skpc_now(), t1;
    uint64_t done = 0, total = SKPC_SEG_HEADER + padded;
    int niov = 3, first = 0;
    memset(sb, 0, sizeof sb);
    skpc_put32(sb, kind); skpc_put64(sb + 8, stream_len); skpc_put64(sb + 16, plen); skpc_put64(sb + 24, skpc_sum64(payload, plen));
    t1 = skpc_now();
    iov[0].iov_base = sb; iov[0].iov_len = sizeof sb;
    iov[1].iov_base = (void *)(uintptr_t)payload; iov[1].iov_len = (size_t)plen;
    iov[2].iov_base = (void *)(uintptr_t)pad; iov[2].iov_len = (size_t)(padded - plen);
    pthread_mutex_lock(&w->mu);
    w->t_sum += t1 - t0;
    while (!w->err && done < total) {
        const ssize_t r = writev(w->fd, iov + first, niov - first);
        uint64_t got;
        if (r < 0 && errno == EINTR) continue;
        if (r <= 0) { w->err = 1; break; }
        done += (uint64_t)r;
        for (got = (uint64_t)r; first < niov && got; ) {
            if (got >= iov[first].iov_len) { got -= iov[first].iov_len; first++; }
            else { iov[first].iov_base = (uint8_t *)iov[first].iov_base + got; iov[first].iov_len -= (size_t)got; got = 0; }
        }
    }
    w->h.segments++;
    w->h.payload_bytes += padded;
    w->t_write += skpc_now() - t1;
    pthread_mutex_unlock(&w->mu);
}

/* commit != 0: the item was parsed to the end -- the header goes in and the file takes its name (1 returned); otherwise, or when a
 * write failed, the temporary file is removed (0).  Frees w. */
static inline int skpc_end(skpc_writer *w, int commit, uint64_t records, uint64_t bases)
{
    int ok = commit && !w->err;
    if (ok) {
        uint8_t hb[SKPC_HEADER];
        w->h.records = records; w->h.bases = bases;
        skpc_header_put(&w->h, hb);
        ok = pwrite(w->fd, hb, sizeof hb, 0) == (ssize_t)sizeof hb;
    }
    if (close(w->fd) != 0) ok = 0;
    if (ok && rename(w->tmp, w->final) != 0) ok = 0;
    if (!ok) unlink(w->tmp);
    pthread_mutex_destroy(&w->mu);
    free(w->tmp); free(w->final); free(w);
    return ok;
}

/* ---- version 2: strain_detect's targets (DIR/<basename>.<the same 16 hex digits>.skt) ------------------------------------------
 * The same header (version 2; the chunk cap is the largest stream length that was written, known at the end), other segments: one
 * segment is one chunk of sk_host_sd.c as its consumer sees it -- WHOLE records, and the length of EVERY record, the ones shorter
 * than k included (the replay of the reference's read-after-read bookkeeping needs them).
 *   per segment: 64 bytes { 0 u32 kind (1 packed, 2 bytes)   4 u32 flags (bit 0: the file's last chunk)   8 u64 stream length
 *       16 u64 payload length   24 u64 skpc_sum64 of the payload   32 u32 records   36 u32 records of k bases or more
 *       40 u32 how the parser ended (last chunk only)   44 zero   48 u64 the ending's length (last chunk only)   56 zero },
 *   the payload -- the stream (packed, or its bytes), zero padding to a multiple of 8, then one little-endian u32 length per record
 *   -- and zero padding to a multiple of 8.  ONE sum covers stream, padding and lengths.
 * The stream is what sd_on_record lays down: every record of k bases or more, in order, its bases and a '\n'; so the lengths must
 * reproduce the segment's second record count and its stream length exactly (skpt_lengths), a record of 2^32 bases or more cannot be
 * written, and a segment whose records are all shorter than k has an EMPTY stream (version 1 forbids that; here it is the rule for
 * such a chunk).  The last segment, and only it, carries the last flag; a file without it was never committed.
 * A version-1 reader rejects a .skt and this reader a .skp by the header's version field. */
#define SKPT_VERSION     2u
#define SKPT_SEG_HEADER  64u
#define SKPT_LAST        1u

typedef struct { uint32_t kind, flags, nrec, np, end_kind; uint64_t stream_len, payload_len, sum, end_len, payload_off; } skpt_seg;

static inline uint64_t skpt_stream_part(uint32_t kind, uint64_t stream_len) { return skpc_pad8(kind == SKPC_PACKED ? skpc_packed_bytes(stream_len) : stream_len); }
static inline uint64_t skpt_payload_len(uint32_t kind, uint64_t stream_len, uint32_t nrec) { return skpt_stream_part(kind, stream_len) + 4u * (uint64_t)nrec; }

static inline char *skpt_path(const char *dir, const char *item)
{
    char *out = skpc_path(dir, item);
    if (out) out[strlen(out) - 1] = 't';
    return out;
}

/* skpc_open for a target's file: SKPC_OK, SKPC_MISS or SKPC_INVALID (another version -- a .skp under this name --, another k,
 * source size or mtime, a size that is not what the header implies) */
static inline int skpt_open(skpc_reader *r, const char *path, const struct stat *src)
{
    uint8_t hb[SKPC_HEADER];
    struct stat st;
    memset(r, 0, sizeof *r);
    r->fd = open(path, O_RDONLY | O_CLOEXEC);
    if (r->fd < 0) return errno == ENOENT ? SKPC_MISS : SKPC_INVALID;
    if (fstat(r->fd, &st) != 0 || !S_ISREG(st.st_mode) || (uint64_t)st.st_size < SKPC_HEADER || skpc_read_all(r->fd, hb, SKPC_HEADER, 0) != 0 ||
        skpc_header_get(hb, &r->h) != 0 || r->h.version != SKPT_VERSION || r->h.k != SKPC_K ||
        r->h.src_size != (uint64_t)src->st_size || r->h.src_mtime != skpc_mtime_ns(src) || r->h.segments == 0 ||
        r->h.segments > ((uint64_t)st.st_size - SKPC_HEADER) / SKPT_SEG_HEADER ||
        (uint64_t)st.st_size != SKPC_HEADER + r->h.segments * SKPT_SEG_HEADER + r->h.payload_bytes) {
        close(r->fd);
        r->fd = -1;
        return SKPC_INVALID;
    }
    r->size = (uint64_t)st.st_size;
    r->off = SKPC_HEADER;
    return SKPC_OK;
}

/* the next segment's header: SKPC_OK, SKPC_MISS after the last one, SKPC_CORRUPT for a header that cannot be, SKPC_IO */
static inline int skpt_next(skpc_reader *r, skpt_seg *s)
{
    uint8_t sb[SKPT_SEG_HEADER];
    if (r->seg >= r->h.segments) return r->off == r->size ? SKPC_MISS : SKPC_CORRUPT;
    if (r->off + SKPT_SEG_HEADER > r->size) return SKPC_CORRUPT;
    if (skpc_read_all(r->fd, sb, SKPT_SEG_HEADER, r->off) != 0) return SKPC_IO;
    s->kind = skpc_le32(sb); s->flags = skpc_le32(sb + 4); s->stream_len = skpc_le64(sb + 8); s->payload_len = skpc_le64(sb + 16); s->sum = skpc_le64(sb + 24);
    s->nrec = skpc_le32(sb + 32); s->np = skpc_le32(sb + 36); s->end_kind = skpc_le32(sb + 40); s->end_len = skpc_le64(sb + 48);
    s->payload_off = r->off + SKPT_SEG_HEADER;
    if ((s->kind != SKPC_PACKED && s->kind != SKPC_BYTES) || (s->flags & ~SKPT_LAST) || skpc_le32(sb + 44) != 0 || skpc_le64(sb + 56) != 0 ||
        s->stream_len > r->h.chunk_cap || s->stream_len > 0xFFFFFFF0ull || s->np > s->nrec || (s->np == 0) != (s->stream_len == 0) ||
        ((s->flags & SKPT_LAST) != 0) != (r->seg + 1 == r->h.segments) || (!(s->flags & SKPT_LAST) && (s->end_kind || s->end_len)) ||
        s->payload_len != skpt_payload_len(s->kind, s->stream_len, s->nrec) || skpc_pad8(s->payload_len) > r->size - s->payload_off)
        return SKPC_CORRUPT;
    r->off = s->payload_off + skpc_pad8(s->payload_len);
    r->seg++;
    return SKPC_OK;
}

/* the payload into buf (room for payload_len), its sum checked: SKPC_OK, SKPC_IO, SKPC_CORRUPT */
static inline int skpt_payload(const skpc_reader *r, const skpt_seg *s, void *buf, double *t_sum, double *t_read)
{
    double t0 = skpc_now(), t1;
    uint64_t sum;
    if (s->payload_len && skpc_read_all(r->fd, buf, s->payload_len, s->payload_off) != 0) return SKPC_IO;
    t1 = skpc_now();
    sum = skpc_sum64(buf, s->payload_len);
    if (t_read) *t_read += t1 - t0;
    if (t_sum) *t_sum += skpc_now() - t1;
    return sum == s->sum ? SKPC_OK : SKPC_CORRUPT;
}

/* where the segment's length table lies in its payload */
static inline const uint8_t *skpt_table(const skpt_seg *s, const void *payload) { return (const uint8_t *)payload + skpt_stream_part(s->kind, s->stream_len); }

/* the structure behind a sum that held: the lengths must reproduce the stream -- every record of k bases or more takes its length
 * and a '\n' -- and the count of such records.  SKPC_OK or SKPC_CORRUPT. */
static inline int skpt_lengths(const skpt_seg *s, const void *payload)
{
    const uint8_t *t = skpt_table(s, payload);
    uint64_t at = 0;
    uint32_t i, np = 0;
    for (i = 0; i < s->nrec; i++) {
        const uint32_t l = skpc_le32(t + 4u * (size_t)i);
        if (l >= SKPC_K) { at += (uint64_t)l + 1u; np++; }
    }
    return at == s->stream_len && np == s->np ? SKPC_OK : SKPC_CORRUPT;
}

/* the writer: skpc_begin's temporary file, sweep and rename, skpc_end's commit; the header says version 2 and its chunk cap grows
 * with what is appended */
static inline skpc_writer *skpt_begin(const char *final_path, const struct stat *src)
{
    skpc_writer *w = skpc_begin(final_path, src, 0);
    if (w) w->h.version = SKPT_VERSION;
    return w;
}

/* one chunk: `payload` is the stream part (packed or bytes, padded to 8 with zeros) with the nrec u32 lengths behind it, in one
 * piece of skpt_payload_len(kind, stream_len, nrec) bytes.  From one thread per file, in the file's order. */
static inline void skpt_append(skpc_writer *w, uint32_t kind, uint64_t stream_len, uint32_t nrec, uint32_t np, int last, uint32_t end_kind, uint64_t end_len,
                               const void *payload)
{
    static const uint8_t pad[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const uint64_t plen = skpt_payload_len(kind, stream_len, nrec), padded = skpc_pad8(plen);
    uint8_t sb[SKPT_SEG_HEADER];
    struct iovec iov[3];
    double t0 = skpc_now(), t1;
    uint64_t done = 0, total = SKPT_SEG_HEADER + padded;
    int niov = 3, first = 0;
    memset(sb, 0, sizeof sb);
    skpc_put32(sb, kind); skpc_put32(sb + 4, last ? SKPT_LAST : 0u); skpc_put64(sb + 8, stream_len); skpc_put64(sb + 16, plen);
    skpc_put64(sb + 24, skpc_sum64(payload, plen));
    skpc_put32(sb + 32, nrec); skpc_put32(sb + 36, np); skpc_put32(sb + 40, last ? end_kind : 0u); skpc_put64(sb + 48, last ? end_len : 0u);
    t1 = skpc_now();
    iov[0].iov_base = sb; iov[0].iov_len = sizeof sb;
    iov[1].iov_base = (void *)(uintptr_t)payload; iov[1].iov_len = (size_t)plen;
    iov[2].iov_base = (void *)(uintptr_t)pad; iov[2].iov_len = (size_t)(padded - plen);
    pthread_mutex_lock(&w->mu);
    w->t_sum += t1 - t0;
    while (!w->err && done < total) {
        const ssize_t r = writev(w->fd, iov + first, niov - first);
        uint64_t got;
        if (r < 0 && errno == EINTR) continue;
        if (r <= 0) { w->err = 1; break; }
        done += (uint64_t)r;
        for (got = (uint64_t)r; first < niov && got; ) {
            if (got >= iov[first].iov_len) { got -= iov[first].iov_len; first++; }
            else { iov[first].iov_base = (uint8_t *)iov[first].iov_base + got; iov[first].iov_len -= (size_t)got; got = 0; }
        }
    }
    w->h.segments++;
    w->h.payload_bytes += padded;
    if (stream_len > w->h.chunk_cap) w->h.chunk_cap = stream_len;
    w->t_write += skpc_now() - t1;
    pthread_mutex_unlock(&w->mu);
}
#endif
