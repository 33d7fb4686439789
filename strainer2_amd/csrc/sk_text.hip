// sk_text.hip -- plain FASTA/FASTQ text parsed ON THE DEVICE (gfx950): text in HBM -> record stream in HBM.
//
// What the host's parser (sk_parser.h: the reference's src/kseq.h:171-211) does byte by byte on a CPU thread is, for plain
// text, a line classifier plus a compaction.  Two forms are covered, each exact by induction over verified records from a
// true record boundary (the piece's first byte); whatever they do not cover DECLINES the piece and the host parses it:
//
//   FASTQ4  the piece starts with '@' and its third line with '+': line i has kind i mod 4 (header '@', ONE non-empty
//           sequence line starting with none of > @ +, '+' line, quality line of the sequence's length after the CR rule).
//   FASTA   otherwise, when it starts with '>' or '@': a line starting with > or @ is a header, a line starting with '+'
//           declines (the reference goes into quality mode there), empty lines are skipped, every other line is sequence.
//
// Passes (all integer, bandwidth-shaped; `n` text bytes, T lines):
//   sk_text_mark     16 bytes per lane and load, four loads in flight: '\n' by an exact SWAR compare, newlines per tile
//   sk_text_scan     one workgroup: exclusive scan of a u64 array (tile counts; later the line blocks' {bytes, records})
//   sk_text_lines    the position of every '\n', in order: line i is [nl[i-1] + 1, nl[i])
//   sk_text_records  per line: kind, checks, kept length after the CR rule (src/kseq.h:136), decline flag, last header
//   sk_text_emit     a wave takes 64 consecutive lines, whose kept bytes are ONE contiguous range of the output: every lane
//                    writes aligned words of it and finds each byte's line by a search over the wave's 64 offsets in LDS --
//                    coalesced for 150-byte reads and for a 5 Mbp record of 60-column lines alike
//   sk_text_batch_close  (strain_detect's batches, sk_batch_fill_text) the tile index the TALLY scan reads behind the record starts, by
//                    a lower-bound search per 32 KiB tile, and the starts copied home, 16 bytes per lane
// Ordinary vector loads and stores throughout; the flags are plain atomics.
#include <hip/hip_runtime.h>
#include <pthread.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <map>
#include <new>
#include <vector>
#include "sk_internal.h"

#define TX_TILE     SK_TEXT_TILE          // text bytes per workgroup of sk_text_mark / sk_text_lines
#define TX_THREADS  256
#define TX_LOADS    (TX_TILE / (TX_THREADS * 16))
#define TX_LB       256u                  // lines per workgroup of sk_text_records / sk_text_emit
#define TX_HDR      0x80000000u           // line value: the line is a header (low bits: bytes it puts into the stream)
#define TX_MAX      (256ull << 20)

// what the passes hand each other (device memory, zeroed before every parse)
struct tx_head {
    uint32_t nl;          // '\n' bytes in the text
    uint32_t nlines;      // T: lines, the unterminated last one included
    uint32_t form;        // SK_TEXT_FASTA | SK_TEXT_FASTQ4 | 0 = neither
    uint32_t decline;
    uint32_t hmax;        // FASTA: the last line that is a header
    uint32_t lim;         // lines [0, lim) are whole records
    uint32_t bad;         // a record failed its check (sk_text_records; folded into `decline` by the closing scan)
    uint32_t pad;
    sk_text_info info;
};

__device__ __forceinline__ uint32_t tx_nl_mask4(uint32_t x)
{
    // exact zero-byte test of x ^ "\n\n\n\n" (no borrow between bytes), then one bit per byte
    const uint32_t y = x ^ 0x0A0A0A0Au;
    const uint32_t t = ~(((y & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | y | 0x7F7F7F7Fu);
    return ((t >> 7) & 1u) | ((t >> 14) & 2u) | ((t >> 21) & 4u) | ((t >> 28) & 8u);
}

// newline mask of the 16-byte chunk `ch` of the text (bit b: byte 16 ch + b), bytes at or behind n masked off
__device__ __forceinline__ uint32_t tx_chunk_mask(const uint4 *__restrict__ text16, uint64_t ch, uint64_t n)
{
    const uint64_t at = ch * 16u;
    if (at >= n) return 0u;
    const uint4 v = text16[ch];                     // (an aligned 16-byte chunk never leaves the page of its first byte)
    uint32_t m = tx_nl_mask4(v.x) | (tx_nl_mask4(v.y) << 4) | (tx_nl_mask4(v.z) << 8) | (tx_nl_mask4(v.w) << 12);
    if (n - at < 16u) m &= (1u << (uint32_t)(n - at)) - 1u;
    return m;
}

// exclusive prefix of v over the workgroup's TX_THREADS threads (in thread order); *total = the sum
__device__ __forceinline__ uint32_t tx_block_excl(uint32_t v, uint32_t *lds /* 4 */, uint32_t *total)
{
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    uint32_t inc = v;
    for (uint32_t d = 1; d < 64u; d <<= 1) { const uint32_t o = (uint32_t)__shfl_up((int)inc, d); if (lane >= d) inc += o; }
    __syncthreads();                                // (lds may still be read from the call before)
    if (lane == 63u) lds[w] = inc;
    __syncthreads();
    uint32_t base = 0, tot = 0;
    for (uint32_t k = 0; k < TX_THREADS / 64u; k++) { const uint32_t s = lds[k]; if (k < w) base += s; tot += s; }
    *total = tot;
    return base + inc - v;
}

__global__ void __launch_bounds__(TX_THREADS) sk_text_mark(const uint4 *__restrict__ text16, uint64_t n, unsigned long long *__restrict__ tile_cnt)
{
    __shared__ uint32_t lds[4];
    const uint64_t ch0 = (uint64_t)blockIdx.x * (TX_TILE / 16u);
    uint32_t m[TX_LOADS], c = 0;
#pragma unroll
    for (uint32_t j = 0; j < TX_LOADS; j++) m[j] = tx_chunk_mask(text16, ch0 + j * TX_THREADS + threadIdx.x, n);
#pragma unroll
    for (uint32_t j = 0; j < TX_LOADS; j++) c += (uint32_t)__popc(m[j]);
    uint32_t total;
    (void)tx_block_excl(c, lds, &total);
    if (threadIdx.x == 0) tile_cnt[blockIdx.x] = total;
}

// One workgroup: a[0..cnt) becomes its own exclusive prefix and a[cnt] the total.  mode 1: the tile counts (cnt given); it also
// closes the first half (line count, "starts with a header character").  mode 2: the line blocks' {records << 32 | bytes}, whose
// number only the device knows; it also closes the parse (lim, consumed, the info block).
__global__ void __launch_bounds__(1024) sk_text_scan(unsigned long long *__restrict__ a, uint32_t cnt_in, int mode, tx_head *__restrict__ h,
                                                       const uint8_t *__restrict__ text, uint64_t n, const uint32_t *__restrict__ nl_pos,
                                                       const uint32_t *__restrict__ lineval, uint32_t line_cap, int is_eof)
{
    __shared__ unsigned long long wsum[16];
    __shared__ unsigned long long carry_s;
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    uint32_t cnt = cnt_in;
    if (mode == 2) {
        const uint32_t bad = h->bad;
        if (h->decline || bad) { if (bad && threadIdx.x == 0) h->decline = 1; return; }
        cnt = h->nlines / TX_LB + 1u;
    }
    if (threadIdx.x == 0) carry_s = 0;
    __syncthreads();
    for (uint32_t base = 0; base < cnt; base += 1024u) {
        const uint32_t i = base + threadIdx.x;
        const unsigned long long v = i < cnt ? a[i] : 0ull;
        unsigned long long inc = v;
        for (uint32_t d = 1; d < 64u; d <<= 1) {
            const unsigned long long o = (unsigned long long)__shfl_up((long long)inc, d);
            if (lane >= d) inc += o;
        }
        if (lane == 63u) wsum[w] = inc;
        __syncthreads();
        unsigned long long pre = carry_s, tot = 0;
        for (uint32_t k = 0; k < 16u; k++) { const unsigned long long s = wsum[k]; if (k < w) pre += s; tot += s; }
        if (i < cnt) a[i] = pre + inc - v;
        __syncthreads();
        if (threadIdx.x == 0) carry_s += tot;
        __syncthreads();
    }
    if (threadIdx.x == 0) a[cnt] = carry_s;
    __syncthreads();
    if (mode == 1 && threadIdx.x == 0) {
        const uint32_t nl = (uint32_t)carry_s;
        h->nl = nl;
        h->nlines = nl + (n && text[n - 1] != '\n' ? 1u : 0u);
        // a piece starts with a header character, or is none of ours (FASTQ4 is told from FASTA in sk_text_records, once the third line's
        // start is known); more lines than the scratch was sized for -- under two bytes a line on average -- are left to the host as well
        const uint8_t c0 = n ? text[0] : 0;
        h->form = c0 == '>' || c0 == '@' ? SK_TEXT_FASTA : 0u;
        if (!h->form || nl + 2u > line_cap) h->decline = 1;
    }
    if (mode == 2) {
        // the exclusive prefix at line `lim`: its block's, plus the values of the block's lines before it
        const uint32_t T = h->nlines, nl = h->nl;
        uint32_t lim;
        if (h->form == SK_TEXT_FASTQ4) lim = is_eof ? T : (nl & ~3u);
        else lim = is_eof ? T : h->hmax;
        const uint32_t b = lim / TX_LB;
        unsigned long long part = 0;
        for (uint32_t i = b * TX_LB + threadIdx.x; i < lim; i += 1024u) { const uint32_t v = lineval[i]; part += ((unsigned long long)(v >> 31) << 32) | (v & ~TX_HDR); }
        for (uint32_t d = 32; d; d >>= 1) part += (unsigned long long)__shfl_down((long long)part, d);
        __syncthreads();
        if (lane == 0) wsum[w] = part;
        __syncthreads();
        if (threadIdx.x == 0) {
            unsigned long long p = a[b];
            for (uint32_t k = 0; k < 16u; k++) p += wsum[k];
            const uint32_t body = (uint32_t)p, nrec = (uint32_t)(p >> 32);
            h->lim = lim;
            h->info.status = SK_TEXT_OK;
            h->info.form = h->form;
            h->info.consumed = lim == T ? n : (lim ? (uint64_t)nl_pos[lim - 1] + 1u : 0u);
            h->info.stream_bytes = nrec ? (uint64_t)body + 1u : 0u;
            h->info.nrecords = nrec;
            h->info.bases = nrec ? (uint64_t)body - (nrec - 1u) : 0u;
        }
    }
}

__global__ void __launch_bounds__(TX_THREADS) sk_text_lines(const uint4 *__restrict__ text16, uint64_t n, const unsigned long long *__restrict__ tile_base,
                                                              uint32_t *__restrict__ nl_pos, uint32_t line_cap, tx_head *__restrict__ h)
{
    __shared__ uint32_t lds[4];
    if (h->decline) return;
    const uint64_t ch0 = (uint64_t)blockIdx.x * (TX_TILE / 16u);
    uint32_t rank = (uint32_t)tile_base[blockIdx.x];
    uint32_t m[TX_LOADS];
#pragma unroll
    for (uint32_t j = 0; j < TX_LOADS; j++) m[j] = tx_chunk_mask(text16, ch0 + j * TX_THREADS + threadIdx.x, n);
#pragma unroll
    for (uint32_t j = 0; j < TX_LOADS; j++) {
        uint32_t total, mm = m[j];
        uint32_t r = rank + tx_block_excl((uint32_t)__popc(mm), lds, &total);
        const uint32_t at = (uint32_t)((ch0 + j * TX_THREADS + threadIdx.x) * 16u);
        while (mm) {
            const uint32_t b = (uint32_t)__builtin_ctz(mm);
            mm &= mm - 1u;
            if (r < line_cap) nl_pos[r] = at + b;
            r++;
        }
        rank += total;
    }
}

struct tx_line { uint32_t start, len; uint8_t first, last; };
__device__ __forceinline__ tx_line tx_get_line(const uint8_t *__restrict__ text, uint64_t n, const uint32_t *__restrict__ nl_pos, uint32_t nl, uint32_t i)
{
    tx_line L;
    L.start = i ? nl_pos[i - 1] + 1u : 0u;
    const uint32_t end = i < nl ? nl_pos[i] : (uint32_t)n;
    L.len = end - L.start;
    L.first = L.len ? text[L.start] : 0;
    L.last = L.len ? text[end - 1u] : 0;
    return L;
}
__device__ __forceinline__ bool tx_is_head(uint8_t c) { return c == '>' || c == '@'; }
// the CR rule for a line that is a record's whole sequence or quality (src/kseq.h:136)
__device__ __forceinline__ uint32_t tx_kept_single(const tx_line &L) { return L.len - (L.len > 1u && L.last == '\r' ? 1u : 0u); }

__device__ __forceinline__ uint32_t tx_form(const uint8_t *__restrict__ text, uint64_t n, const uint32_t *__restrict__ nl_pos, const tx_head *__restrict__ h)
{
    // FASTQ4: starts with '@' and the third line starts with '+' (the first line's workgroup writes the answer back while the others
    // still ask: either value read here leads to the same one)
    const uint32_t f = h->form;
    if (f && text[0] == '@' && h->nl >= 2u) {
        const uint64_t s2 = (uint64_t)nl_pos[1] + 1u;
        if (s2 < n && text[s2] == '+') return SK_TEXT_FASTQ4;
    }
    return f;
}

__global__ void __launch_bounds__(TX_THREADS) sk_text_records(const uint8_t *__restrict__ text, uint64_t n, const uint32_t *__restrict__ nl_pos,
                                                                tx_head *__restrict__ h, uint32_t *__restrict__ lineval,
                                                                unsigned long long *__restrict__ blksum, int is_eof)
{
    __shared__ unsigned long long wsum[4];
    __shared__ uint32_t wmax[4];
    if (h->decline) return;
    const uint32_t T = h->nlines, nl = h->nl;
    const uint32_t b0 = blockIdx.x * TX_LB;
    if (b0 > T) return;
    const uint32_t form = tx_form(text, n, nl_pos, h);
    const uint32_t i = b0 + threadIdx.x;
    uint32_t val = 0, hline = 0;
    bool bad = false;
    if (form == SK_TEXT_FASTQ4) {
        const uint32_t lim = is_eof ? T : (nl & ~3u);
        if (i == 0 && is_eof && (T & 3u)) bad = true;             // (a record cut by the end of the file: the host says what it is)
        if (i < lim) {
            const tx_line L = tx_get_line(text, n, nl_pos, nl, i);
            switch (i & 3u) {
            case 0: if (L.first != '@') bad = true; val = TX_HDR | (i ? 1u : 0u); break;
            case 1: if (!L.len || tx_is_head(L.first) || L.first == '+') bad = true; val = tx_kept_single(L); break;
            case 2: if (L.first != '+') bad = true; break;
            default: {
                const tx_line S = tx_get_line(text, n, nl_pos, nl, i - 2u);
                if (tx_kept_single(L) != tx_kept_single(S)) bad = true;
                break; }
            }
        }
    } else if (i < T) {
        const bool terminated = i < nl;
        const tx_line L = tx_get_line(text, n, nl_pos, nl, i);
        if (!L.len) val = 0;
        else if (tx_is_head(L.first)) {
            val = TX_HDR | (i ? 1u : 0u);
            hline = i;
            if (!terminated && is_eof) bad = true;                 // (a header cut by the end of the file)
        } else if (!terminated && !is_eof) val = 0;                // (the piece's cut line: behind the last header, never taken)
        else if (L.first == '+') bad = true;                       // (the reference reads quality from here)
        else {
            val = L.len;
            if (L.last == '\r') {
                if (L.len > 1u) val--;
                else if (!terminated || i == 0) bad = true;
                else {
                    // a line of one CR: dropped when the record already has sequence (the accumulated length then exceeds 1), which the
                    // line before shows when it is sequence itself; anything else is left to the host
                    const tx_line P = tx_get_line(text, n, nl_pos, nl, i - 1u);
                    if (P.len && !tx_is_head(P.first) && P.first != '+' && !(P.len == 1u && P.last == '\r')) val = 0;
                    else bad = true;
                }
            }
        }
    }
    if (i < T + 1u || i == 0) lineval[i] = val;
    if (bad) atomicOr(&h->bad, 1u);
    if (i == 0 && form != h->form) h->form = form;                // (every workgroup computed it from the same bytes)
    unsigned long long s = ((unsigned long long)(val >> 31) << 32) | (val & ~TX_HDR);
    uint32_t mx = hline;
    for (uint32_t d = 32; d; d >>= 1) {
        s += (unsigned long long)__shfl_down((long long)s, d);
        const uint32_t o = (uint32_t)__shfl_down((int)mx, d);
        mx = o > mx ? o : mx;
    }
    if ((threadIdx.x & 63u) == 0) { wsum[threadIdx.x >> 6] = s; wmax[threadIdx.x >> 6] = mx; }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long t = 0; uint32_t m = 0;
        for (uint32_t k = 0; k < 4u; k++) { t += wsum[k]; m = wmax[k] > m ? wmax[k] : m; }
        blksum[blockIdx.x] = t;
        if (m) atomicMax(&h->hmax, m);
    }
}

__global__ void __launch_bounds__(TX_THREADS) sk_text_emit(const uint8_t *__restrict__ text, uint64_t n, const uint32_t *__restrict__ nl_pos,
                                                             const tx_head *__restrict__ h, const uint32_t *__restrict__ lineval,
                                                             const unsigned long long *__restrict__ blk_base, uint8_t *__restrict__ out,
                                                             uint32_t *__restrict__ rec_start, uint64_t nrec_cap)
{
    __shared__ uint32_t lds[4];
    __shared__ uint32_t s_off[4][65];
    __shared__ uint32_t s_src[4][64];
    if (h->decline) return;
    const uint32_t lim = h->lim, b0 = blockIdx.x * TX_LB;
    const uint32_t nrec = (uint32_t)h->info.nrecords;
    if (!nrec) return;
    const uint32_t body = (uint32_t)h->info.stream_bytes - 1u;
    if (blockIdx.x == 0 && threadIdx.x == 0) out[body] = '\n';   // the last record's end
    if (b0 >= lim) return;
    const uint32_t i = b0 + threadIdx.x, lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const uint32_t val = i < lim ? lineval[i] : 0u;
    const uint32_t len = val & ~TX_HDR, isH = val >> 31;
    uint32_t tot_b, tot_h;
    const uint32_t off_l = tx_block_excl(len, lds, &tot_b);
    const uint32_t rec_l = tx_block_excl(isH, lds, &tot_h);
    const unsigned long long base = blk_base[blockIdx.x];
    uint32_t off = (uint32_t)base + off_l;
    if (i >= lim || off > body) off = body;
    uint32_t src = 0;
    if (i < lim && len) {
        const uint32_t start = i ? nl_pos[i - 1] + 1u : 0u;
        src = isH ? start - 1u : start;                          // (a header ends the record before it: the '\n' in front of it serves)
    }
    if (i < lim && isH && rec_start) {
        const uint64_t r = (uint64_t)(uint32_t)(base >> 32) + rec_l;
        if (r < nrec_cap) rec_start[r] = off + (i ? 1u : 0u);
    }
    s_off[w][lane] = off;
    s_src[w][lane] = src;
    uint32_t end = off + len;
    if (end > body) end = body;
    if (lane == 63u) s_off[w][64] = end;
    __syncthreads();
    const uint32_t A = s_off[w][0], B = s_off[w][64];
    for (uint32_t wd = (A >> 2) + lane; wd * 4u < B; wd += 64u) {
        const uint32_t o0 = wd * 4u;
        const uint32_t first = o0 < A ? A : o0;
        // the last line of the wave's 64 that starts at or before `first` (lines without bytes share their successor's offset and lose)
        uint32_t lo = 0, hi = 64;
        while (hi - lo > 1u) { const uint32_t mid = (lo + hi) >> 1; if (s_off[w][mid] <= first) lo = mid; else hi = mid; }
        uint32_t word = 0, have = 0;
        for (uint32_t k = 0; k < 4u; k++) {
            const uint32_t o = o0 + k;
            if (o < A || o >= B) continue;
            while (lo < 63u && s_off[w][lo + 1u] <= o) lo++;
            const uint32_t c = text[s_src[w][lo] + (o - s_off[w][lo])];
            word |= c << (8u * k);
            have |= 1u << k;
        }
        if (have == 15u) *(uint32_t *)(out + o0) = word;
        else for (uint32_t k = 0; k < 4u; k++) if (have >> k & 1u) out[o0 + k] = (uint8_t)(word >> (8u * k));
    }
}

// A batch filled from text is finished on the device: nrec and the stream's length are known only here.  (a) tile_first[t], for the
// ntiles + 2 entries the TALLY scan reads behind rec_start[nrec]: the first record starting at or after byte t << 15 -- one lane per
// tile, a lower-bound search of the starts (ascending, all different: an empty record's start is one byte before the next one's).
// (b) the starts go home: 16 bytes per lane into the batch's page-locked staging, from which the host derives every record's length.
// More records than there is room for (a piece the host treats as declined): nothing is written.
__global__ void __launch_bounds__(TX_THREADS) sk_text_batch_close(const tx_head *__restrict__ h, uint32_t *__restrict__ rec, uint32_t nrec_cap,
                                                                    uint4 *__restrict__ host_rec)
{
    if (h->decline) return;
    const uint64_t nrec64 = h->info.nrecords;
    if (!nrec64 || nrec64 > nrec_cap) return;
    const uint32_t nrec = (uint32_t)nrec64;
    const uint32_t ntiles = (uint32_t)((h->info.stream_bytes + 32767u) >> 15);
    const uint32_t gid = blockIdx.x * TX_THREADS + threadIdx.x, gsz = gridDim.x * TX_THREADS;
    for (uint32_t t = gid; t < ntiles + 2u; t += gsz) {
        const uint64_t edge = (uint64_t)t << 15;
        uint32_t lo = 0, hi = nrec;                               // the first r in [0, nrec] with rec[r] >= edge
        while (lo < hi) { const uint32_t mid = lo + ((hi - lo) >> 1); if (rec[mid] < edge) lo = mid + 1u; else hi = mid; }
        rec[nrec + t] = lo;
    }
    const uint4 *const rec16 = (const uint4 *)rec;                // (whole 16-byte groups: the last one may take in tile entries, for which both sides have room)
    for (uint32_t i = gid; i < (nrec + 3u) / 4u; i += gsz) host_rec[i] = rec16[i];
}

// ---- host side ---------------------------------------------------------------------------------------------------
// The scratch of a context: made when the context first parses, sized for the piece at hand (the list scan's pieces have one
// size; a piece that grew makes it grow once more), kept until sk_text_release or the end of the process.
// what one parse works in: a stream, the scratch of the passes, the head block and where it lands.  A context has one (tx_state), and so
// has every batch that is filled from text (tx_batch: two batches of one context are parsed side by side).
struct tx_work {
    hipStream_t  stream = NULL;
    uint64_t     cap = 0;             // text bytes the scratch serves
    uint32_t     line_cap = 0;
    unsigned long long *d_tiles = NULL;   // newline count per tile, then its prefix
    uint32_t    *d_nl = NULL;         // [line_cap] position of every '\n'
    uint32_t    *d_lineval = NULL;    // [line_cap]
    unsigned long long *d_blk = NULL; // per block of TX_LB lines {records << 32 | bytes}, then its prefix
    tx_head     *d_head = NULL;
    tx_head     *h_head = NULL;       // page-locked landing place
    hipEvent_t   ev0 = NULL, ev1 = NULL;  // around the passes of the last parse (sk_text_timing); NULL: not timed
};
struct tx_state : tx_work {
    int          device = 0;
    // sk_scan_text_pinned: the text as uploaded, two record-stream buffers taking turns; readers[b]: the contexts whose scans
    // of d_out[b] have not been waited for -- they are, before a parse writes that buffer again
    uint64_t     up_cap = 0;
    uint8_t     *d_text = NULL, *d_out[2] = {NULL, NULL};
    std::vector<sk_ctx *> readers[2];
    int          cur = 0;
    uint64_t     pieces = 0, declined = 0;
    int          opt = -1;            // sk_text_option: 0 off, 1 on, -1 not set (SK_DEVICE_PARSE decides)
};
static pthread_mutex_t tx_mu = PTHREAD_MUTEX_INITIALIZER;
static std::map<sk_ctx *, tx_state *> tx_states;

#define TX_HIP(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return sk_fail_(ctx, SK_E_HIP, "%s failed: %s", #call, hipGetErrorString(e_)); } while (0)

static void tx_free_scratch(tx_work *s)
{
    (void)hipFree(s->d_tiles); (void)hipFree(s->d_nl); (void)hipFree(s->d_lineval); (void)hipFree(s->d_blk);
    s->d_tiles = NULL; s->d_nl = NULL; s->d_lineval = NULL; s->d_blk = NULL; s->cap = 0;
}
static void tx_free_upload(tx_state *s)
{
    (void)hipFree(s->d_text); (void)hipFree(s->d_out[0]); (void)hipFree(s->d_out[1]);
    s->d_text = NULL; s->d_out[0] = s->d_out[1] = NULL; s->up_cap = 0;
}

static void tx_free_device(tx_state *s)
{
    if (s->stream && hipSetDevice(s->device) == hipSuccess) {
        (void)hipStreamSynchronize(s->stream);
        tx_free_scratch(s);
        tx_free_upload(s);
        (void)hipFree(s->d_head);
        (void)hipHostFree(s->h_head);
        (void)hipEventDestroy(s->ev0);
        (void)hipEventDestroy(s->ev1);
        (void)hipStreamDestroy(s->stream);
    }
    s->stream = NULL; s->d_head = NULL; s->h_head = NULL; s->ev0 = s->ev1 = NULL;
    s->readers[0].clear(); s->readers[1].clear();
}

// The context's entry, made under the lock when it is first asked for (an int and a few counters: sk_text_option costs no device
// resources); `device`: with its stream, events and head block, made by the context's one caller when it first parses.
static int tx_state_get(sk_ctx *ctx, tx_state **out, bool device)
{
    pthread_mutex_lock(&tx_mu);
    tx_state *&slot = tx_states[ctx];
    if (!slot && (slot = new (std::nothrow) tx_state()) != NULL) slot->opt = -1;
    tx_state *const s = slot;
    if (!s) tx_states.erase(ctx);
    pthread_mutex_unlock(&tx_mu);
    if (!s) return SK_E_NOMEM;
    *out = s;
    if (!device) return SK_OK;
    const int dev = sk_ctx_device_(ctx);
    if (s->stream && s->device != dev) tx_free_device(s);          // (a context made anew at the address of one that was never released)
    if (!s->stream) {
        TX_HIP(hipSetDevice(dev));
        s->device = dev;
        if (hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking) != hipSuccess || hipMalloc((void **)&s->d_head, sizeof(tx_head)) != hipSuccess ||
            hipEventCreate(&s->ev0) != hipSuccess || hipEventCreate(&s->ev1) != hipSuccess ||
            hipHostMalloc((void **)&s->h_head, sizeof(tx_head), hipHostMallocDefault) != hipSuccess) {
            if (s->ev0) (void)hipEventDestroy(s->ev0);
            if (s->ev1) (void)hipEventDestroy(s->ev1);
            (void)hipFree(s->d_head);
            if (s->stream) (void)hipStreamDestroy(s->stream);
            s->stream = NULL; s->d_head = NULL; s->ev0 = s->ev1 = NULL;
            return sk_fail_(ctx, SK_E_HIP, "no stream or memory for the text parser");
        }
    }
    return SK_OK;
}

extern "C" void sk_text_release(sk_ctx *ctx)
{
    pthread_mutex_lock(&tx_mu);
    tx_state *s = NULL;
    std::map<sk_ctx *, tx_state *>::iterator it = tx_states.find(ctx);
    if (it != tx_states.end()) { s = it->second; tx_states.erase(it); }
    pthread_mutex_unlock(&tx_mu);
    if (!s) return;
    tx_free_device(s);
    delete s;
}

static int tx_scratch(sk_ctx *ctx, tx_work *s, uint64_t nbytes)
{
    if (nbytes <= s->cap) return SK_OK;
    TX_HIP(hipStreamSynchronize(s->stream));
    tx_free_scratch(s);
    const uint64_t cap = (nbytes + ((1u << 20) - 1u)) & ~(uint64_t)((1u << 20) - 1u);
    const uint64_t ntiles = cap / TX_TILE + 1u, line_cap = cap / 2u + 1024u;
    TX_HIP(hipMalloc((void **)&s->d_tiles, (ntiles + 1u) * 8u));
    TX_HIP(hipMalloc((void **)&s->d_nl, line_cap * 4u));
    TX_HIP(hipMalloc((void **)&s->d_lineval, line_cap * 4u));
    TX_HIP(hipMalloc((void **)&s->d_blk, (line_cap / TX_LB + 2u) * 8u));
    s->cap = cap;
    s->line_cap = (uint32_t)line_cap;
    return SK_OK;
}

// the passes, on s->stream (enqueued only: nothing here waits); the info lands in s->h_head (valid after the stream is synchronised)
static int tx_enqueue(sk_ctx *ctx, tx_work *s, const void *dev_text, uint64_t nbytes, int is_eof, void *dev_stream, uint32_t *dev_rec_start, uint64_t nrec_cap)
{
    const uint32_t ntiles = (uint32_t)((nbytes + TX_TILE - 1u) / TX_TILE);
    uint64_t max_lines = nbytes + 1u;
    if (max_lines > s->line_cap) max_lines = s->line_cap;
    const uint32_t nblk = (uint32_t)(max_lines / TX_LB + 1u);
    const uint8_t *text = (const uint8_t *)dev_text;
    if (s->ev0) TX_HIP(hipEventRecord(s->ev0, s->stream));
    TX_HIP(hipMemsetAsync(s->d_head, 0, sizeof(tx_head), s->stream));
    hipLaunchKernelGGL(sk_text_mark, dim3(ntiles), dim3(TX_THREADS), 0, s->stream, (const uint4 *)dev_text, nbytes, s->d_tiles);
    hipLaunchKernelGGL(sk_text_scan, dim3(1), dim3(1024), 0, s->stream, s->d_tiles, ntiles, 1, s->d_head, text, nbytes,
                       (const uint32_t *)s->d_nl, (const uint32_t *)s->d_lineval, s->line_cap, is_eof);
    hipLaunchKernelGGL(sk_text_lines, dim3(ntiles), dim3(TX_THREADS), 0, s->stream, (const uint4 *)dev_text, nbytes,
                       (const unsigned long long *)s->d_tiles, s->d_nl, s->line_cap, s->d_head);
    hipLaunchKernelGGL(sk_text_records, dim3(nblk), dim3(TX_THREADS), 0, s->stream, text, nbytes, (const uint32_t *)s->d_nl, s->d_head,
                       s->d_lineval, s->d_blk, is_eof);
    hipLaunchKernelGGL(sk_text_scan, dim3(1), dim3(1024), 0, s->stream, s->d_blk, 0u, 2, s->d_head, text, nbytes,
                       (const uint32_t *)s->d_nl, (const uint32_t *)s->d_lineval, s->line_cap, is_eof);
    hipLaunchKernelGGL(sk_text_emit, dim3(nblk), dim3(TX_THREADS), 0, s->stream, text, nbytes, (const uint32_t *)s->d_nl, (const tx_head *)s->d_head,
                       (const uint32_t *)s->d_lineval, (const unsigned long long *)s->d_blk, (uint8_t *)dev_stream, dev_rec_start, nrec_cap);
    TX_HIP(hipGetLastError());
    if (s->ev1) TX_HIP(hipEventRecord(s->ev1, s->stream));
    TX_HIP(hipMemcpyAsync(s->h_head, s->d_head, sizeof(tx_head), hipMemcpyDeviceToHost, s->stream));
    return SK_OK;
}

static void tx_result(const tx_work *s, sk_text_info *info)
{
    memset(info, 0, sizeof *info);
    if (s->h_head->decline) { info->status = SK_TEXT_DECLINED; info->form = s->h_head->form; }
    else *info = s->h_head->info;
}

static int tx_check(sk_ctx *ctx, const void *text, uint64_t nbytes, sk_text_info *info)
{
    if (!ctx || !info || (!text && nbytes)) return SK_E_ARG;
    if (nbytes > TX_MAX) return sk_fail_(ctx, SK_E_ARG, "a piece of text is at most 256 MiB");
    return SK_OK;
}

extern "C" int sk_text_parse_device(sk_ctx *ctx, const void *dev_text, uint64_t nbytes, int is_eof, void *dev_stream, uint32_t *dev_rec_start,
                                    uint64_t nrec_cap, sk_text_info *info)
{
    int rc = tx_check(ctx, dev_text, nbytes, info);
    if (rc) return rc;
    memset(info, 0, sizeof *info);
    if (!nbytes) { info->status = is_eof ? SK_TEXT_OK : SK_TEXT_DECLINED; info->form = SK_TEXT_FASTA; return SK_OK; }
    if (!dev_stream) return SK_E_ARG;
    if (((uintptr_t)dev_text & 15u) || ((uintptr_t)dev_stream & 3u)) return sk_fail_(ctx, SK_E_ARG, "device text must be 16-byte aligned, the stream 4-byte aligned");
    tx_state *s;
    if ((rc = tx_state_get(ctx, &s, true)) != SK_OK) return rc;
    TX_HIP(hipSetDevice(s->device));
    if ((rc = sk_sync(ctx)) != SK_OK) return rc;                  // (the text may have been put there by work on the context's stream)
    if ((rc = tx_scratch(ctx, s, nbytes)) != SK_OK) return rc;
    if ((rc = tx_enqueue(ctx, s, dev_text, nbytes, is_eof, dev_stream, dev_rec_start, nrec_cap)) != SK_OK) return rc;
    TX_HIP(hipStreamSynchronize(s->stream));
    tx_result(s, info);
    if (info->status == SK_TEXT_OK && dev_rec_start && info->nrecords > nrec_cap)
        return sk_fail_(ctx, SK_E_ARG, "%llu records, room for %llu record starts", (unsigned long long)info->nrecords, (unsigned long long)nrec_cap);
    return SK_OK;
}

// d_out[b] is about to be written: whoever may still read it is waited for.  A reader that is one of this call's contexts is
// synchronised; one that is not (the caller changed its set of contexts, and that one may be gone by now) is not touched -- the
// whole device is waited for instead.
static int tx_wait_readers(sk_ctx *ctx, tx_state *s, int b, sk_ctx *const *ctxs, uint32_t nctx)
{
    bool all = false;
    for (sk_ctx *r : s->readers[b]) {
        bool mine = false;
        for (uint32_t i = 0; i < nctx; i++) mine |= ctxs[i] == r;
        if (!mine) all = true;
        else { const int rc = sk_sync(r); if (rc != SK_OK) return rc; }
    }
    s->readers[b].clear();
    if (all) TX_HIP(hipDeviceSynchronize());
    return SK_OK;
}

// Upload, parse, scan.  Two record-stream buffers take turns, and only an accepted piece with records takes one.  The upload and the
// parse of piece n run on the parser's stream while the contexts still scan piece n - 1 out of the other buffer; then every context is
// waited for -- which frees that other buffer for piece n + 1 -- and its scan of piece n queued.  Whatever is left in a buffer's list
// of readers when it comes up again (a call with other contexts in between) is waited for before the parse writes it.  On return
// `pinned_text` has been read.
extern "C" int sk_scan_text_pinned_many(sk_ctx *const *ctxs, uint32_t nctx, const uint8_t *pinned_text, uint64_t nbytes, int is_eof, uint32_t col,
                                        sk_text_info *info)
{
    if (!ctxs || nctx < 1) return SK_E_ARG;
    sk_ctx *const ctx = ctxs[0];
    int rc = tx_check(ctx, pinned_text, nbytes, info);
    if (rc) return rc;
    for (uint32_t i = 0; i < nctx; i++) {
        if (!ctxs[i]) return SK_E_ARG;
        if (sk_ctx_device_(ctxs[i]) != sk_ctx_device_(ctx)) return sk_fail_(ctx, SK_E_ARG, "context %u is on another device: one upload serves one device", i);
        if (col >= sk_table_cols(ctxs[i])) return sk_fail_(ctx, SK_E_ARG, "context %u: column %u out of range", i, col);
    }
    memset(info, 0, sizeof *info);
    if (!nbytes) { info->status = is_eof ? SK_TEXT_OK : SK_TEXT_DECLINED; info->form = SK_TEXT_FASTA; return SK_OK; }
    tx_state *s;
    if ((rc = tx_state_get(ctx, &s, true)) != SK_OK) return rc;
    TX_HIP(hipSetDevice(s->device));
    if ((rc = tx_scratch(ctx, s, nbytes)) != SK_OK) return rc;
    if (nbytes > s->up_cap) {
        for (int b = 0; b < 2; b++) if ((rc = tx_wait_readers(ctx, s, b, ctxs, nctx)) != SK_OK) return rc;    // (a scan may still read the old buffers)
        TX_HIP(hipStreamSynchronize(s->stream));
        tx_free_upload(s);
        const uint64_t cap = s->cap;
        TX_HIP(hipMalloc((void **)&s->d_text, cap + 64u));
        TX_HIP(hipMalloc((void **)&s->d_out[0], cap + 4096u));
        TX_HIP(hipMalloc((void **)&s->d_out[1], cap + 4096u));
        s->up_cap = cap;
    }
    const int b = s->cur ^ 1;                                   // (taken for good only if the piece is accepted and has records)
    if ((rc = tx_wait_readers(ctx, s, b, ctxs, nctx)) != SK_OK) return rc;
    uint8_t *const d_out = s->d_out[b];
    TX_HIP(hipMemcpyAsync(s->d_text, pinned_text, nbytes, hipMemcpyHostToDevice, s->stream));
    if ((rc = tx_enqueue(ctx, s, s->d_text, nbytes, is_eof, d_out, NULL, 0)) != SK_OK) return rc;
    TX_HIP(hipStreamSynchronize(s->stream));
    tx_result(s, info);
    s->pieces++;
    if (info->status != SK_TEXT_OK) { s->declined++; return SK_OK; }
    if (!info->stream_bytes) return SK_OK;
    s->cur = b;
    for (uint32_t i = 0; i < nctx; i++) {
        // the scan of the piece before is waited for: this context no longer reads the other buffer
        std::vector<sk_ctx *> &other = s->readers[b ^ 1];
        if ((rc = sk_sync(ctxs[i])) != SK_OK) return rc;
        for (size_t k = 0; k < other.size(); ) { if (other[k] == ctxs[i]) other.erase(other.begin() + (long)k); else k++; }
        s->readers[b].push_back(ctxs[i]);                       // (before the launch: a scan that failed half-way may have queued work)
        if ((rc = sk_scan_device(ctxs[i], d_out, info->stream_bytes, col)) != SK_OK)
            return ctxs[i] == ctx ? rc : sk_fail_(ctx, rc, "context %u: %s", i, sk_last_error(ctxs[i]));
    }
    return SK_OK;
}

extern "C" int sk_scan_text_pinned(sk_ctx *ctx, const uint8_t *pinned_text, uint64_t nbytes, int is_eof, uint32_t col, sk_text_info *info)
{
    return sk_scan_text_pinned_many(&ctx, 1, pinned_text, nbytes, is_eof, col, info);
}

// ---- a strain_detect batch filled from text (sk_batch_fill_text / sk_batch_text_finish) ---------------------------------------
// Begin enqueues, on the batch's own stream: the upload of the text, the passes above writing the record stream and every record's
// start straight into the batch's buffers, sk_text_batch_close, and the copy home of the info; the batch's `ready` event follows
// them.  Nothing waits, so strain_detect's upload-ahead stays what it is.  Finish waits and says what the batch holds.  Every batch
// has its own scratch and head block: the two batches of a stream, and those of two streams (PE), are parsed side by side.
#define TX_BATCH_RECS (1u << 22)          // records in one piece at most (the host path's cap per chunk); more declines

struct tx_batch : tx_work {
    uint8_t *d_text = NULL;
    uint64_t text_cap = 0;
    uint32_t nrec_cap = 0;
    bool     pending = false;
};

static void tx_batch_free(void *p)        // (sk_batch_destroy: the device is set and the batch's stream has run dry)
{
    tx_batch *t = (tx_batch *)p;
    tx_free_scratch(t);
    (void)hipFree(t->d_text);
    (void)hipFree(t->d_head);
    if (t->h_head) (void)hipHostFree(t->h_head);
    delete t;
}

extern "C" int sk_batch_fill_text(sk_batch *b, const uint8_t *pinned_text, uint64_t nbytes, int is_eof)
{
    if (!b || !pinned_text || !nbytes || nbytes > TX_MAX) return SK_E_ARG;
    // a record takes two bytes of text at least (a header character and its '\n'), and the stream is shorter than the text
    const uint32_t nrec_cap = nbytes / 2u + 1u < TX_BATCH_RECS ? (uint32_t)(nbytes / 2u + 1u) : TX_BATCH_RECS;
    const uint32_t tiles_max = (uint32_t)((nbytes + 32767u) >> 15) + 2u;
    sk_batch_hook hk;
    int rc = sk_batch_hook_(b, nbytes, (uint64_t)nrec_cap + tiles_max + 4u, &hk);
    if (rc != SK_OK) return rc;
    sk_ctx *const ctx = hk.owner;
    sk_batch_contents_(b, 0, 0);                                  // (nothing to launch on until sk_batch_text_finish says so)
    tx_batch *t = (tx_batch *)*hk.text;
    if (!t) {
        if ((t = new (std::nothrow) tx_batch()) == NULL) return SK_E_NOMEM;
        t->stream = (hipStream_t)hk.stream;
        if (hipMalloc((void **)&t->d_head, sizeof(tx_head)) != hipSuccess || hipHostMalloc((void **)&t->h_head, sizeof(tx_head), hipHostMallocDefault) != hipSuccess) {
            tx_batch_free(t);
            return sk_fail_(ctx, SK_E_HIP, "no memory for the batch's text parser");
        }
        *hk.text = t;
        *hk.text_free = tx_batch_free;
    }
    t->pending = false;
    if ((rc = tx_scratch(ctx, t, nbytes)) != SK_OK) return rc;
    if (t->cap > t->text_cap) {
        (void)hipFree(t->d_text); t->d_text = NULL; t->text_cap = 0;
        TX_HIP(hipMalloc((void **)&t->d_text, t->cap + 64u));
        t->text_cap = t->cap;
    }
    uint4 *host_rec = NULL;
    TX_HIP(hipHostGetDevicePointer((void **)&host_rec, hk.h_rec, 0));
    TX_HIP(hipMemcpyAsync(t->d_text, pinned_text, nbytes, hipMemcpyHostToDevice, t->stream));
    if ((rc = tx_enqueue(ctx, t, t->d_text, nbytes, is_eof, hk.d_stream, hk.d_rec, nrec_cap)) != SK_OK) return rc;
    uint32_t work = nrec_cap / 4u + 1u > tiles_max ? nrec_cap / 4u + 1u : tiles_max, blocks = (work + TX_THREADS - 1u) / TX_THREADS;
    if (blocks > 1024u) blocks = 1024u;
    hipLaunchKernelGGL(sk_text_batch_close, dim3(blocks), dim3(TX_THREADS), 0, t->stream, (const tx_head *)t->d_head, hk.d_rec, nrec_cap, host_rec);
    TX_HIP(hipGetLastError());
    TX_HIP(hipEventRecord((hipEvent_t)hk.ready, t->stream));
    t->nrec_cap = nrec_cap;
    t->pending = true;
    return SK_OK;
}

extern "C" int sk_batch_text_finish(sk_batch *b, sk_text_info *info, const uint32_t **rec_start)
{
    if (!b || !info) return SK_E_ARG;
    sk_batch_hook hk;
    const int rc = sk_batch_hook_(b, 0, 0, &hk);                  // (waits for the batch's stream)
    if (rc != SK_OK) return rc;
    tx_batch *const t = (tx_batch *)*hk.text;
    if (!t || !t->pending) return sk_fail_(hk.owner, SK_E_STATE, "no text in flight for this batch");
    t->pending = false;
    tx_result(t, info);
    if (info->status == SK_TEXT_OK && info->nrecords > t->nrec_cap) {     // too many records for one batch: the host takes the piece
        const uint32_t form = info->form;
        memset(info, 0, sizeof *info);
        info->status = SK_TEXT_DECLINED; info->form = form;
    }
    if (info->status == SK_TEXT_OK && info->nrecords) sk_batch_contents_(b, info->stream_bytes, (uint32_t)info->nrecords);
    if (rec_start) *rec_start = hk.h_rec;
    return SK_OK;
}

extern "C" int sk_text_stats(sk_ctx *ctx, uint64_t *pieces, uint64_t *declined, int reset)
{
    if (!ctx) return SK_E_ARG;
    pthread_mutex_lock(&tx_mu);
    std::map<sk_ctx *, tx_state *>::iterator it = tx_states.find(ctx);
    tx_state *s = it != tx_states.end() ? it->second : NULL;
    if (pieces) *pieces = s ? s->pieces : 0;
    if (declined) *declined = s ? s->declined : 0;
    if (s && reset) s->pieces = s->declined = 0;
    pthread_mutex_unlock(&tx_mu);
    return SK_OK;
}

// The list scan's switch: 1 = whole plain-text items of skh_scan_file / skh_scan_list[_many] go this way, 0 = none does; a context
// that was never told follows SK_DEVICE_PARSE=1.
extern "C" int sk_text_option(sk_ctx *ctx, int on)
{
    if (!ctx) return SK_E_ARG;
    tx_state *s;
    const int rc = tx_state_get(ctx, &s, false);
    if (rc != SK_OK) return rc;
    s->opt = on ? 1 : 0;
    return SK_OK;
}

extern "C" int sk_text_enabled(sk_ctx *ctx)
{
    int opt = -1;
    pthread_mutex_lock(&tx_mu);
    std::map<sk_ctx *, tx_state *>::iterator it = tx_states.find(ctx);
    if (it != tx_states.end()) opt = it->second->opt;
    pthread_mutex_unlock(&tx_mu);
    if (opt >= 0) return opt;
    const char *e = getenv("SK_DEVICE_PARSE");
    return e && e[0] == '1';
}

// milliseconds the passes of the context's last parse kept the device busy (HIP events around them; the upload is not in it)
extern "C" int sk_text_timing(sk_ctx *ctx, double *last_ms)
{
    if (!ctx || !last_ms) return SK_E_ARG;
    pthread_mutex_lock(&tx_mu);
    std::map<sk_ctx *, tx_state *>::iterator it = tx_states.find(ctx);
    tx_state *s = it != tx_states.end() ? it->second : NULL;
    pthread_mutex_unlock(&tx_mu);
    float ms = 0.f;
    if (!s || !s->stream || hipSetDevice(s->device) != hipSuccess || hipStreamSynchronize(s->stream) != hipSuccess || hipEventElapsedTime(&ms, s->ev0, s->ev1) != hipSuccess)
        return sk_fail_(ctx, SK_E_STATE, "no parse to time");
    *last_ms = ms;
    return SK_OK;
}
