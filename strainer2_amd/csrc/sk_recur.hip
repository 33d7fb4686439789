// sk_recur.hip -- the recurrence engine: bit planes over the samples of a run, and the two tables that come out of them
// (include/strainer_kmer.h has the rule; strain_detect --coverage-recurrence / --recurrence-pairs, coverage_depth --recurrence), for
// gfx950.
//
// The state is generic: nmembers members of nbits[m] bits each, nsamples planes, plane[sample][word] of u64; a member's bits start
// at a word boundary, so no word holds bits of two members, and the padding bits behind nbits[m] in a member's last word are never
// set (every mark is checked against nbits[m] before it is made; the sweeps do not mask).  Three feeders set bits: sk_recur_mark_bits
// (bits from the host), sk_covacc_mark_target (sk_covacc.hip: the non-zero counters of a target) and sk_distinct_recurrence
// (sk_cover.hip: the slots of a hit list's key set).  Two kernels read the planes, neither writes them:
//   recur_hist   per member, how many bit positions are set in exactly m planes.  A lane owns one word column and walks the T planes
//                (word-major planes: a wave reads 512 contiguous bytes per plane) with a bit-sliced vertical counter: RECUR_CARRY =
//                13 u64 carry planes (2^13 > SK_RECUR_SAMPLES_MAX), a ripple add per incoming word that stops at the first empty
//                carry.  After the last plane only the positions with a non-zero counter are decoded, each into an LDS histogram of
//                T + 1 u32 bins; a workgroup adds its non-empty bins to HBM once (the discipline of covacc_finish_spectrum, for its
//                reason: one global atomic per row on one address is what cost sk_union_compact 587 us).
//   recur_gram   shared[i][j] = sum over words of popcount(P_i & P_j): a blocked "popcount GEMM".  A workgroup takes one member, one
//                64 x 64 block of sample pairs (blocks with bi <= bj only) and a chunk of words; it stages the two tiles of 64 planes x
//                RECUR_TW words in LDS, rows padded by one u64 so that lanes reading different planes at one word do not sit on one
//                bank, each of its 256 threads keeps a 4 x 4 block of pairs in registers over the chunk and adds its non-zero pairs
//                with i <= j to HBM.  The host mirrors the triangle.  Planes beyond T and words beyond the member read as zero.
//                (RECUR_TW is 32, not 64: two padded tiles of 64 words would be 66 560 bytes, above the 64 KB a workgroup may declare.)
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <new>
#include <vector>
#include "sk_internal.h"

#define RECUR_CARRY 13
#define RECUR_BINS  (SK_RECUR_SAMPLES_MAX + 1u)
#define RECUR_TW    32u                 // words of a tile row
#define RECUR_LD    (RECUR_TW + 1u)     // ... and its stride in LDS
#define RECUR_CHUNK 256u                // words of a member one gram workgroup takes

// bits[i] of `member` into plane `sample`: the host has checked every bit against the member's size
__global__ void recur_mark(const uint32_t *__restrict__ bits, uint64_t n, uint32_t nbits, unsigned long long *__restrict__ plane_member)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint32_t b = bits[i];
        if (b < nbits) atomicOr(plane_member + (b >> 6), 1ull << (b & 63u));
    }
}

__device__ __forceinline__ void recur_ripple(unsigned long long (&c)[RECUR_CARRY], unsigned long long x)
{
#pragma unroll
    for (int k = 0; k < RECUR_CARRY; k++) {
        const unsigned long long t = c[k] & x;
        c[k] ^= x;
        x = t;
        if (!x) break;                                         // (the carry has died: at 1 % of the bits set, after a level or two)
    }
}

// blockIdx.y = member; hist + member * (T + 1) holds its bins, bin 0 is the host's (nbits minus the rest)
__global__ void __launch_bounds__(64) recur_hist(const unsigned long long *__restrict__ planes, uint64_t words, uint32_t T,
                                                 const uint64_t *__restrict__ word_base, unsigned long long *__restrict__ hist)
{
    __shared__ uint32_t h[RECUR_BINS];
    const uint32_t m = blockIdx.y, nb = T + 1u;                // (T <= SK_RECUR_SAMPLES_MAX: the host has checked)
    const uint64_t w0 = word_base[m], nw = word_base[m + 1u] - w0;
    if ((uint64_t)blockIdx.x * 64u >= nw) return;              // (the whole workgroup)
    for (uint32_t b = threadIdx.x; b < nb; b += 64u) h[b] = 0u;
    __syncthreads();
    for (uint64_t w = (uint64_t)blockIdx.x * 64u + threadIdx.x; w < nw; w += (uint64_t)gridDim.x * 64u) {
        const unsigned long long *p = planes + w0 + w;
        unsigned long long c[RECUR_CARRY];
#pragma unroll
        for (int k = 0; k < RECUR_CARRY; k++) c[k] = 0ull;
        uint32_t s = 0;
        for (; s + 4u <= T; s += 4u) {                         // four loads in flight, then their adds
            const unsigned long long x0 = p[(uint64_t)s * words], x1 = p[(uint64_t)(s + 1u) * words],
                                     x2 = p[(uint64_t)(s + 2u) * words], x3 = p[(uint64_t)(s + 3u) * words];
            if (x0) recur_ripple(c, x0);
            if (x1) recur_ripple(c, x1);
            if (x2) recur_ripple(c, x2);
            if (x3) recur_ripple(c, x3);
        }
        for (; s < T; s++) {
            const unsigned long long x = p[(uint64_t)s * words];
            if (x) recur_ripple(c, x);
        }
        unsigned long long nz = 0ull;
#pragma unroll
        for (int k = 0; k < RECUR_CARRY; k++) nz |= c[k];
        while (nz) {
            const uint32_t b = (uint32_t)__builtin_ctzll(nz);
            nz &= nz - 1ull;
            uint32_t v = 0;
#pragma unroll
            for (int k = 0; k < RECUR_CARRY; k++) v |= (uint32_t)((c[k] >> b) & 1ull) << k;
            if (v < nb) atomicAdd(&h[v], 1u);                   // (always: a position is set in at most T planes)
        }
    }
    __syncthreads();
    for (uint32_t b = 1u + threadIdx.x; b < nb; b += 64u)
        if (h[b]) atomicAdd(hist + (size_t)m * nb + b, (unsigned long long)h[b]);
}

// blockIdx.x = chunk of words, blockIdx.y = block pair (bi <= bj, row after row of the upper triangle), blockIdx.z = member
__global__ void __launch_bounds__(256) recur_gram(const unsigned long long *__restrict__ planes, uint64_t words, uint32_t T,
                                                  const uint64_t *__restrict__ word_base, unsigned long long *__restrict__ pairs)
{
    __shared__ unsigned long long ta[64u * RECUR_LD];
    __shared__ unsigned long long tb[64u * RECUR_LD];
    const uint32_t m = blockIdx.z, nblk = (T + 63u) / 64u;
    const uint64_t w0 = word_base[m], nw = word_base[m + 1u] - w0;
    const uint64_t c0 = (uint64_t)blockIdx.x * RECUR_CHUNK;
    if (c0 >= nw) return;                                      // (the whole workgroup)
    uint32_t bi = 0, left = blockIdx.y;
    while (bi < nblk && left >= nblk - bi) { left -= nblk - bi; bi++; }
    if (bi >= nblk) return;                                    // (never: the grid has nblk (nblk + 1) / 2 rows)
    const uint32_t bj = bi + left;
    const bool diag = bi == bj;
    const unsigned long long *tbp = diag ? ta : tb;
    const uint64_t c1 = c0 + RECUR_CHUNK < nw ? c0 + RECUR_CHUNK : nw;
    const uint32_t ti = threadIdx.x >> 4, tj = threadIdx.x & 15u;   // pairs (ti + 16 x, tj + 16 y): neighbours read neighbouring rows
    uint32_t acc[4][4];
#pragma unroll
    for (int x = 0; x < 4; x++)
#pragma unroll
        for (int y = 0; y < 4; y++) acc[x][y] = 0u;
    for (uint64_t t0 = c0; t0 < c1; t0 += RECUR_TW) {
        for (uint32_t e = threadIdx.x; e < 64u * RECUR_TW; e += 256u) {
            const uint32_t row = e / RECUR_TW, col = e % RECUR_TW;
            const uint64_t w = t0 + col;
            const uint32_t si = bi * 64u + row, sj = bj * 64u + row;
            ta[row * RECUR_LD + col] = (si < T && w < c1) ? planes[(uint64_t)si * words + w0 + w] : 0ull;
            if (!diag) tb[row * RECUR_LD + col] = (sj < T && w < c1) ? planes[(uint64_t)sj * words + w0 + w] : 0ull;
        }
        __syncthreads();
        for (uint32_t col = 0; col < RECUR_TW; col++) {
            unsigned long long a[4], b[4];
#pragma unroll
            for (int x = 0; x < 4; x++) { a[x] = ta[(ti + 16u * x) * RECUR_LD + col]; b[x] = tbp[(tj + 16u * x) * RECUR_LD + col]; }
#pragma unroll
            for (int x = 0; x < 4; x++)
#pragma unroll
                for (int y = 0; y < 4; y++) acc[x][y] += (uint32_t)__popcll(a[x] & b[y]);
        }
        __syncthreads();
    }
    unsigned long long *out = pairs + (size_t)m * T * T;
#pragma unroll
    for (int x = 0; x < 4; x++)
#pragma unroll
        for (int y = 0; y < 4; y++) {
            const uint32_t i = bi * 64u + ti + 16u * x, j = bj * 64u + tj + 16u * y;
            if (acc[x][y] && i <= j && j < T) atomicAdd(out + (size_t)i * T + j, (unsigned long long)acc[x][y]);
        }
}

struct sk_recur {
    sk_ctx *ctx; int device;
    hipStream_t stream;
    uint32_t nm, ns;
    std::vector<uint32_t> nbits; std::vector<uint64_t> wbase;  // [nm], [nm + 1]: where a member's words begin in a plane
    uint64_t words; uint64_t max_words;
    unsigned long long *d_planes; uint64_t *d_wbase;
    void *d_bits; size_t bits_cap;
    void *d_out; size_t out_cap;
    bool timed; hipEvent_t ev[3]; double ms_hist, ms_gram;
};

#define RC_HIP(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return sk_fail_(r->ctx, SK_E_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); } while (0)

static int recur_room(sk_recur *r, void **p, size_t *cap, size_t need)
{
    if (need <= *cap) return SK_OK;
    if (*p) { RC_HIP(hipStreamSynchronize(r->stream)); (void)hipFree(*p); *p = NULL; *cap = 0; }
    const size_t want = need + need / 4 + 4096;
    RC_HIP(hipMalloc(p, want));
    *cap = want;
    return SK_OK;
}

extern "C" void sk_recur_destroy(sk_recur *r)
{
    if (!r) return;
    (void)hipSetDevice(r->device);
    if (r->stream) (void)hipStreamSynchronize(r->stream);
    (void)hipFree(r->d_planes); (void)hipFree(r->d_wbase); (void)hipFree(r->d_bits); (void)hipFree(r->d_out);
    if (r->timed) for (int i = 0; i < 3; i++) (void)hipEventDestroy(r->ev[i]);
    if (r->stream) (void)hipStreamDestroy(r->stream);
    delete r;
}

static int recur_create_steps(sk_recur *r)
{
    const size_t bytes = (size_t)(r->words ? r->words : 1u) * r->ns * 8u;
    RC_HIP(hipSetDevice(r->device));
    RC_HIP(hipStreamCreateWithFlags(&r->stream, hipStreamNonBlocking));
    RC_HIP(hipMalloc((void **)&r->d_planes, bytes));
    RC_HIP(hipMalloc((void **)&r->d_wbase, (size_t)(r->nm + 1u) * 8u));
    RC_HIP(hipMemsetAsync(r->d_planes, 0, bytes, r->stream));
    RC_HIP(hipMemcpyAsync(r->d_wbase, r->wbase.data(), (size_t)(r->nm + 1u) * 8u, hipMemcpyHostToDevice, r->stream));
    RC_HIP(hipStreamSynchronize(r->stream));
    return SK_OK;
}

extern "C" int sk_recur_create(sk_ctx *ctx, uint32_t nmembers, const uint32_t *nbits, uint32_t nsamples, sk_recur **out)
{
    if (!ctx || !out || !nbits || nmembers < 1u || nmembers > SK_RECUR_MEMBERS_MAX) return SK_E_ARG;
    *out = NULL;
    if (nsamples < 1u || nsamples > SK_RECUR_SAMPLES_MAX) return sk_fail_(ctx, SK_E_ARG, "%u samples: from 1 to %u", nsamples, SK_RECUR_SAMPLES_MAX);
    sk_recur *r = new (std::nothrow) sk_recur();
    if (!r) return SK_E_NOMEM;
    r->ctx = ctx; r->device = sk_ctx_device_(ctx); r->nm = nmembers; r->ns = nsamples;
    r->nbits.assign(nbits, nbits + nmembers);
    r->wbase.resize((size_t)nmembers + 1u);
    for (uint32_t m = 0; m < nmembers; m++) {
        const uint64_t w = ((uint64_t)nbits[m] + 63u) / 64u;
        r->wbase[m] = r->words;
        r->words += w;
        if (w > r->max_words) r->max_words = w;
    }
    r->wbase[nmembers] = r->words;
    const int rc = recur_create_steps(r);
    if (rc != SK_OK) { sk_recur_destroy(r); return rc; }
    *out = r;
    return SK_OK;
}

extern "C" int sk_recur_mark_bits(sk_recur *r, uint32_t member, uint32_t sample, const uint32_t *bits, uint64_t n)
{
    if (!r || (n && !bits)) return SK_E_ARG;
    if (member >= r->nm) return sk_fail_(r->ctx, SK_E_ARG, "member %u: the planes have %u", member, r->nm);
    if (sample >= r->ns) return sk_fail_(r->ctx, SK_E_ARG, "sample %u: the planes have %u", sample, r->ns);
    for (uint64_t i = 0; i < n; i++)
        if (bits[i] >= r->nbits[member]) return sk_fail_(r->ctx, SK_E_ARG, "bit %u: member %u has %u", bits[i], member, r->nbits[member]);
    if (!n) return SK_OK;
    RC_HIP(hipSetDevice(r->device));
    const int rc = recur_room(r, &r->d_bits, &r->bits_cap, (size_t)n * 4u);
    if (rc != SK_OK) return rc;
    const uint64_t g = (n + 255u) / 256u;
    RC_HIP(hipMemcpyAsync(r->d_bits, bits, (size_t)n * 4u, hipMemcpyHostToDevice, r->stream));
    hipLaunchKernelGGL(recur_mark, dim3((unsigned)(g > 4096u ? 4096u : g)), dim3(256), 0, r->stream, (const uint32_t *)r->d_bits, n,
                       r->nbits[member], r->d_planes + (size_t)sample * r->words + r->wbase[member]);
    RC_HIP(hipGetLastError());
    RC_HIP(hipStreamSynchronize(r->stream));
    return SK_OK;
}

extern "C" int sk_recur_finish(sk_recur *r, uint64_t *hist, uint64_t *pairs)
{
    if (!r || !hist) return SK_E_ARG;
    if (pairs && r->ns > SK_RECUR_PAIRS_MAX) return sk_fail_(r->ctx, SK_E_ARG, "%u samples: the pair table takes at most %u", r->ns, SK_RECUR_PAIRS_MAX);
    const uint32_t T = r->ns, nb = T + 1u;
    const size_t nh = (size_t)r->nm * nb, np = pairs ? (size_t)r->nm * T * T : 0u;
    RC_HIP(hipSetDevice(r->device));
    const int rc = recur_room(r, &r->d_out, &r->out_cap, (nh + np) * 8u);
    if (rc != SK_OK) return rc;
    unsigned long long *d_hist = (unsigned long long *)r->d_out, *d_pairs = d_hist + nh;
    RC_HIP(hipMemsetAsync(r->d_out, 0, (nh + np) * 8u, r->stream));
    if (r->timed) (void)hipEventRecord(r->ev[0], r->stream);
    if (r->max_words) {
        const uint64_t g = (r->max_words + 63u) / 64u;
        hipLaunchKernelGGL(recur_hist, dim3((unsigned)(g > 1024u ? 1024u : g), r->nm), dim3(64), 0, r->stream,
                           (const unsigned long long *)r->d_planes, r->words, T, (const uint64_t *)r->d_wbase, d_hist);
        RC_HIP(hipGetLastError());
    }
    if (r->timed) (void)hipEventRecord(r->ev[1], r->stream);
    if (pairs && r->max_words) {
        const uint32_t nblk = (T + 63u) / 64u;
        const uint64_t g = (r->max_words + RECUR_CHUNK - 1u) / RECUR_CHUNK;     // (2^32 bits at most: 2^18 chunks)
        hipLaunchKernelGGL(recur_gram, dim3((unsigned)g, nblk * (nblk + 1u) / 2u, r->nm), dim3(256), 0, r->stream,
                           (const unsigned long long *)r->d_planes, r->words, T, (const uint64_t *)r->d_wbase, d_pairs);
        RC_HIP(hipGetLastError());
    }
    if (r->timed) (void)hipEventRecord(r->ev[2], r->stream);
    RC_HIP(hipMemcpyAsync(hist, d_hist, nh * 8u, hipMemcpyDeviceToHost, r->stream));
    if (np) RC_HIP(hipMemcpyAsync(pairs, d_pairs, np * 8u, hipMemcpyDeviceToHost, r->stream));
    RC_HIP(hipStreamSynchronize(r->stream));
    if (r->timed) {
        float a = 0.f, b = 0.f;
        if (hipEventElapsedTime(&a, r->ev[0], r->ev[1]) == hipSuccess) r->ms_hist += (double)a;
        if (hipEventElapsedTime(&b, r->ev[1], r->ev[2]) == hipSuccess) r->ms_gram += (double)b;
    }
    for (uint32_t m = 0; m < r->nm; m++) {
        uint64_t seen = 0;
        for (uint32_t b = 1; b < nb; b++) seen += hist[(size_t)m * nb + b];
        hist[(size_t)m * nb] = (uint64_t)r->nbits[m] - seen;
        if (!pairs) continue;
        uint64_t *p = pairs + (size_t)m * T * T;
        for (uint32_t i = 0; i < T; i++)
            for (uint32_t j = i + 1u; j < T; j++) p[(size_t)j * T + i] = p[(size_t)i * T + j];
    }
    return SK_OK;
}

extern "C" int sk_recur_view_(sk_recur *r, sk_recur_view *out)
{
    if (!r || !out) return SK_E_ARG;
    out->device = r->device; out->nmembers = r->nm; out->nsamples = r->ns; out->nbits = r->nbits.data();
    out->word_base = r->wbase.data(); out->d_word_base = r->d_wbase; out->d_planes = r->d_planes; out->words = r->words;
    return SK_OK;
}

extern "C" int sk_recur_timing_(sk_recur *r, int on, double *ms_hist, double *ms_gram)
{
    if (!r) return SK_E_ARG;
    if (on && !r->timed) {
        if (hipSetDevice(r->device) != hipSuccess) return SK_E_HIP;
        for (int i = 0; i < 3; i++)
            if (hipEventCreate(&r->ev[i]) != hipSuccess) { while (i--) (void)hipEventDestroy(r->ev[i]); return SK_E_HIP; }
        r->timed = true;
    }
    if (ms_hist) *ms_hist = r->ms_hist;
    if (ms_gram) *ms_gram = r->ms_gram;
    return SK_OK;
}
