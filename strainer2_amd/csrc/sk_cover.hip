// sk_cover.hip -- device side of the coverage/depth aggregation (the consumer of strain_detect's hit
// list: reference scripts/coverage_depth.py, step 4 of test/example.sh) for gfx950.
//
// Per metagenome the script counts the hit lines that pass its read filter ("depth") and how many
// DIFFERENT k-mers they name ("coverage").  Here a hit is a (sample, key) pair -- key = the k-mer packed
// to 62 bits, or a row number -- and one kernel does both counts: every sample owns a power-of-two
// segment of one open-addressed u64 set; a lane inserts its key with one atomicCAS (a fresh slot = one
// more distinct k-mer for that sample) and runs of lanes with the same sample add their line count with
// one atomic.  HBM-bound integer work: 12 B read per hit + one random 8-B probe.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <new>
#include <vector>
#include "sk_internal.h"

#define COV_EMPTY 0xFFFFFFFFFFFFFFFFull

__device__ __forceinline__ uint64_t cov_mix(uint64_t x)
{
    x ^= x >> 33; x *= 0xFF51AFD7ED558CCDull; x ^= x >> 33; x *= 0xC4CEB9FE1A85EC53ull; x ^= x >> 33;
    return x;
}

__global__ void cov_count(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ sample, uint64_t n,
                          const uint64_t *__restrict__ seg_base, const uint64_t *__restrict__ seg_mask,
                          unsigned long long *__restrict__ table, unsigned long long *__restrict__ uniq, unsigned long long *__restrict__ total)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u;
    const bool live = i < n;
    const uint32_t s = live ? sample[i] : 0xFFFFFFFFu;
    bool fresh = false;
    if (live) {
        const uint64_t k = keys[i], base = seg_base[s], mask = seg_mask[s];
        uint64_t slot = cov_mix(k) & mask;
        for (;;) {
            const unsigned long long old = atomicCAS(&table[base + slot], COV_EMPTY, (unsigned long long)k);
            if (old == COV_EMPTY) { fresh = true; break; }
            if (old == k) break;
            slot = (slot + 1) & mask;
        }
    }
    // runs of equal sample within the wave: one atomic per run and counter
    const uint32_t prev = (uint32_t)__shfl_up((int)s, 1);
    const bool first = (lane == 0u) | (s != prev);
    const unsigned long long fm = __ballot(first), lm = __ballot(live), um = __ballot(fresh);
    if (first & live) {
        const unsigned long long above = lane == 63u ? 0ull : fm & ~((2ull << lane) - 1ull);
        const uint32_t end = above ? (uint32_t)__builtin_ctzll(above) : 64u;
        const unsigned long long seg = (end == 64u ? ~0ull : ((1ull << end) - 1ull)) & ~((1ull << lane) - 1ull);
        atomicAdd(&total[s], (unsigned long long)__popcll(lm & seg));
        const uint32_t nu = (uint32_t)__popcll(um & seg);
        if (nu) atomicAdd(&uniq[s], (unsigned long long)nu);
    }
}

// "first sighting" counting, for hit lists whose k-mer text is not a fixed-length ACGT word: the script then
// keys its uniqueness test by the joined string <sample><k-mer>, globally, and credits the sample of the FIRST
// line that shows a string.  id[i] = number of line i's joined string (dense, < nids), in file order.
__global__ void cov_first_min(const uint32_t *__restrict__ id, uint64_t n, unsigned long long *__restrict__ first)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) atomicMin(&first[id[i]], (unsigned long long)i);
}
__global__ void cov_first_count(const uint32_t *__restrict__ id, const uint32_t *__restrict__ sample, uint64_t n,
                                const unsigned long long *__restrict__ first, unsigned long long *__restrict__ uniq,
                                unsigned long long *__restrict__ total)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    atomicAdd(&total[sample[i]], 1ull);
    if (first[id[i]] == (unsigned long long)i) atomicAdd(&uniq[sample[i]], 1ull);
}

extern "C" int sk_first_seen_count(sk_ctx *ctx, const uint32_t *id, const uint32_t *sample, uint64_t n, uint32_t nids, uint32_t nsamples,
                                   uint64_t *out_unique, uint64_t *out_total)
{
    if (!ctx || !out_unique || !out_total || (n && (!id || !sample))) return SK_E_ARG;
    if (nsamples == 0) return n ? SK_E_ARG : SK_OK;
    memset(out_unique, 0, (size_t)nsamples * 8);
    memset(out_total, 0, (size_t)nsamples * 8);
    if (!n) return SK_OK;
    for (uint64_t i = 0; i < n; i++)
        if (id[i] >= nids || sample[i] >= nsamples) return sk_fail_(ctx, SK_E_ARG, "id or sample out of range");
    int rc = SK_OK;
    void *d_id = NULL, *d_sample = NULL, *d_first = NULL, *d_out = NULL;
#define COV_HIP(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { rc = sk_fail_(ctx, SK_E_HIP, "%s failed: %s", #call, hipGetErrorString(e_)); goto out; } } while (0)
    COV_HIP(hipSetDevice(sk_ctx_device_(ctx)));
    COV_HIP(hipMalloc(&d_id, n * 4));
    COV_HIP(hipMalloc(&d_sample, n * 4));
    COV_HIP(hipMalloc(&d_first, (size_t)nids * 8));
    COV_HIP(hipMalloc(&d_out, (size_t)nsamples * 16));
    COV_HIP(hipMemcpy(d_id, id, n * 4, hipMemcpyHostToDevice));
    COV_HIP(hipMemcpy(d_sample, sample, n * 4, hipMemcpyHostToDevice));
    COV_HIP(hipMemset(d_first, 0xFF, (size_t)nids * 8));
    COV_HIP(hipMemset(d_out, 0, (size_t)nsamples * 16));
    hipLaunchKernelGGL(cov_first_min, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, (const uint32_t *)d_id, n, (unsigned long long *)d_first);
    hipLaunchKernelGGL(cov_first_count, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, (const uint32_t *)d_id, (const uint32_t *)d_sample, n,
                       (const unsigned long long *)d_first, (unsigned long long *)d_out, (unsigned long long *)d_out + nsamples);
    COV_HIP(hipGetLastError());
    COV_HIP(hipMemcpy(out_unique, d_out, (size_t)nsamples * 8, hipMemcpyDeviceToHost));
    COV_HIP(hipMemcpy(out_total, (uint64_t *)d_out + nsamples, (size_t)nsamples * 8, hipMemcpyDeviceToHost));
#undef COV_HIP
out:
    (void)hipFree(d_id); (void)hipFree(d_sample); (void)hipFree(d_first); (void)hipFree(d_out);
    return rc;
}

// Distinct and total number of keys per sample.  Keys must not be 0xFFFFFFFFFFFFFFFF.  Synchronous.
extern "C" int sk_distinct_count(sk_ctx *ctx, const uint64_t *keys, const uint32_t *sample, uint64_t n, uint32_t nsamples,
                                 uint64_t *out_unique, uint64_t *out_total)
{
    if (!ctx || !out_unique || !out_total || (n && (!keys || !sample))) return SK_E_ARG;
    if (nsamples == 0) return n ? SK_E_ARG : SK_OK;
    memset(out_unique, 0, (size_t)nsamples * 8);
    memset(out_total, 0, (size_t)nsamples * 8);
    if (!n) return SK_OK;
    // segment sizes: next power of two >= 2 * (keys of that sample)
    std::vector<uint64_t> cnt(nsamples, 0), base(nsamples), mask(nsamples);
    for (uint64_t i = 0; i < n; i++) {
        if (sample[i] >= nsamples) return sk_fail_(ctx, SK_E_ARG, "sample %u out of range", sample[i]);
        if (keys[i] == COV_EMPTY) return sk_fail_(ctx, SK_E_ARG, "reserved key value");
        cnt[sample[i]]++;
    }
    uint64_t slots = 0;
    for (uint32_t s = 0; s < nsamples; s++) {
        uint64_t c = 2;
        while (c < 2 * cnt[s]) c <<= 1;
        base[s] = slots; mask[s] = c - 1; slots += c;
    }
    int rc = SK_OK;
    void *d_keys = NULL, *d_sample = NULL, *d_seg = NULL, *d_table = NULL, *d_out = NULL;
#define COV_HIP(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { rc = sk_fail_(ctx, SK_E_HIP, "%s failed: %s", #call, hipGetErrorString(e_)); goto out; } } while (0)
    COV_HIP(hipSetDevice(sk_ctx_device_(ctx)));
    COV_HIP(hipMalloc(&d_keys, n * 8));
    COV_HIP(hipMalloc(&d_sample, n * 4));
    COV_HIP(hipMalloc(&d_seg, (size_t)nsamples * 16));
    COV_HIP(hipMalloc(&d_table, slots * 8));
    COV_HIP(hipMalloc(&d_out, (size_t)nsamples * 16));
    COV_HIP(hipMemcpy(d_keys, keys, n * 8, hipMemcpyHostToDevice));
    COV_HIP(hipMemcpy(d_sample, sample, n * 4, hipMemcpyHostToDevice));
    COV_HIP(hipMemcpy(d_seg, base.data(), (size_t)nsamples * 8, hipMemcpyHostToDevice));
    COV_HIP(hipMemcpy((uint64_t *)d_seg + nsamples, mask.data(), (size_t)nsamples * 8, hipMemcpyHostToDevice));
    COV_HIP(hipMemset(d_table, 0xFF, slots * 8));
    COV_HIP(hipMemset(d_out, 0, (size_t)nsamples * 16));
    hipLaunchKernelGGL(cov_count, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, (const uint64_t *)d_keys, (const uint32_t *)d_sample, n,
                       (const uint64_t *)d_seg, (const uint64_t *)d_seg + nsamples, (unsigned long long *)d_table,
                       (unsigned long long *)d_out, (unsigned long long *)d_out + nsamples);
    COV_HIP(hipGetLastError());
    COV_HIP(hipMemcpy(out_unique, d_out, (size_t)nsamples * 8, hipMemcpyDeviceToHost));
    COV_HIP(hipMemcpy(out_total, (uint64_t *)d_out + nsamples, (size_t)nsamples * 8, hipMemcpyDeviceToHost));
#undef COV_HIP
out:
    (void)hipFree(d_keys); (void)hipFree(d_sample); (void)hipFree(d_seg); (void)hipFree(d_table); (void)hipFree(d_out);
    return rc;
}

// ---- the depth spectrum of a hit list (include/strainer_kmer.h has the rule; coverage_depth --spectrum) ----
// cov_count with a u32 count beside every slot of the set: the lane that finds or claims its key's slot adds 1 to that slot's count.
// The two numbers and the spectrum then come from one sweep of the counts.
__global__ void cov_count_depth(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ sample, uint64_t n, uint32_t nsamples,
                                const uint64_t *__restrict__ seg_base, const uint64_t *__restrict__ seg_mask,
                                unsigned long long *__restrict__ table, uint32_t *__restrict__ cnt)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t s = sample[i];
    if (s >= nsamples) return;                                // (never: the host has checked)
    const uint64_t k = keys[i], base = seg_base[s], mask = seg_mask[s];
    uint64_t slot = cov_mix(k) & mask;
    for (;;) {
        const unsigned long long old = atomicCAS(&table[base + slot], COV_EMPTY, (unsigned long long)k);
        if (old == COV_EMPTY || old == k) break;
        slot = (slot + 1) & mask;
    }
    atomicAdd(&cnt[base + slot], 1u);
}

// blockIdx.y = sample (and on by gridDim.y): the sample's segment of counts into LDS bins min(v, D + 1) - 1 -- plain LDS atomics, as
// in sk_covacc.hip's sweep and for its reason: at most half of a segment's slots are taken -- each workgroup adds its non-empty bins
// and its sums to HBM once.  out: [nsamples] pairs {unique, total}; spec: [nsamples x (D + 1)]; deep: [nsamples].
__global__ void __launch_bounds__(256) cov_spectrum(const uint32_t *__restrict__ cnt, const uint64_t *__restrict__ seg_base,
                                                    const uint64_t *__restrict__ seg_mask, uint32_t nsamples, uint32_t max_depth,
                                                    unsigned long long *__restrict__ out, unsigned long long *__restrict__ spec,
                                                    unsigned long long *__restrict__ deep)
{
    __shared__ uint32_t h_n[SK_COVACC_SPECTRUM_MAX + 1u];
    __shared__ unsigned long long h_sum[3];                   // unique, total, deep
    const uint32_t D = max_depth < SK_COVACC_SPECTRUM_MAX ? max_depth : SK_COVACC_SPECTRUM_MAX, ns = D + 1u;
    for (uint32_t s = blockIdx.y; s < nsamples; s += gridDim.y) {
        const uint64_t nslot = seg_mask[s] + 1u;
        if ((uint64_t)blockIdx.x * 256u >= nslot) continue;   // (the whole workgroup)
        const uint32_t *c = cnt + seg_base[s];
        for (uint32_t b = threadIdx.x; b < ns; b += 256u) h_n[b] = 0u;
        if (threadIdx.x < 3u) h_sum[threadIdx.x] = 0ull;
        __syncthreads();
        unsigned long long t = 0, dp = 0;
        uint32_t u = 0;
        for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < nslot; i += (uint64_t)gridDim.x * 256u) {
            const uint32_t v = c[i];
            if (!v) continue;
            u++; t += v;
            atomicAdd(&h_n[(v < ns ? v : ns) - 1u], 1u);
            if (v > D) dp += v;
        }
        if (u) { atomicAdd(&h_sum[0], (unsigned long long)u); atomicAdd(&h_sum[1], t); if (dp) atomicAdd(&h_sum[2], dp); }
        __syncthreads();
        if (threadIdx.x == 0u && h_sum[0]) {
            atomicAdd(out + 2ull * s, h_sum[0]);
            atomicAdd(out + 2ull * s + 1ull, h_sum[1]);
            if (h_sum[2]) atomicAdd(deep + s, h_sum[2]);
        }
        for (uint32_t b = threadIdx.x; b < ns; b += 256u)
            if (h_n[b]) atomicAdd(spec + (size_t)s * ns + b, (unsigned long long)h_n[b]);
        __syncthreads();
    }
}

// sk_distinct_count, and per sample how many of its keys came 1, 2, ..., max_depth and more than max_depth times.  Synchronous.
extern "C" int sk_distinct_spectrum(sk_ctx *ctx, const uint64_t *keys, const uint32_t *sample, uint64_t n, uint32_t nsamples, uint32_t max_depth,
                                    uint64_t *out_unique, uint64_t *out_total, uint64_t *spec, uint64_t *deep_total)
{
    if (!ctx || !out_unique || !out_total || !spec || !deep_total || (n && (!keys || !sample))) return SK_E_ARG;
    if (max_depth < 1u || max_depth > SK_COVACC_SPECTRUM_MAX) return SK_E_ARG;
    if (nsamples == 0) return n ? SK_E_ARG : SK_OK;
    const size_t nspec = (size_t)nsamples * (max_depth + 1u);
    memset(out_unique, 0, (size_t)nsamples * 8);
    memset(out_total, 0, (size_t)nsamples * 8);
    memset(deep_total, 0, (size_t)nsamples * 8);
    memset(spec, 0, nspec * 8);
    if (!n) return SK_OK;
    std::vector<uint64_t> cnt(nsamples, 0), base(nsamples), mask(nsamples);
    for (uint64_t i = 0; i < n; i++) {
        if (sample[i] >= nsamples) return sk_fail_(ctx, SK_E_ARG, "sample %u out of range", sample[i]);
        if (keys[i] == COV_EMPTY) return sk_fail_(ctx, SK_E_ARG, "reserved key value");
        cnt[sample[i]]++;
    }
    uint64_t slots = 0, max_seg = 0;
    for (uint32_t s = 0; s < nsamples; s++) {
        uint64_t c = 2;
        while (c < 2 * cnt[s]) c <<= 1;
        base[s] = slots; mask[s] = c - 1; slots += c;
        if (c > max_seg) max_seg = c;
    }
    int rc = SK_OK;
    void *d_keys = NULL, *d_sample = NULL, *d_seg = NULL, *d_table = NULL, *d_cnt = NULL, *d_out = NULL;
    std::vector<unsigned long long> h((size_t)nsamples * 3u + nspec);
#define COV_HIP(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { rc = sk_fail_(ctx, SK_E_HIP, "%s failed: %s", #call, hipGetErrorString(e_)); goto out; } } while (0)
    COV_HIP(hipSetDevice(sk_ctx_device_(ctx)));
    COV_HIP(hipMalloc(&d_keys, n * 8));
    COV_HIP(hipMalloc(&d_sample, n * 4));
    COV_HIP(hipMalloc(&d_seg, (size_t)nsamples * 16));
    COV_HIP(hipMalloc(&d_table, slots * 8));
    COV_HIP(hipMalloc(&d_cnt, slots * 4));
    COV_HIP(hipMalloc(&d_out, h.size() * 8));                 // [nsamples] pairs, [nsamples] deep sums, the bins
    COV_HIP(hipMemcpy(d_keys, keys, n * 8, hipMemcpyHostToDevice));
    COV_HIP(hipMemcpy(d_sample, sample, n * 4, hipMemcpyHostToDevice));
    COV_HIP(hipMemcpy(d_seg, base.data(), (size_t)nsamples * 8, hipMemcpyHostToDevice));
    COV_HIP(hipMemcpy((uint64_t *)d_seg + nsamples, mask.data(), (size_t)nsamples * 8, hipMemcpyHostToDevice));
    COV_HIP(hipMemset(d_table, 0xFF, slots * 8));
    COV_HIP(hipMemset(d_cnt, 0, slots * 4));
    COV_HIP(hipMemset(d_out, 0, h.size() * 8));
    hipLaunchKernelGGL(cov_count_depth, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, (const uint64_t *)d_keys, (const uint32_t *)d_sample, n,
                       nsamples, (const uint64_t *)d_seg, (const uint64_t *)d_seg + nsamples, (unsigned long long *)d_table, (uint32_t *)d_cnt);
    COV_HIP(hipGetLastError());
    {
        const uint64_t g = (max_seg + 255u) / 256u;
        hipLaunchKernelGGL(cov_spectrum, dim3((unsigned)(g > 256u ? 256u : g), nsamples > 4096u ? 4096u : nsamples), dim3(256), 0, 0,
                           (const uint32_t *)d_cnt, (const uint64_t *)d_seg, (const uint64_t *)d_seg + nsamples, nsamples, max_depth,
                           (unsigned long long *)d_out, (unsigned long long *)d_out + 3ull * nsamples, (unsigned long long *)d_out + 2ull * nsamples);
    }
    COV_HIP(hipGetLastError());
    COV_HIP(hipMemcpy(h.data(), d_out, h.size() * 8, hipMemcpyDeviceToHost));
    for (uint32_t s = 0; s < nsamples; s++) { out_unique[s] = h[2u * s]; out_total[s] = h[2u * s + 1u]; deep_total[s] = h[2ull * nsamples + s]; }
    for (size_t i = 0; i < nspec; i++) spec[i] = h[3ull * nsamples + i];
#undef COV_HIP
out:
    (void)hipFree(d_keys); (void)hipFree(d_sample); (void)hipFree(d_seg); (void)hipFree(d_table); (void)hipFree(d_cnt); (void)hipFree(d_out);
    return rc;
}

// ---- recurrence of a hit list (include/strainer_kmer.h has the rule; coverage_depth --recurrence) ----
// All samples share ONE open-addressed set here (cov_count gives every sample a segment of its own): a key's slot number is its bit,
// the same in every sample's plane.  cov_count's insert, then one atomicOr into the lane's sample's plane of the engine
// (sk_recur.hip), whose two sweeps then run over one member of nslots bits.
__global__ void cov_recur_insert(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ sample, uint64_t n, uint32_t nsamples,
                                 uint64_t mask, unsigned long long *__restrict__ table, unsigned long long *__restrict__ planes, uint64_t words)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint32_t s = sample[i];
        if (s >= nsamples) continue;                          // (never: the host has checked)
        const uint64_t k = keys[i];
        uint64_t slot = cov_mix(k) & mask;
        for (;;) {
            const unsigned long long old = atomicCAS(&table[slot], COV_EMPTY, (unsigned long long)k);
            if (old == COV_EMPTY || old == k) break;
            slot = (slot + 1) & mask;
        }
        atomicOr(planes + (uint64_t)s * words + (slot >> 6), 1ull << (slot & 63u));   // (slot <= mask < nbits = 64 * words)
    }
}

extern "C" int sk_distinct_recurrence(sk_ctx *ctx, const uint64_t *keys, const uint32_t *sample, uint64_t n, uint32_t nsamples,
                                      uint64_t *hist, uint64_t *pairs)
{
    if (!ctx || !hist || (n && (!keys || !sample))) return SK_E_ARG;
    if (nsamples < 1u || nsamples > SK_RECUR_SAMPLES_MAX) return sk_fail_(ctx, SK_E_ARG, "%u samples: from 1 to %u", nsamples, SK_RECUR_SAMPLES_MAX);
    if (pairs && nsamples > SK_RECUR_PAIRS_MAX) return sk_fail_(ctx, SK_E_ARG, "%u samples: the pair table takes at most %u", nsamples, SK_RECUR_PAIRS_MAX);
    if (n > (1ull << 30)) return sk_fail_(ctx, SK_E_ARG, "too many hits for one key set");
    for (uint64_t i = 0; i < n; i++) {
        if (sample[i] >= nsamples) return sk_fail_(ctx, SK_E_ARG, "sample %u out of range", sample[i]);
        if (keys[i] == COV_EMPTY) return sk_fail_(ctx, SK_E_ARG, "reserved key value");
    }
    memset(hist, 0, ((size_t)nsamples + 1u) * 8);
    if (pairs) memset(pairs, 0, (size_t)nsamples * nsamples * 8);
    if (!n) return SK_OK;
    uint64_t slots = 64;                                      // next power of two >= 2 n, whole words
    while (slots < 2 * n) slots <<= 1;
    const uint32_t nbits = (uint32_t)slots;
    sk_recur *r = NULL;
    sk_recur_view v;
    int rc = sk_recur_create(ctx, 1u, &nbits, nsamples, &r);
    if (rc != SK_OK) return rc;
    void *d_keys = NULL, *d_sample = NULL, *d_table = NULL;
#define COV_HIP(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { rc = sk_fail_(ctx, SK_E_HIP, "%s failed: %s", #call, hipGetErrorString(e_)); goto out; } } while (0)
    if ((rc = sk_recur_view_(r, &v)) != SK_OK) goto out;
    COV_HIP(hipSetDevice(sk_ctx_device_(ctx)));
    COV_HIP(hipMalloc(&d_keys, n * 8));
    COV_HIP(hipMalloc(&d_sample, n * 4));
    COV_HIP(hipMalloc(&d_table, slots * 8));
    COV_HIP(hipMemcpy(d_keys, keys, n * 8, hipMemcpyHostToDevice));
    COV_HIP(hipMemcpy(d_sample, sample, n * 4, hipMemcpyHostToDevice));
    COV_HIP(hipMemset(d_table, 0xFF, slots * 8));
    {
        const uint64_t g = (n + 255) / 256;
        hipLaunchKernelGGL(cov_recur_insert, dim3((unsigned)(g > 65536u ? 65536u : g)), dim3(256), 0, 0, (const uint64_t *)d_keys,
                           (const uint32_t *)d_sample, n, nsamples, slots - 1, (unsigned long long *)d_table, v.d_planes, v.words);
    }
    COV_HIP(hipGetLastError());
    COV_HIP(hipStreamSynchronize(0));
    rc = sk_recur_finish(r, hist, pairs);
    hist[0] = 0;                                              // (the engine's "never set" counts empty slots here)
#undef COV_HIP
out:
    (void)hipFree(d_keys); (void)hipFree(d_sample); (void)hipFree(d_table);
    sk_recur_destroy(r);
    return rc;
}

// ---- a hit list at several thresholds (include/strainer_kmer.h has the rule; coverage_depth --thresholds) ----
// cov_count_depth's insert with the highest class of a key's lines beside its slot instead of their number: a line's class is the
// number of thresholds its pair's total exceeds, a line of class 0 counts nowhere and is not inserted.  cov_thr_sweep then bins each
// sample's slots by class as cov_spectrum bins them by depth; the host takes the suffix sums.  The lines per sample and class are
// counted by the host in the pass that sizes the samples' segments, which has to classify every line anyway.
struct cov_thr_list { long long t[SK_COVACC_THRESHOLDS_MAX]; uint32_t n; };

__global__ void cov_thr_insert(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ sample, const uint32_t *__restrict__ total_hits,
                               uint64_t n, uint32_t nsamples, const uint64_t *__restrict__ seg_base, const uint64_t *__restrict__ seg_mask,
                               cov_thr_list th, unsigned long long *__restrict__ table, uint32_t *__restrict__ cls)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    const uint32_t nt = th.n < SK_COVACC_THRESHOLDS_MAX ? th.n : SK_COVACC_THRESHOLDS_MAX;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint32_t s = sample[i];
        if (s >= nsamples) continue;                          // (never: the host has checked)
        uint32_t c = 0;
        for (uint32_t q = 0; q < nt; q++) c += (long long)total_hits[i] > th.t[q] ? 1u : 0u;
        if (!c) continue;
        const uint64_t k = keys[i], base = seg_base[s], mask = seg_mask[s];
        uint64_t slot = cov_mix(k) & mask;
        for (;;) {                                            // (ends: the segment has twice the slots of the sample's lines of class >= 1)
            const unsigned long long old = atomicCAS(&table[base + slot], COV_EMPTY, (unsigned long long)k);
            if (old == COV_EMPTY || old == k) break;
            slot = (slot + 1) & mask;
        }
        atomicMax(&cls[base + slot], c);
    }
}

// blockIdx.y = sample (and on by gridDim.y): out[s * (MAX + 1) + c] = the sample's keys whose highest class is c
__global__ void __launch_bounds__(256) cov_thr_sweep(const uint32_t *__restrict__ cls, const uint64_t *__restrict__ seg_base,
                                                     const uint64_t *__restrict__ seg_mask, uint32_t nsamples, unsigned long long *__restrict__ out)
{
    __shared__ uint32_t h_n[SK_COVACC_THRESHOLDS_MAX + 1u];
    for (uint32_t s = blockIdx.y; s < nsamples; s += gridDim.y) {
        const uint64_t nslot = seg_mask[s] + 1u;
        if ((uint64_t)blockIdx.x * 256u >= nslot) continue;   // (the whole workgroup)
        const uint32_t *c = cls + seg_base[s];
        if (threadIdx.x <= SK_COVACC_THRESHOLDS_MAX) h_n[threadIdx.x] = 0u;
        __syncthreads();
        for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < nslot; i += (uint64_t)gridDim.x * 256u) {
            const uint32_t v = c[i];
            if (v && v <= SK_COVACC_THRESHOLDS_MAX) atomicAdd(&h_n[v], 1u);      // (at most half of the slots are taken)
        }
        __syncthreads();
        if (threadIdx.x <= SK_COVACC_THRESHOLDS_MAX && h_n[threadIdx.x])
            atomicAdd(out + (size_t)s * (SK_COVACC_THRESHOLDS_MAX + 1u) + threadIdx.x, (unsigned long long)h_n[threadIdx.x]);
        __syncthreads();
    }
}

extern "C" int sk_distinct_thresholds(sk_ctx *ctx, const uint64_t *keys, const uint32_t *sample, const uint32_t *total_hits, uint64_t n,
                                      uint32_t nsamples, const int64_t *t, uint32_t nt, uint64_t *out_unique, uint64_t *out_total)
{
    const uint32_t NC = SK_COVACC_THRESHOLDS_MAX + 1u;
    if (!ctx || !out_unique || !out_total || !t || nt < 1u || nt > SK_COVACC_THRESHOLDS_MAX || (n && (!keys || !sample || !total_hits))) return SK_E_ARG;
    for (uint32_t q = 0; q < nt; q++)
        if (t[q] < 0 || t[q] > 0x7FFFFFFEll || (q && t[q] <= t[q - 1])) return SK_E_ARG;
    if (nsamples == 0) return n ? SK_E_ARG : SK_OK;
    memset(out_unique, 0, (size_t)nsamples * nt * 8);
    memset(out_total, 0, (size_t)nsamples * nt * 8);
    if (!n) return SK_OK;
    cov_thr_list th;
    memset(&th, 0, sizeof th);
    for (uint32_t q = 0; q < nt; q++) th.t[q] = (long long)t[q];
    th.n = nt;
    std::vector<uint64_t> lines((size_t)nsamples * NC, 0), cnt(nsamples, 0), base(nsamples), mask(nsamples);
    for (uint64_t i = 0; i < n; i++) {
        if (sample[i] >= nsamples) return sk_fail_(ctx, SK_E_ARG, "sample %u out of range", sample[i]);
        if (keys[i] == COV_EMPTY) return sk_fail_(ctx, SK_E_ARG, "reserved key value");
        uint32_t c = 0;
        for (uint32_t q = 0; q < nt; q++) c += (long long)total_hits[i] > th.t[q] ? 1u : 0u;
        lines[(size_t)sample[i] * NC + c]++;
        if (c) cnt[sample[i]]++;
    }
    uint64_t slots = 0, max_seg = 0;
    for (uint32_t s = 0; s < nsamples; s++) {
        uint64_t c = 2;
        while (c < 2 * cnt[s]) c <<= 1;
        base[s] = slots; mask[s] = c - 1; slots += c;
        if (c > max_seg) max_seg = c;
    }
    int rc = SK_OK;
    void *d_keys = NULL, *d_sample = NULL, *d_tot = NULL, *d_seg = NULL, *d_table = NULL, *d_cls = NULL, *d_out = NULL;
    std::vector<unsigned long long> h((size_t)nsamples * NC);
#define COV_HIP(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { rc = sk_fail_(ctx, SK_E_HIP, "%s failed: %s", #call, hipGetErrorString(e_)); goto out; } } while (0)
    COV_HIP(hipSetDevice(sk_ctx_device_(ctx)));
    COV_HIP(hipMalloc(&d_keys, n * 8));
    COV_HIP(hipMalloc(&d_sample, n * 4));
    COV_HIP(hipMalloc(&d_tot, n * 4));
    COV_HIP(hipMalloc(&d_seg, (size_t)nsamples * 16));
    COV_HIP(hipMalloc(&d_table, slots * 8));
    COV_HIP(hipMalloc(&d_cls, slots * 4));
    COV_HIP(hipMalloc(&d_out, h.size() * 8));
    COV_HIP(hipMemcpy(d_keys, keys, n * 8, hipMemcpyHostToDevice));
    COV_HIP(hipMemcpy(d_sample, sample, n * 4, hipMemcpyHostToDevice));
    COV_HIP(hipMemcpy(d_tot, total_hits, n * 4, hipMemcpyHostToDevice));
    COV_HIP(hipMemcpy(d_seg, base.data(), (size_t)nsamples * 8, hipMemcpyHostToDevice));
    COV_HIP(hipMemcpy((uint64_t *)d_seg + nsamples, mask.data(), (size_t)nsamples * 8, hipMemcpyHostToDevice));
    COV_HIP(hipMemset(d_table, 0xFF, slots * 8));
    COV_HIP(hipMemset(d_cls, 0, slots * 4));
    COV_HIP(hipMemset(d_out, 0, h.size() * 8));
    {
        const uint64_t g = (n + 255) / 256, gs = (max_seg + 255u) / 256u;
        hipLaunchKernelGGL(cov_thr_insert, dim3((unsigned)(g > 65536u ? 65536u : g)), dim3(256), 0, 0, (const uint64_t *)d_keys,
                           (const uint32_t *)d_sample, (const uint32_t *)d_tot, n, nsamples, (const uint64_t *)d_seg,
                           (const uint64_t *)d_seg + nsamples, th, (unsigned long long *)d_table, (uint32_t *)d_cls);
        COV_HIP(hipGetLastError());
        hipLaunchKernelGGL(cov_thr_sweep, dim3((unsigned)(gs > 256u ? 256u : gs), nsamples > 4096u ? 4096u : nsamples), dim3(256), 0, 0,
                           (const uint32_t *)d_cls, (const uint64_t *)d_seg, (const uint64_t *)d_seg + nsamples, nsamples,
                           (unsigned long long *)d_out);
    }
    COV_HIP(hipGetLastError());
    COV_HIP(hipMemcpy(h.data(), d_out, h.size() * 8, hipMemcpyDeviceToHost));
    for (uint32_t s = 0; s < nsamples; s++) {                 // class c counts for the thresholds 0 .. c - 1: suffix sums
        uint64_t u = 0, l = 0;
        for (uint32_t q = nt; q-- > 0u; ) {
            u += h[(size_t)s * NC + q + 1u]; l += lines[(size_t)s * NC + q + 1u];
            out_unique[(size_t)s * nt + q] = u; out_total[(size_t)s * nt + q] = l;
        }
    }
#undef COV_HIP
out:
    (void)hipFree(d_keys); (void)hipFree(d_sample); (void)hipFree(d_tot); (void)hipFree(d_seg); (void)hipFree(d_table); (void)hipFree(d_cls);
    (void)hipFree(d_out);
    return rc;
}

// ---- a hit list by scrub class (include/strainer_kmer.h has the rule; coverage_depth --scrub-sweep) ----
// cov_thr_insert with every line's class handed in instead of worked out from its pair's total: the lines of a (sample, key) pair carry
// one class, which lands beside the pair's slot, and cov_thr_sweep bins each sample's slots by class; the host counts the lines per
// sample and class in the pass that sizes the segments and takes the suffix sums.
static_assert(SK_SCRUB_SWEEP_MAX == SK_COVACC_THRESHOLDS_MAX, "cov_thr_sweep's bins serve both lists");

__global__ void cov_cls_insert(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ sample, const uint8_t *__restrict__ kcls,
                               uint64_t n, uint32_t nsamples, uint32_t ncls, const uint64_t *__restrict__ seg_base,
                               const uint64_t *__restrict__ seg_mask, unsigned long long *__restrict__ table, uint32_t *__restrict__ cls)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint32_t s = sample[i], c = kcls[i];
        if (s >= nsamples || c < 1u || c > ncls) continue;    // (never: the host has checked)
        const uint64_t k = keys[i], base = seg_base[s], mask = seg_mask[s];
        uint64_t slot = cov_mix(k) & mask;
        for (;;) {                                            // (ends: the segment has twice the slots of the sample's lines)
            const unsigned long long old = atomicCAS(&table[base + slot], COV_EMPTY, (unsigned long long)k);
            if (old == COV_EMPTY || old == k) break;
            slot = (slot + 1) & mask;
        }
        atomicMax(&cls[base + slot], c);
    }
}

extern "C" int sk_distinct_classes(sk_ctx *ctx, const uint64_t *keys, const uint32_t *sample, const uint8_t *cls, uint64_t n, uint32_t nsamples,
                                   uint32_t ncls, uint64_t *out_unique, uint64_t *out_total)
{
    const uint32_t NC = SK_SCRUB_SWEEP_MAX + 1u;
    if (!ctx || !out_unique || !out_total || ncls < 1u || ncls > SK_SCRUB_SWEEP_MAX || (n && (!keys || !sample || !cls))) return SK_E_ARG;
    if (nsamples == 0) return n ? SK_E_ARG : SK_OK;
    memset(out_unique, 0, (size_t)nsamples * ncls * 8);
    memset(out_total, 0, (size_t)nsamples * ncls * 8);
    if (!n) return SK_OK;
    std::vector<uint64_t> lines((size_t)nsamples * NC, 0), cnt(nsamples, 0), base(nsamples), mask(nsamples);
    for (uint64_t i = 0; i < n; i++) {
        if (sample[i] >= nsamples) return sk_fail_(ctx, SK_E_ARG, "sample %u out of range", sample[i]);
        if (keys[i] == COV_EMPTY) return sk_fail_(ctx, SK_E_ARG, "reserved key value");
        if (cls[i] < 1u || cls[i] > ncls) return sk_fail_(ctx, SK_E_ARG, "class %u: 1 to %u", cls[i], ncls);
        lines[(size_t)sample[i] * NC + cls[i]]++;
        cnt[sample[i]]++;
    }
    uint64_t slots = 0, max_seg = 0;
    for (uint32_t s = 0; s < nsamples; s++) {
        uint64_t c = 2;
        while (c < 2 * cnt[s]) c <<= 1;
        base[s] = slots; mask[s] = c - 1; slots += c;
        if (c > max_seg) max_seg = c;
    }
    int rc = SK_OK;
    void *d_keys = NULL, *d_sample = NULL, *d_kcls = NULL, *d_seg = NULL, *d_table = NULL, *d_cls = NULL, *d_out = NULL;
    std::vector<unsigned long long> h((size_t)nsamples * NC);
#define COV_HIP(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { rc = sk_fail_(ctx, SK_E_HIP, "%s failed: %s", #call, hipGetErrorString(e_)); goto out; } } while (0)
    COV_HIP(hipSetDevice(sk_ctx_device_(ctx)));
    COV_HIP(hipMalloc(&d_keys, n * 8));
    COV_HIP(hipMalloc(&d_sample, n * 4));
    COV_HIP(hipMalloc(&d_kcls, n));
    COV_HIP(hipMalloc(&d_seg, (size_t)nsamples * 16));
    COV_HIP(hipMalloc(&d_table, slots * 8));
    COV_HIP(hipMalloc(&d_cls, slots * 4));
    COV_HIP(hipMalloc(&d_out, h.size() * 8));
    COV_HIP(hipMemcpy(d_keys, keys, n * 8, hipMemcpyHostToDevice));
    COV_HIP(hipMemcpy(d_sample, sample, n * 4, hipMemcpyHostToDevice));
    COV_HIP(hipMemcpy(d_kcls, cls, n, hipMemcpyHostToDevice));
    COV_HIP(hipMemcpy(d_seg, base.data(), (size_t)nsamples * 8, hipMemcpyHostToDevice));
    COV_HIP(hipMemcpy((uint64_t *)d_seg + nsamples, mask.data(), (size_t)nsamples * 8, hipMemcpyHostToDevice));
    COV_HIP(hipMemset(d_table, 0xFF, slots * 8));
    COV_HIP(hipMemset(d_cls, 0, slots * 4));
    COV_HIP(hipMemset(d_out, 0, h.size() * 8));
    {
        const uint64_t g = (n + 255) / 256, gs = (max_seg + 255u) / 256u;
        hipLaunchKernelGGL(cov_cls_insert, dim3((unsigned)(g > 65536u ? 65536u : g)), dim3(256), 0, 0, (const uint64_t *)d_keys,
                           (const uint32_t *)d_sample, (const uint8_t *)d_kcls, n, nsamples, ncls, (const uint64_t *)d_seg,
                           (const uint64_t *)d_seg + nsamples, (unsigned long long *)d_table, (uint32_t *)d_cls);
        COV_HIP(hipGetLastError());
        hipLaunchKernelGGL(cov_thr_sweep, dim3((unsigned)(gs > 256u ? 256u : gs), nsamples > 4096u ? 4096u : nsamples), dim3(256), 0, 0,
                           (const uint32_t *)d_cls, (const uint64_t *)d_seg, (const uint64_t *)d_seg + nsamples, nsamples,
                           (unsigned long long *)d_out);
    }
    COV_HIP(hipGetLastError());
    COV_HIP(hipMemcpy(h.data(), d_out, h.size() * 8, hipMemcpyDeviceToHost));
    for (uint32_t s = 0; s < nsamples; s++) {                 // class c counts for the fractions 0 .. c - 1: suffix sums
        uint64_t u = 0, l = 0;
        for (uint32_t q = ncls; q-- > 0u; ) {
            u += h[(size_t)s * NC + q + 1u]; l += lines[(size_t)s * NC + q + 1u];
            out_unique[(size_t)s * ncls + q] = u; out_total[(size_t)s * ncls + q] = l;
        }
    }
#undef COV_HIP
out:
    (void)hipFree(d_keys); (void)hipFree(d_sample); (void)hipFree(d_kcls); (void)hipFree(d_seg); (void)hipFree(d_table); (void)hipFree(d_cls);
    (void)hipFree(d_out);
    return rc;
}
