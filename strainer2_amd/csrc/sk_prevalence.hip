// sk_prevalence.hip -- the fold where a list item ends (kmer_scrub_count --prevalence; the rule is in include/strainer_kmer.h at
// sk_item_fold).  New: the reference adds every file of a list into one column (src/genome_compare.c:220-223) and keeps nothing
// per file.
//
// The counts are made by the COUNT scan as it is: while an item slot is set (sk_item_slot) its increments go into the slot's own
// scratch column and difference array instead of the column's.  What is here is the pass that takes a slot apart again.  The
// plain form, three launches on the context's stream: the difference array's block sums and their scan (the kernels sk_diff_flush
// uses), then ONE apply kernel of the shape of sk_diff_apply -- 256 threads, 16 consecutive entries each, the running prefix of
// the difference array in registers -- which per row takes v = prefix + scratch, adds v to the count column and (v >= min_count)
// to the prevalence column, writes zeros behind every non-zero entry it read, and counts the item's record: the two sums meet in a
// wave reduction, then in LDS, and a workgroup with anything to report adds them to HBM with one 64-bit atomic each.
// The fold of a UNION's slot (sk_union_item_fold: many strains over one pass, kmer_scrub_count -S --prevalence=SUFFIX) is further down.
#include <hip/hip_runtime.h>
#include <pthread.h>
#include <stdint.h>
#include <vector>
#include "sk_internal.h"

#define PV_PER_BLOCK 4096u                                          // 256 threads x 16 entries (SK_DIFF_PER_BLOCK: the block sums are per this many)

__global__ void __launch_bounds__(256) item_apply(uint32_t *__restrict__ diff, uint32_t n, const uint32_t *__restrict__ sums,
                                                  uint32_t *__restrict__ scratch, uint32_t *__restrict__ count, uint32_t *__restrict__ prev,
                                                  uint32_t nrows, uint32_t min_count, unsigned long long *__restrict__ record)
{
    __shared__ uint32_t part[256];
    __shared__ unsigned long long w_hits[4];
    __shared__ uint32_t w_present[4];
    const uint32_t base = blockIdx.x * PV_PER_BLOCK + threadIdx.x * 16u;
    uint32_t v[16], t = 0;
    for (uint32_t i = 0; i < 16u; i++) { v[i] = base + i < n ? diff[base + i] : 0u; t += v[i]; }
    part[threadIdx.x] = t;
    __syncthreads();
    for (uint32_t d = 1u; d < 256u; d <<= 1) {
        const uint32_t u = threadIdx.x >= d ? part[threadIdx.x - d] : 0u;
        __syncthreads();
        part[threadIdx.x] += u;
        __syncthreads();
    }
    uint32_t run = sums[blockIdx.x] + part[threadIdx.x] - t;
    uint32_t present = 0;
    unsigned long long hits = 0ull;
    for (uint32_t i = 0; i < 16u; i++) {
        run += v[i];
        if (base + i < nrows) {
            const uint32_t s = scratch[base + i], x = run + s;      // (mod 2^32, as the column's own adds are)
            if (x) count[base + i] += x;
            if (x >= min_count) { prev[base + i] += 1u; present++; }
            hits += x;
            if (s) scratch[base + i] = 0u;
        }
        if (base + i < n && v[i]) diff[base + i] = 0u;
    }
    for (int off = 32; off; off >>= 1) { present += __shfl_down(present, off, 64); hits += __shfl_down(hits, off, 64); }
    if ((threadIdx.x & 63u) == 0u) { w_present[threadIdx.x >> 6] = present; w_hits[threadIdx.x >> 6] = hits; }
    __syncthreads();
    if (threadIdx.x == 0u && record) {
        const unsigned long long p = (unsigned long long)w_present[0] + w_present[1] + w_present[2] + w_present[3];
        const unsigned long long h = w_hits[0] + w_hits[1] + w_hits[2] + w_hits[3];
        if (p) atomicAdd(record, p);
        if (h) atomicAdd(record + 1, h);
    }
}

// the folds' device time (SK_TIMING of the list walk; tools/prevalence_bench.py): an event pair around every fold while the clocks
// are on, added up when the caller asks -- off unless asked for, so a run without it makes no event
static pthread_mutex_t pv_mu = PTHREAD_MUTEX_INITIALIZER;
static bool pv_clocks = false;
static std::vector<hipEvent_t> pv_ev;
extern "C" int sk_item_fold_timing_(sk_ctx *ctx, int on, double *ms, uint64_t *folds)
{
    (void)ctx;
    pthread_mutex_lock(&pv_mu);
    double sum = 0.0;
    for (size_t i = 0; i + 1 < pv_ev.size(); i += 2) {
        float one = 0.f;
        if (hipEventSynchronize(pv_ev[i + 1]) == hipSuccess && hipEventElapsedTime(&one, pv_ev[i], pv_ev[i + 1]) == hipSuccess) sum += one;
        else (void)hipGetLastError();
    }
    if (ms) *ms = sum;
    if (folds) *folds = pv_ev.size() / 2;
    for (hipEvent_t e : pv_ev) (void)hipEventDestroy(e);
    pv_ev.clear();
    pv_clocks = on != 0;
    pthread_mutex_unlock(&pv_mu);
    return SK_OK;
}

// ---- the fold of an item slot of a UNION's context (sk_union_item_fold; kmer_scrub_count -S --prevalence=SUFFIX) ----
// The slot holds global rows, and the scan credits whichever row of a key it found: the slot row when a probe found the key, a
// member's own row when the window was verified against that member's text.  Two passes and a memset behind the block sums, whatever
// the number of members:
//   gather -- item_apply's shape (256 threads, 16 consecutive entries each, the running prefix in registers).  A row that is not its
//     key's slot row adds its value (prefix + scratch) to scratch[canon[g]] and zeroes its own scratch; a slot row adds its prefix to
//     its own scratch.  Both adds are atomic, and only slot rows are atomic targets: canon[w] == w, so no row both gives and takes
//     (the argument of sk_union_fold_canon).  Every difference entry read non-zero is zeroed.  Afterwards scratch[w] = V_w on slot
//     rows and 0 elsewhere.
//   apply -- ONE pass over the global rows, 256 consecutive rows per step so that a wave reads 64 neighbours: a row finds its member
//     in base[] (at most 33 values, in LDS), reads V at scratch[canon[g]] and updates the member's two columns (each (member, row) is
//     one global row: plain adds).  The records meet in a wave reduction where the wave lies in one member, otherwise per lane, in an
//     LDS table of 32 x 2 u64; the workgroup's non-zero cells go out with one 64-bit atomic each (sk_union_share_sweep's idiom).
//     A wave of rows the item did not touch skips the record part after one ballot (its rows are still looked up and read).
//   the scratch column is zeroed once every reader is done (a memset on the stream: non-slot rows are zero already, the slot rows
//     are not known without reading canon[] again, which costs what the memset's 4 bytes a row cost).
struct pv_union_args { uint32_t base[SK_UNION_MAX + 1]; uint32_t *count[SK_UNION_MAX]; uint32_t *prev[SK_UNION_MAX]; };

__global__ void __launch_bounds__(256) union_item_gather(uint32_t *__restrict__ diff, uint32_t n, const uint32_t *__restrict__ sums,
                                                         uint32_t *scratch, const uint32_t *__restrict__ canon, uint32_t nrows)
{
    __shared__ uint32_t part[256];
    const uint32_t base = blockIdx.x * PV_PER_BLOCK + threadIdx.x * 16u;
    uint32_t v[16], t = 0;
    for (uint32_t i = 0; i < 16u; i++) { v[i] = base + i < n ? diff[base + i] : 0u; t += v[i]; }
    part[threadIdx.x] = t;
    __syncthreads();
    for (uint32_t d = 1u; d < 256u; d <<= 1) {
        const uint32_t u = threadIdx.x >= d ? part[threadIdx.x - d] : 0u;
        __syncthreads();
        part[threadIdx.x] += u;
        __syncthreads();
    }
    uint32_t run = sums[blockIdx.x] + part[threadIdx.x] - t;
    for (uint32_t i = 0; i < 16u; i++) {
        run += v[i];
        const uint32_t g = base + i;
        if (g < nrows) {
            const uint32_t w = canon[g];
            if (w != g && w < nrows) {
                const uint32_t s = scratch[g], x = run + s;         // (mod 2^32, as the column's own adds are)
                if (x) atomicAdd(&scratch[w], x);
                if (s) scratch[g] = 0u;
            } else if (run) atomicAdd(&scratch[g], run);
        }
        if (g < n && v[i]) diff[g] = 0u;
    }
}

__global__ void __launch_bounds__(256) union_item_apply(const uint32_t *scratch, const uint32_t *__restrict__ canon, uint32_t nrows,
                                                        uint32_t members, uint32_t member_mask, uint32_t min_count, const pv_union_args a,
                                                        unsigned long long *__restrict__ records)
{
    __shared__ uint32_t s_base[SK_UNION_MAX + 1];
    __shared__ uint32_t *s_count[SK_UNION_MAX], *s_prev[SK_UNION_MAX];
    __shared__ unsigned long long cell[2 * SK_UNION_MAX];           // [member][0] rows with V >= min_count, [member][1] the sum of V
    if (threadIdx.x <= SK_UNION_MAX) s_base[threadIdx.x] = a.base[threadIdx.x];
    if (threadIdx.x < SK_UNION_MAX) { s_count[threadIdx.x] = a.count[threadIdx.x]; s_prev[threadIdx.x] = a.prev[threadIdx.x]; }
    if (threadIdx.x < 2 * SK_UNION_MAX) cell[threadIdx.x] = 0ull;
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u;
    for (uint32_t it = 0; it < 16u; it++) {
        const uint32_t g = blockIdx.x * PV_PER_BLOCK + it * 256u + threadIdx.x, g0 = g - lane;     // g0: the wave's first row
        if (g0 >= nrows) break;                                    // (wave-uniform; the later steps lie further on)
        uint32_t s = 0, V = 0, p = 0;
        if (g < nrows) {
            uint32_t lo = 0, hi = members;                         // base[lo] <= g < base[hi]
            while (hi - lo > 1u) { const uint32_t mid = (lo + hi) >> 1; if (s_base[mid] <= g) lo = mid; else hi = mid; }
            s = lo;
            if ((member_mask >> s) & 1u) {
                const uint32_t w = canon[g], i = g - s_base[s];
                V = scratch[w < nrows ? w : g];
                p = V >= min_count ? 1u : 0u;
                if (V) s_count[s][i] += V;
                if (p) s_prev[s][i] += 1u;
            }
        }
        if (!records || !__ballot(V != 0u)) continue;              // (wave-uniform)
        const uint32_t s0 = __shfl(s, 0, 64), last = g0 + 63u < nrows ? g0 + 63u : nrows - 1u;
        if (s_base[s0 + 1u] > last) {                              // the wave lies in one member
            unsigned long long h = V;
            for (int off = 32; off; off >>= 1) { p += __shfl_down(p, off, 64); h += __shfl_down(h, off, 64); }
            if (lane == 0u) {
                if (p) atomicAdd(&cell[2u * s0], (unsigned long long)p);
                if (h) atomicAdd(&cell[2u * s0 + 1u], h);
            }
        } else if (V) {
            if (p) atomicAdd(&cell[2u * s], 1ull);
            atomicAdd(&cell[2u * s + 1u], (unsigned long long)V);
        }
    }
    __syncthreads();
    if (records && threadIdx.x < 2 * SK_UNION_MAX) {
        const unsigned long long x = cell[threadIdx.x];
        if (x) atomicAdd(records + threadIdx.x, x);
    }
}

extern "C" int sk_union_item_fold(sk_union *u, uint32_t slot, uint32_t count_col, uint32_t prev_col, uint32_t member_mask, uint32_t min_count,
                                  uint64_t *d_records)
{
    if (!u) return SK_E_ARG;
    sk_ctx *ctx = sk_union_context(u);
    if (min_count < 1u) return sk_fail_(ctx, SK_E_ARG, "sk_union_item_fold: min_count must be at least 1");
    if (((uintptr_t)d_records & 7u) != 0) return sk_fail_(ctx, SK_E_ARG, "sk_union_item_fold: the records must be 8-byte aligned");
    sk_union_item_view v;
    { const int rc = sk_union_item_view_(u, slot, count_col, prev_col, member_mask, &v); if (rc != SK_OK) return rc; }
    if (!v.nrows) return SK_OK;
    const uint32_t n = v.nrows + 1u, nb = (n + PV_PER_BLOCK - 1u) / PV_PER_BLOCK;
    const hipStream_t st = (hipStream_t)v.stream;
    hipEvent_t e0 = NULL, e1 = NULL;
    pthread_mutex_lock(&pv_mu);
    const bool clocks = pv_clocks;
    pthread_mutex_unlock(&pv_mu);
    if (clocks && (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess || hipEventRecord(e0, st) != hipSuccess)) {
        (void)hipGetLastError();
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
        e0 = e1 = NULL;
    }
    {
        const int rc = sk_diff_sums_(ctx, v.d_diff, n, v.d_sums);
        if (rc != SK_OK) {                                          // (the pair is not in the list yet: nobody else destroys it)
            if (e0) (void)hipEventDestroy(e0);
            if (e1) (void)hipEventDestroy(e1);
            return rc;
        }
    }
    hipLaunchKernelGGL(union_item_gather, dim3(nb), dim3(256), 0, st, v.d_diff, n, (const uint32_t *)v.d_sums, v.d_scratch, v.d_canon, v.nrows);
    if (member_mask) {
        pv_union_args a;
        for (uint32_t s = 0; s <= SK_UNION_MAX; s++) a.base[s] = v.base[s];
        for (uint32_t s = 0; s < SK_UNION_MAX; s++) { a.count[s] = v.d_count[s]; a.prev[s] = v.d_prev[s]; }
        hipLaunchKernelGGL(union_item_apply, dim3((v.nrows + PV_PER_BLOCK - 1u) / PV_PER_BLOCK), dim3(256), 0, st, (const uint32_t *)v.d_scratch,
                           v.d_canon, v.nrows, v.members, member_mask, min_count, a, (unsigned long long *)d_records);
    }
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemsetAsync(v.d_scratch, 0, (size_t)v.nrows * 4, st);
    if (e0 && e1) {
        (void)hipEventRecord(e1, st);
        pthread_mutex_lock(&pv_mu);
        pv_ev.push_back(e0); pv_ev.push_back(e1);
        pthread_mutex_unlock(&pv_mu);
    }
    if (e != hipSuccess) return sk_fail_(ctx, SK_E_HIP, "sk_union_item_fold failed: %s", hipGetErrorString(e));
    return SK_OK;
}

extern "C" int sk_item_fold(sk_ctx *ctx, uint32_t slot, uint32_t count_col, uint32_t prev_col, uint32_t min_count, uint64_t *d_item_record)
{
    if (!ctx) return SK_E_ARG;
    if (min_count < 1u) return sk_fail_(ctx, SK_E_ARG, "sk_item_fold: min_count must be at least 1");
    if (((uintptr_t)d_item_record & 7u) != 0) return sk_fail_(ctx, SK_E_ARG, "sk_item_fold: the record must be 8-byte aligned");
    sk_item_view v;
    { const int rc = sk_item_view_(ctx, slot, count_col, prev_col, &v); if (rc != SK_OK) return rc; }
    if (!v.nrows) return SK_OK;
    const uint32_t n = v.nrows + 1u, nb = (n + PV_PER_BLOCK - 1u) / PV_PER_BLOCK;
    hipEvent_t e0 = NULL, e1 = NULL;
    pthread_mutex_lock(&pv_mu);
    const bool clocks = pv_clocks;
    pthread_mutex_unlock(&pv_mu);
    if (clocks && (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess || hipEventRecord(e0, (hipStream_t)v.stream) != hipSuccess)) {
        (void)hipGetLastError();
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
        e0 = e1 = NULL;
    }
    {
        const int rc = sk_diff_sums_(ctx, v.d_diff, n, v.d_sums);
        if (rc != SK_OK) {                                          // (the pair is not in the list yet: nobody else destroys it)
            if (e0) (void)hipEventDestroy(e0);
            if (e1) (void)hipEventDestroy(e1);
            return rc;
        }
    }
    hipLaunchKernelGGL(item_apply, dim3(nb), dim3(256), 0, (hipStream_t)v.stream, v.d_diff, n, (const uint32_t *)v.d_sums, v.d_scratch,
                       v.d_count, v.d_prev, v.nrows, min_count, (unsigned long long *)d_item_record);
    const hipError_t e = hipGetLastError();
    if (e0 && e1) {
        (void)hipEventRecord(e1, (hipStream_t)v.stream);
        pthread_mutex_lock(&pv_mu);
        pv_ev.push_back(e0); pv_ev.push_back(e1);
        pthread_mutex_unlock(&pv_mu);
    }
    if (e != hipSuccess) return sk_fail_(ctx, SK_E_HIP, "sk_item_fold failed: %s", hipGetErrorString(e));
    return SK_OK;
}
