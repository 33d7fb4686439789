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
    { const int rc = sk_diff_sums_(ctx, v.d_diff, n, v.d_sums); if (rc != SK_OK) return rc; }
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
