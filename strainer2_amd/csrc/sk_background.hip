// sk_background.hip -- the background of step 4's numbers for one context (strain_detect --coverage-background; the rule is in
// include/strainer_kmer.h at sk_background_finish).  New: the reference has no counterpart -- its tables speak of the informative
// k-mers alone.
//
// The counts are made by the COUNT scan as it is (sk_scan_batch into a column of the strain's table); what is here is the pass
// where a target ends: ONE grid-stride sweep over the column, 256-thread workgroups, each row classed by the type column beside it
// (class 0 informative, 1 background).  Counted in LDS first, per class: D + 2 u32 cells -- depths 0..D and the rows above D --
// and two u64, the hits above D and all hits; a workgroup adds its non-zero cells to HBM once, with 64-bit atomics (the discipline
// of covacc_finish_spectrum, sk_covacc.hip).  Unlike there, nearly every row takes part: 99 % of a table are background rows and,
// in a metagenome that does not hold the strain, at depth 0.  So the rows at depth 0 are counted per wave -- a ballot per class
// and one LDS add of its population count -- and only covered rows take an LDS atomic of their own; the hit sums travel in
// registers and meet in a wave reduction.  The sweep writes a zero behind every covered row: the column is zero afterwards.
// The union's form of the same sweep lives with the union's kernels (sk_dev_union.hip.h: sk_union_background_sweep).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include "sk_internal.h"

#define BG_BLOCKS 256u                                              // at most this many workgroups of 256: one per CU
#define BG_CELLS (SK_BACKGROUND_MAX_DEPTH + 2u)

__global__ void __launch_bounds__(256) background_sweep(uint32_t *__restrict__ col, const uint32_t *__restrict__ type, uint32_t inf_value,
                                                        uint32_t n, uint32_t D, unsigned long long *__restrict__ out)
{
    __shared__ uint32_t bins[2][BG_CELLS];                          // [class][depth 0..D, then the rows above D]
    __shared__ unsigned long long wide[2][2];                       // [class][hits above D, all hits]
    for (uint32_t i = threadIdx.x; i < 2u * BG_CELLS; i += 256u) (&bins[0][0])[i] = 0u;
    if (threadIdx.x < 4u) (&wide[0][0])[threadIdx.x] = 0ull;
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u;
    unsigned long long tot[2] = {0ull, 0ull}, deep[2] = {0ull, 0ull};
    const uint64_t stride = (uint64_t)gridDim.x * 256u;
    for (uint64_t i0 = (uint64_t)blockIdx.x * 256u; i0 < n; i0 += stride) {            // (uniform: every lane makes the ballots)
        const uint64_t i = i0 + threadIdx.x;
        const bool live = i < n;
        const uint32_t v = live ? col[i] : 0u;
        const uint32_t cls = live && type[i] == inf_value ? 0u : 1u;
        const unsigned long long z0 = __ballot(live && !v && cls == 0u), z1 = __ballot(live && !v && cls == 1u);
        if (lane == 0u) {
            if (z0) atomicAdd(&bins[0][0], (uint32_t)__popcll(z0));
            if (z1) atomicAdd(&bins[1][0], (uint32_t)__popcll(z1));
        }
        if (!v) continue;
        col[i] = 0u;
        atomicAdd(&bins[cls][v <= D ? v : D + 1u], 1u);
        tot[cls] += v;
        if (v > D) deep[cls] += v;
    }
    for (uint32_t c = 0; c < 2u; c++) {
        unsigned long long t = tot[c], d = deep[c];
        for (int off = 32; off; off >>= 1) { t += __shfl_down(t, off, 64); d += __shfl_down(d, off, 64); }
        if (lane == 0u) {
            if (t) atomicAdd(&wide[c][1], t);
            if (d) atomicAdd(&wide[c][0], d);
        }
    }
    __syncthreads();
    const uint32_t cwords = SK_BACKGROUND_CLASS_WORDS(D);
    for (uint32_t i = threadIdx.x; i < 2u * BG_CELLS; i += 256u) {
        const uint32_t c = i / BG_CELLS, d = i - c * BG_CELLS, m = bins[c][d];
        if (!m || d > D + 1u) continue;
        atomicAdd(out + (size_t)c * cwords + (d <= D ? SK_BACKGROUND_HEAD + d : 3u), (unsigned long long)m);
    }
    if (threadIdx.x < 4u) {
        const uint32_t c = threadIdx.x >> 1, w = threadIdx.x & 1u;
        const unsigned long long m = wide[c][w];
        if (m) atomicAdd(out + (size_t)c * cwords + (w ? 2u : 4u), m);
    }
}

extern "C" int sk_background_finish(sk_ctx *ctx, uint32_t col, uint32_t type_col, uint32_t informative_value, uint32_t max_depth, uint64_t *out)
{
    if (!ctx || !out) return SK_E_ARG;
    if (max_depth > SK_BACKGROUND_MAX_DEPTH) return sk_fail_(ctx, SK_E_ARG, "depth %u above %u", max_depth, SK_BACKGROUND_MAX_DEPTH);
    sk_background_view v;
    { const int rc = sk_background_view_(ctx, col, type_col, &v); if (rc != SK_OK) return rc; }
    const uint32_t D = max_depth, words = SK_BACKGROUND_WORDS(D), cwords = SK_BACKGROUND_CLASS_WORDS(D);
    memset(out, 0, (size_t)words * sizeof *out);
    if (!v.nrows) return SK_OK;
    const hipStream_t st = (hipStream_t)v.stream;
    unsigned long long h[SK_BACKGROUND_WORDS(SK_BACKGROUND_MAX_DEPTH)];
    unsigned long long *d_out = NULL;
    hipError_t e = hipMalloc((void **)&d_out, (size_t)words * sizeof *d_out);
    if (e != hipSuccess) { (void)hipGetLastError(); return sk_fail_(ctx, SK_E_HIP, "sk_background_finish: %s", hipGetErrorString(e)); }
    uint32_t gx = (v.nrows + 255u) / 256u;
    if (gx > BG_BLOCKS) gx = BG_BLOCKS;
    e = hipMemsetAsync(d_out, 0, (size_t)words * sizeof *d_out, st);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(background_sweep, dim3(gx), dim3(256), 0, st, v.d_col, v.d_type, informative_value, v.nrows, D, d_out);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(h, d_out, (size_t)words * sizeof *d_out, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    (void)hipFree(d_out);
    if (e != hipSuccess) { (void)hipGetLastError(); return sk_fail_(ctx, SK_E_HIP, "sk_background_finish failed: %s", hipGetErrorString(e)); }
    for (uint32_t c = 0; c < 2u; c++) {                         // what the sweep leaves to the host: a class's rows and its covered rows
        unsigned long long *const o = h + (size_t)c * cwords;
        unsigned long long covered = o[3];
        for (uint32_t d = 1; d <= D; d++) covered += o[SK_BACKGROUND_HEAD + d];
        o[0] = covered + o[SK_BACKGROUND_HEAD]; o[1] = covered;
    }
    for (uint32_t i = 0; i < words; i++) out[i] = h[i];
    return SK_OK;
}
