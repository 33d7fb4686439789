// sk_covacc.hip -- the coverage accumulator: step 4's two numbers per strain and target (reference scripts/coverage_depth.py:62-129)
// from what a TALLY launch leaves in HBM, without the hit list of step 3 (src/strain_detect.c:443-626) ever being written, for gfx950.
//
// The rule (include/strainer_kmer.h has it in full): in a run of read pairs whose records all have k bases or more the reference
// prints one line per informative hit of either mate, every line of a pair carries h1 + h2 (the mates' "all hits" tallies), and the
// script counts a line iff h1 + h2 > min_kmer_hits.  A launch leaves the sparse records {record * members + member, all, inf} and
// the hit log {window end, member << SK_UNION_ROW_BITS | row} on the device; three small kernels fold them:
//   covacc_scatter   all of every sparse record of the run -> tot[pair * members + member]  (both mates add into one cell)
//   covacc_hits      every log entry: its record by bisection of the batch's record starts, its pair, and if the pair's total passes
//                    one atomicAdd on depth[member][row].  Rows are spread over the strain and the add returns nothing: no lane
//                    waits for it (the one-address returning atomic that cost sk_union_compact 587 us does not occur here).
//   covacc_scatter   again, storing zeros: tot[] is all zero between folds, so no fold pays a memset of pairs x members.
// covacc_finish sweeps depth[] once per target: non-zero rows, their sum, and zeros left behind.  covacc_finish_regions is the same
// sweep with every non-zero row also added to the pair of its region of the strain's genome (strain_detect --coverage-regions).
// covacc_finish_spectrum is either of them with every non-zero row also counted in the bin of its depth (--coverage-spectrum).
// covacc_mark is a pass of its own in front of any of the three (recurrence: sk_recur.hip has the planes): it reads the counters and
// changes none, so a run that never marks launches exactly the sweeps it launched before.
// covacc_hits_thr is covacc_hits with every entry also classified by how many of a list of thresholds its pair's total exceeds
// (--coverage-thresholds), covacc_thr_finish the pass of its own that turns the rows' highest classes into numbers; like the mark it
// changes no counter, and a run without thresholds launches neither.
// covacc_class_scatter / covacc_class_finish are the scrub sweep (--coverage-scrub-sweep): one class byte per row, and a pass of its own
// in front of the sweep that bins the non-zero rows by class; it changes nothing at all, and a run without classes launches neither.
// covacc_scatter_sup / covacc_take are the read pairs behind those numbers (support: include/strainer_kmer.h has the rule): the scatter
// that also sums each (pair, member)'s informative tallies and marks the pair's word, and the pass between the scatter and the clearing
// scatter in which one lane per marked pair adds the pair's supporters to per-workgroup LDS tables.  A run with support off launches
// neither and allocates nothing of them.
// covacc_rar_hits / covacc_rar_pairs / covacc_rows_rar are rarefaction (step 4's numbers at nested subsamples of the read pairs): a
// classifying pass of its own over each side's log between the scatters and the clearing scatters, the run's pairs binned once per
// run, and covacc_thr_finish again over the rows' highest classes.  A run that never sets a list launches and allocates none of it.
// Every kernel is a grid-stride loop over n items with the bounds of every index it forms checked against the sizes it is given.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <new>
#include <vector>
#include "sk_internal.h"

struct cov_side {                       // one mate's results: a launch's (or the held copy's) records, log and record starts
    const uint32_t *recs; uint64_t nrecs;
    const sk_hit *hits; uint64_t nhits;
    const uint32_t *rec_start; uint32_t nrec;
    uint32_t r0, step;                  // pair j's read is record r0 + j * step
};

// record -> pair of the run, or npairs if the record is not one of the run's
__device__ __forceinline__ uint32_t cov_pair(uint32_t rec, uint32_t r0, uint32_t step, uint32_t npairs)
{
    if (rec < r0) return npairs;
    const uint32_t off = rec - r0, j = off / step;
    return (off - j * step) == 0u && j < npairs ? j : npairs;
}

__global__ void covacc_scatter(const uint32_t *__restrict__ recs, uint64_t n, uint32_t ns, uint32_t nrec, uint32_t r0, uint32_t step,
                               uint32_t npairs, uint32_t *__restrict__ tot, int clear)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint32_t key = recs[3 * i], rec = key / ns, m = key - rec * ns;
        if (rec >= nrec) continue;
        const uint32_t j = cov_pair(rec, r0, step, npairs);
        if (j >= npairs) continue;
        uint32_t *cell = tot + (size_t)j * ns + m;
        if (clear) *cell = 0u;
        else atomicAdd(cell, recs[3 * i + 1]);
    }
}

__global__ void covacc_hits(const sk_hit *__restrict__ hits, uint64_t n, const uint32_t *__restrict__ rec_start, uint32_t nrec,
                            uint32_t ns, int is_union, uint32_t r0, uint32_t step, uint32_t npairs, const uint32_t *__restrict__ tot,
                            long long min_hits, uint32_t *__restrict__ depth, const uint64_t *__restrict__ row_base,
                            const uint32_t *__restrict__ nrows, uint32_t *bad)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const sk_hit e = hits[i];
        uint32_t lo = 0, hi = nrec;                           // the last record that starts at or before the window's end
        while (hi - lo > 1u) { const uint32_t mid = lo + ((hi - lo) >> 1); if (rec_start[mid] <= e.pos) lo = mid; else hi = mid; }
        const uint32_t m = is_union ? e.row >> SK_UNION_ROW_BITS : 0u;
        const uint32_t row = is_union ? e.row & ((1u << SK_UNION_ROW_BITS) - 1u) : e.row;
        if (rec_start[lo] > e.pos || m >= ns || row >= nrows[m]) { *bad = 1u; continue; }   // (never: an entry no table row stands behind)
        const uint32_t j = cov_pair(lo, r0, step, npairs);
        if (j >= npairs) continue;
        if ((long long)tot[(size_t)j * ns + m] > min_hits) atomicAdd(depth + row_base[m] + row, 1u);
    }
}

__global__ void covacc_rows(const uint32_t *__restrict__ rows, uint64_t n, uint32_t nrows, uint32_t *__restrict__ depth)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
        if (rows[i] < nrows) atomicAdd(depth + rows[i], 1u);
}

// the records and log entries of a few records of a launch -- record 0 (first != 0) and the records from tail0 on -- copied out in the
// launch's own form: what the host needs of a folded run (the tallies and rows its last pair leaves to the read after it, and the
// record whose mate sits in another batch).  Matches are rare, so the returning atomic that numbers them costs nothing.
__global__ void covacc_pick(const uint32_t *__restrict__ recs, uint64_t nrecs, const sk_hit *__restrict__ hits, uint64_t nhits,
                            const uint32_t *__restrict__ rec_start, uint32_t nrec, uint32_t ns, int first, uint32_t tail0,
                            uint32_t *__restrict__ out_recs, uint32_t cap_r, sk_hit *__restrict__ out_hits, uint32_t cap_h,
                            uint32_t *__restrict__ cnt)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x, n = nrecs + nhits;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        if (i < nrecs) {
            const uint32_t rec = recs[3 * i] / ns;
            if (rec >= nrec || !((first && rec == 0u) || rec >= tail0)) continue;
            const uint32_t k = atomicAdd(cnt, 1u);
            if (k < cap_r) { out_recs[3 * k] = recs[3 * i]; out_recs[3 * k + 1] = recs[3 * i + 1]; out_recs[3 * k + 2] = recs[3 * i + 2]; }
        } else {
            const sk_hit e = hits[i - nrecs];
            uint32_t lo = 0, hi = nrec;
            while (hi - lo > 1u) { const uint32_t mid = lo + ((hi - lo) >> 1); if (rec_start[mid] <= e.pos) lo = mid; else hi = mid; }
            if (rec_start[lo] > e.pos || !((first && lo == 0u) || lo >= tail0)) continue;
            const uint32_t k = atomicAdd(cnt + 1, 1u);
            if (k < cap_h) out_hits[k] = e;
        }
    }
}

// blockIdx.y = member: its non-zero rows and their sum, one pair of atomics per workgroup; the rows are zero afterwards
__global__ void __launch_bounds__(256) covacc_finish(uint32_t *__restrict__ depth, const uint64_t *__restrict__ row_base,
                                                     const uint32_t *__restrict__ nrows, unsigned long long *__restrict__ out)
{
    __shared__ unsigned long long s_tot[256];
    __shared__ uint32_t s_unq[256];
    const uint32_t m = blockIdx.y, n = nrows[m];
    uint32_t *d = depth + row_base[m];
    unsigned long long t = 0;
    uint32_t u = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256u) {
        const uint32_t v = d[i];
        if (v) { d[i] = 0u; u++; t += v; }
    }
    s_tot[threadIdx.x] = t; s_unq[threadIdx.x] = u;
    __syncthreads();
    for (uint32_t w = 128u; w; w >>= 1) {
        if (threadIdx.x < w) { s_tot[threadIdx.x] += s_tot[threadIdx.x + w]; s_unq[threadIdx.x] += s_unq[threadIdx.x + w]; }
        __syncthreads();
    }
    if (threadIdx.x == 0u && s_unq[0]) {
        atomicAdd(out + 2u * m, (unsigned long long)s_unq[0]);
        atomicAdd(out + 2u * m + 1u, s_tot[0]);
    }
}

// ---- the same sweep, folded by region of the strain's genome as well (include/strainer_kmer.h has the rule) ----
// region[] holds one u32 per row: the row's region, nreg for a row without a text position.  A workgroup keeps the pairs of up to
// COV_BINS regions in LDS and adds each non-empty bin to HBM once when it is done: in a table in strain order the rows of a
// workgroup lie in one or two regions, and one global atomic per non-zero row would put them all on one address (what cost
// sk_union_compact 587 us).  More regions than COV_BINS -- windows of a few bases -- spread the rows over as many addresses, and each
// non-zero row (about 1 % of a table at most: the informative ones) adds to HBM itself.
#define COV_BINS 1024u

__global__ void covacc_map_regions(const uint32_t *__restrict__ first_pos, uint32_t nrows, const uint32_t *__restrict__ starts, uint32_t nreg,
                                   uint32_t *__restrict__ region)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nrows; i += stride) {
        const uint32_t p = first_pos[i];
        uint32_t r = nreg;
        if (p != 0xFFFFFFFFu && nreg && starts[0] <= p) {     // the last region that starts at or before the row's first base
            uint32_t lo = 0, hi = nreg;
            while (hi - lo > 1u) { const uint32_t mid = lo + ((hi - lo) >> 1); if (starts[mid] <= p) lo = mid; else hi = mid; }
            r = lo;
        }
        region[i] = r;
    }
}

// one member's rows and informative rows per region.  Every row counts here, so a thread carries the pair of the region its last
// row lay in and adds it when the region changes: in strain order that is next to never.
__global__ void __launch_bounds__(256) covacc_region_rows(const uint32_t *__restrict__ region, uint32_t n, const uint32_t *__restrict__ type,
                                                          uint32_t value, uint32_t nb, unsigned long long *__restrict__ ro)
{
    __shared__ unsigned long long b_inf[COV_BINS];
    __shared__ unsigned long long b_rows[COV_BINS];
    const bool in_lds = nb <= COV_BINS;
    if (in_lds) {
        for (uint32_t b = threadIdx.x; b < nb; b += 256u) { b_inf[b] = 0ull; b_rows[b] = 0ull; }
        __syncthreads();
    }
    uint32_t cur = 0xFFFFFFFFu;
    unsigned long long rows = 0, inf = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; ; i += (uint64_t)gridDim.x * 256u) {
        const bool more = i < n;
        const uint32_t r = more ? region[i] : 0xFFFFFFFFu;
        if (r != cur || !more) {
            if (cur < nb && rows) {
                if (in_lds) { atomicAdd(&b_rows[cur], rows); if (inf) atomicAdd(&b_inf[cur], inf); }
                else { atomicAdd(ro + 2ull * cur, rows); if (inf) atomicAdd(ro + 2ull * cur + 1ull, inf); }
            }
            cur = r; rows = 0; inf = 0;
        }
        if (!more) break;
        rows++;
        inf += type[i] == value ? 1u : 0u;
    }
    if (in_lds) {
        __syncthreads();
        for (uint32_t b = threadIdx.x; b < nb; b += 256u)
            if (b_rows[b]) { atomicAdd(ro + 2ull * b, b_rows[b]); if (b_inf[b]) atomicAdd(ro + 2ull * b + 1ull, b_inf[b]); }
    }
}

// covacc_finish, and every non-zero row adds {1, its count} to its region's pair: reg_out + 2 * reg_base[m] holds member m's
// nreg[m] + 1 pairs
__global__ void __launch_bounds__(256) covacc_finish_regions(uint32_t *__restrict__ depth, const uint64_t *__restrict__ row_base,
                                                             const uint32_t *__restrict__ nrows, const uint32_t *__restrict__ region,
                                                             const uint32_t *__restrict__ nreg, const uint64_t *__restrict__ reg_base,
                                                             unsigned long long *__restrict__ out, unsigned long long *__restrict__ reg_out)
{
    __shared__ unsigned long long s_tot[256];
    __shared__ uint32_t s_unq[256];
    __shared__ unsigned long long b_tot[COV_BINS];
    __shared__ uint32_t b_unq[COV_BINS];
    const uint32_t m = blockIdx.y, n = nrows[m], nb = nreg[m] + 1u;
    const bool in_lds = nb <= COV_BINS;
    uint32_t *d = depth + row_base[m];
    const uint32_t *rg = region + row_base[m];
    unsigned long long *ro = reg_out + 2ull * reg_base[m];
    if (in_lds) {
        for (uint32_t b = threadIdx.x; b < nb; b += 256u) { b_tot[b] = 0ull; b_unq[b] = 0u; }
        __syncthreads();
    }
    unsigned long long t = 0;
    uint32_t u = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256u) {
        const uint32_t v = d[i];
        if (!v) continue;
        d[i] = 0u; u++; t += v;
        const uint32_t r = rg[i];
        if (r >= nb) continue;                                // (never: a region no start stands behind)
        if (in_lds) { atomicAdd(&b_unq[r], 1u); atomicAdd(&b_tot[r], (unsigned long long)v); }
        else { atomicAdd(ro + 2ull * r, 1ull); atomicAdd(ro + 2ull * r + 1ull, (unsigned long long)v); }
    }
    s_tot[threadIdx.x] = t; s_unq[threadIdx.x] = u;
    __syncthreads();
    for (uint32_t w = 128u; w; w >>= 1) {
        if (threadIdx.x < w) { s_tot[threadIdx.x] += s_tot[threadIdx.x + w]; s_unq[threadIdx.x] += s_unq[threadIdx.x + w]; }
        __syncthreads();
    }
    if (!s_unq[0]) return;                                    // (the whole workgroup: nothing to add anywhere)
    if (threadIdx.x == 0u) {
        atomicAdd(out + 2u * m, (unsigned long long)s_unq[0]);
        atomicAdd(out + 2u * m + 1u, s_tot[0]);
    }
    if (in_lds)
        for (uint32_t b = threadIdx.x; b < nb; b += 256u)
            if (b_unq[b]) { atomicAdd(ro + 2ull * b, (unsigned long long)b_unq[b]); atomicAdd(ro + 2ull * b + 1ull, b_tot[b]); }
}

// ---- the same sweep with the depth spectrum (include/strainer_kmer.h has the rule; strain_detect --coverage-spectrum) ----
// covacc_finish (REGIONS: covacc_finish_regions), and every non-zero row of count v also adds 1 to bin min(v, D + 1) - 1 of its
// member's spectrum and, above D, v to the member's deep sum.  The D + 1 <= COV_SPEC_BINS bins are always in LDS; a workgroup adds
// its non-empty ones to HBM once.  The bins take plain LDS atomics, not a sub-histogram per wave: only informative rows are ever
// non-zero, about 1 % of a table, so a wave's 64 rows hold 0.6 of them on average and two lanes of one DS instruction on one bin are
// the exception; where every row is non-zero at one depth (the test of 70 001 rows at depth 1) the adds of a wave serialise on one
// bank and the sweep is as correct and still one pass.  Sub-histograms would cost 4 x 4 KB of LDS and a merge in every workgroup to
// win that case only.  (An argument from the shape of the data; profiles/coverage_spectrum_bench.txt has what was measured.)
#define COV_SPEC_BINS (SK_COVACC_SPECTRUM_MAX + 1u)

template <bool REGIONS>
__global__ void __launch_bounds__(256) covacc_finish_spectrum(uint32_t *__restrict__ depth, const uint64_t *__restrict__ row_base,
                                                              const uint32_t *__restrict__ nrows, const uint32_t *__restrict__ region,
                                                              const uint32_t *__restrict__ nreg, const uint64_t *__restrict__ reg_base,
                                                              unsigned long long *__restrict__ out, unsigned long long *__restrict__ reg_out,
                                                              uint32_t max_depth, unsigned long long *__restrict__ spec,
                                                              unsigned long long *__restrict__ deep)
{
    __shared__ unsigned long long s_tot[256];
    __shared__ uint32_t s_unq[256];
    __shared__ uint32_t h_n[COV_SPEC_BINS];
    __shared__ unsigned long long h_deep;
    __shared__ unsigned long long b_tot[REGIONS ? COV_BINS : 1u];
    __shared__ uint32_t b_unq[REGIONS ? COV_BINS : 1u];
    const uint32_t m = blockIdx.y, n = nrows[m];
    const uint32_t D = max_depth < SK_COVACC_SPECTRUM_MAX ? max_depth : SK_COVACC_SPECTRUM_MAX, ns = D + 1u;   // (ns <= COV_SPEC_BINS)
    const uint32_t nb = REGIONS ? nreg[m] + 1u : 0u;
    const bool in_lds = REGIONS && nb <= COV_BINS;
    uint32_t *d = depth + row_base[m];
    const uint32_t *rg = REGIONS ? region + row_base[m] : NULL;
    unsigned long long *ro = REGIONS ? reg_out + 2ull * reg_base[m] : NULL;
    for (uint32_t b = threadIdx.x; b < ns; b += 256u) h_n[b] = 0u;
    if (threadIdx.x == 0u) h_deep = 0ull;
    if (in_lds)
        for (uint32_t b = threadIdx.x; b < nb; b += 256u) { b_tot[b] = 0ull; b_unq[b] = 0u; }
    __syncthreads();
    unsigned long long t = 0;
    uint32_t u = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256u) {
        const uint32_t v = d[i];
        if (!v) continue;
        d[i] = 0u; u++; t += v;
        atomicAdd(&h_n[(v < ns ? v : ns) - 1u], 1u);
        if (v > D) atomicAdd(&h_deep, (unsigned long long)v);
        if (REGIONS) {
            const uint32_t r = rg[i];
            if (r >= nb) continue;                            // (never: a region no start stands behind)
            if (in_lds) { atomicAdd(&b_unq[r], 1u); atomicAdd(&b_tot[r], (unsigned long long)v); }
            else { atomicAdd(ro + 2ull * r, 1ull); atomicAdd(ro + 2ull * r + 1ull, (unsigned long long)v); }
        }
    }
    s_tot[threadIdx.x] = t; s_unq[threadIdx.x] = u;
    __syncthreads();
    for (uint32_t w = 128u; w; w >>= 1) {
        if (threadIdx.x < w) { s_tot[threadIdx.x] += s_tot[threadIdx.x + w]; s_unq[threadIdx.x] += s_unq[threadIdx.x + w]; }
        __syncthreads();
    }
    if (!s_unq[0]) return;                                    // (the whole workgroup: nothing to add anywhere)
    if (threadIdx.x == 0u) {
        atomicAdd(out + 2u * m, (unsigned long long)s_unq[0]);
        atomicAdd(out + 2u * m + 1u, s_tot[0]);
        if (h_deep) atomicAdd(deep + m, h_deep);
    }
    for (uint32_t b = threadIdx.x; b < ns; b += 256u)
        if (h_n[b]) atomicAdd(spec + (size_t)m * ns + b, (unsigned long long)h_n[b]);
    if (in_lds)
        for (uint32_t b = threadIdx.x; b < nb; b += 256u)
            if (b_unq[b]) { atomicAdd(ro + 2ull * b, (unsigned long long)b_unq[b]); atomicAdd(ro + 2ull * b + 1ull, b_tot[b]); }
}

// ---- recurrence: each informative row's bit, and the pass that sets the bits of a target's non-zero rows ----
// irank[row] = the row's rank among its member's informative rows, 0xFFFFFFFF for every other row: an exclusive prefix count over the
// member's rows as a block scan in three small kernels -- the informative rows of each block of 256, an exclusive scan of the blocks'
// counts by one workgroup, and each row's rank within its block on top of its block's.
__device__ __forceinline__ uint32_t cov_block_rank(bool f, uint32_t *s_w, uint32_t *total)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const unsigned long long bal = __ballot(f);
    if (lane == 0u) s_w[wave] = (uint32_t)__popcll(bal);
    __syncthreads();
    uint32_t before = 0, all = 0;
    for (uint32_t w = 0; w < 4u; w++) { if (w < wave) before += s_w[w]; all += s_w[w]; }
    *total = all;
    return before + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
}

__global__ void __launch_bounds__(256) covacc_rank_count(const uint32_t *__restrict__ type, uint32_t n, uint32_t value, uint32_t *__restrict__ blk)
{
    __shared__ uint32_t s_w[4];
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    uint32_t total;
    (void)cov_block_rank(i < n && type[i] == value, s_w, &total);
    if (threadIdx.x == 0u) blk[blockIdx.x] = total;
}

// one workgroup: blk[] becomes its exclusive prefix sums, blk[nblk] the total
__global__ void __launch_bounds__(256) covacc_rank_scan(uint32_t *__restrict__ blk, uint32_t nblk)
{
    __shared__ uint32_t s[256];
    __shared__ uint32_t carry;
    if (threadIdx.x == 0u) carry = 0u;
    __syncthreads();
    for (uint32_t b0 = 0; b0 < nblk; b0 += 256u) {
        const uint32_t i = b0 + threadIdx.x, v = i < nblk ? blk[i] : 0u;
        s[threadIdx.x] = v;
        __syncthreads();
        for (uint32_t d = 1u; d < 256u; d <<= 1) {
            const uint32_t t = threadIdx.x >= d ? s[threadIdx.x - d] : 0u;
            __syncthreads();
            s[threadIdx.x] += t;
            __syncthreads();
        }
        if (i < nblk) blk[i] = carry + s[threadIdx.x] - v;
        __syncthreads();
        if (threadIdx.x == 0u) carry += s[255];
        __syncthreads();
    }
    if (threadIdx.x == 0u) blk[nblk] = carry;
}

__global__ void __launch_bounds__(256) covacc_rank_write(const uint32_t *__restrict__ type, uint32_t n, uint32_t value,
                                                         const uint32_t *__restrict__ blk, uint32_t *__restrict__ irank)
{
    __shared__ uint32_t s_w[4];
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const bool f = i < n && type[i] == value;
    uint32_t total;
    const uint32_t r = cov_block_rank(f, s_w, &total);
    if (i < n) irank[i] = f ? blk[blockIdx.x] + r : 0xFFFFFFFFu;
}

// blockIdx.y = member: every row with a non-zero counter sets its bit of plane[word_base[m] ..]; a non-zero row whose rank is not
// below the member's nbits (0xFFFFFFFF: not informative) sets nothing and is counted.  The counters are only read.
__global__ void __launch_bounds__(256) covacc_mark(const uint32_t *__restrict__ depth, const uint64_t *__restrict__ row_base,
                                                   const uint32_t *__restrict__ nrows, const uint32_t *__restrict__ irank,
                                                   const uint32_t *__restrict__ nbits, const uint64_t *__restrict__ word_base,
                                                   unsigned long long *__restrict__ plane, unsigned long long *__restrict__ stray)
{
    const uint32_t m = blockIdx.y, n = nrows[m], nb = nbits[m];
    const uint32_t *d = depth + row_base[m], *rk = irank + row_base[m];
    unsigned long long *p = plane + word_base[m];
    uint32_t bad = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256u) {
        if (!d[i]) continue;
        const uint32_t b = rk[i];
        if (b < nb) atomicOr(p + (b >> 6), 1ull << (b & 63u));
        else bad++;
    }
    if (bad) atomicAdd(stray, (unsigned long long)bad);      // (never in the programs: only informative rows are logged)
}

// ---- thresholds: step 4's two numbers at several min_kmer_hits from one pass (include/strainer_kmer.h has the rule) ----
// The class of a log entry is c = the number of thresholds its pair's total exceeds (the list ascends, so c says which).  total[q] is
// the number of entries of class > q and unique[q] the number of rows with some entry of class > q, so the folds keep
//   cls_cnt[member][c]   entries per class: LDS bins per workgroup, one 64-bit atomic per non-empty bin and workgroup at its end;
//   thr_max[row]         the row's highest class: one atomicMax per entry with c >= 1, spread over the rows as the depth adds are,
// and covacc_thr_finish bins thr_max[] by class (and leaves it zero); the host takes the suffix sums.  One u32 per accumulator row
// whatever the list's length.  Most entries of a wave share one (member, class) -- a present strain's pairs pass every threshold --
// so the lanes of a wave first agree on who holds which bin and the first lane of each bin adds the count for all of them
// (cov_bin_add): one LDS atomic per distinct bin and wave, not 64 on one address.
#define COV_THR_CLASSES (SK_COVACC_THRESHOLDS_MAX + 1u)
#define COV_THR_LDS_MEMBERS SK_UNION_MAX
struct cov_thr { long long t[SK_COVACC_THRESHOLDS_MAX]; uint32_t n; };

__device__ __forceinline__ uint32_t cov_class(const cov_thr &th, uint32_t total)
{
    uint32_t c = 0;
    const uint32_t n = th.n < SK_COVACC_THRESHOLDS_MAX ? th.n : SK_COVACC_THRESHOLDS_MAX;
    for (uint32_t q = 0; q < n; q++) c += (long long)total > th.t[q] ? 1u : 0u;
    return c;
}

// every lane of the wave calls it (converged); bin = 0xFFFFFFFF: this lane has nothing.  bins[] has nbins entries.
__device__ __forceinline__ void cov_bin_add(unsigned long long *bins, uint32_t nbins, uint32_t bin)
{
    const uint32_t lane = threadIdx.x & 63u;
    if (bin >= nbins) bin = 0xFFFFFFFFu;
    unsigned long long todo = __ballot(bin != 0xFFFFFFFFu);
    while (todo) {
        const uint32_t lead = (uint32_t)__builtin_ctzll(todo);
        const uint32_t b0 = (uint32_t)__shfl((int)bin, (int)lead);
        const unsigned long long same = __ballot(bin == b0);
        if (lane == lead) atomicAdd(&bins[b0], (unsigned long long)__popcll(same));
        todo &= ~same;
    }
}

// covacc_hits, and every entry also classified: cls_cnt + member0's offset is the caller's, thr_max indexed like depth
__global__ void __launch_bounds__(256) covacc_hits_thr(const sk_hit *__restrict__ hits, uint64_t n, const uint32_t *__restrict__ rec_start,
                                                       uint32_t nrec, uint32_t ns, int is_union, uint32_t r0, uint32_t step, uint32_t npairs,
                                                       const uint32_t *__restrict__ tot, long long min_hits, uint32_t *__restrict__ depth,
                                                       const uint64_t *__restrict__ row_base, const uint32_t *__restrict__ nrows, uint32_t *bad,
                                                       cov_thr th, uint32_t *__restrict__ thr_max, unsigned long long *__restrict__ cls_cnt)
{
    __shared__ unsigned long long s_bin[COV_THR_LDS_MEMBERS * COV_THR_CLASSES];
    const bool in_lds = ns <= COV_THR_LDS_MEMBERS;
    const uint32_t nbins = in_lds ? ns * COV_THR_CLASSES : 0u;
    for (uint32_t b = threadIdx.x; b < nbins; b += 256u) s_bin[b] = 0ull;
    __syncthreads();
    const uint64_t stride = (uint64_t)gridDim.x * 256u;
    for (uint64_t i0 = (uint64_t)blockIdx.x * 256u; i0 < n; i0 += stride) {      // (i0 is the workgroup's: every wave stays whole)
        const uint64_t i = i0 + threadIdx.x;
        uint32_t bin = 0xFFFFFFFFu;
        if (i < n) {
            const sk_hit e = hits[i];
            uint32_t lo = 0, hi = nrec;
            while (hi - lo > 1u) { const uint32_t mid = lo + ((hi - lo) >> 1); if (rec_start[mid] <= e.pos) lo = mid; else hi = mid; }
            const uint32_t m = is_union ? e.row >> SK_UNION_ROW_BITS : 0u;
            const uint32_t row = is_union ? e.row & ((1u << SK_UNION_ROW_BITS) - 1u) : e.row;
            if (rec_start[lo] > e.pos || m >= ns || row >= nrows[m]) *bad = 1u;   // (never: an entry no table row stands behind)
            else {
                const uint32_t j = cov_pair(lo, r0, step, npairs);
                if (j < npairs) {
                    const uint32_t total = tot[(size_t)j * ns + m];
                    if ((long long)total > min_hits) atomicAdd(depth + row_base[m] + row, 1u);
                    const uint32_t c = cov_class(th, total);
                    if (c) {
                        atomicMax(thr_max + row_base[m] + row, c);
                        if (in_lds) bin = m * COV_THR_CLASSES + c;
                        else atomicAdd(cls_cnt + (size_t)m * COV_THR_CLASSES + c, 1ull);
                    }
                }
            }
        }
        if (in_lds) cov_bin_add(s_bin, nbins, bin);
    }
    __syncthreads();
    for (uint32_t b = threadIdx.x; b < nbins; b += 256u)
        if (s_bin[b]) atomicAdd(cls_cnt + b, s_bin[b]);
}

// host-replayed entries of one member, unfiltered, each with its pair's total: depth/thr_max are the member's, cls_cnt its
// COV_THR_CLASSES bins; th.n = 0: only the main counters
__global__ void __launch_bounds__(256) covacc_rows_hits(const uint32_t *__restrict__ rows, const uint32_t *__restrict__ totals, uint64_t n,
                                                        uint32_t nrows, long long min_hits, uint32_t *__restrict__ depth, cov_thr th,
                                                        uint32_t *__restrict__ thr_max, unsigned long long *__restrict__ cls_cnt)
{
    __shared__ unsigned long long s_bin[COV_THR_CLASSES];
    if (threadIdx.x < COV_THR_CLASSES) s_bin[threadIdx.x] = 0ull;
    __syncthreads();
    const uint64_t stride = (uint64_t)gridDim.x * 256u;
    for (uint64_t i0 = (uint64_t)blockIdx.x * 256u; i0 < n; i0 += stride) {
        const uint64_t i = i0 + threadIdx.x;
        uint32_t bin = 0xFFFFFFFFu;
        if (i < n && rows[i] < nrows) {
            const uint32_t total = totals[i];
            if ((long long)total > min_hits) atomicAdd(depth + rows[i], 1u);
            const uint32_t c = cov_class(th, total);
            if (c) { atomicMax(thr_max + rows[i], c); bin = c; }
        }
        if (th.n) cov_bin_add(s_bin, COV_THR_CLASSES, bin);
    }
    __syncthreads();
    if (th.n && threadIdx.x < COV_THR_CLASSES && s_bin[threadIdx.x]) atomicAdd(cls_cnt + threadIdx.x, s_bin[threadIdx.x]);
}

// blockIdx.y = member: its rows' highest classes binned into row_cnt[m][class]; thr_max is zero afterwards.  The depth counters are
// not touched.
__global__ void __launch_bounds__(256) covacc_thr_finish(uint32_t *__restrict__ thr_max, const uint64_t *__restrict__ row_base,
                                                         const uint32_t *__restrict__ nrows, unsigned long long *__restrict__ row_cnt)
{
    __shared__ unsigned long long s_bin[COV_THR_CLASSES];
    const uint32_t m = blockIdx.y, n = nrows[m];
    uint32_t *mx = thr_max + row_base[m];
    if (threadIdx.x < COV_THR_CLASSES) s_bin[threadIdx.x] = 0ull;
    __syncthreads();
    for (uint64_t i0 = (uint64_t)blockIdx.x * 256u; i0 < n; i0 += (uint64_t)gridDim.x * 256u) {
        const uint64_t i = i0 + threadIdx.x;
        uint32_t bin = 0xFFFFFFFFu;
        if (i < n) {
            const uint32_t v = mx[i];
            if (v) { mx[i] = 0u; bin = v; }                   // (v < COV_THR_CLASSES, or cov_bin_add drops it)
        }
        cov_bin_add(s_bin, COV_THR_CLASSES, bin);
    }
    __syncthreads();
    if (threadIdx.x < COV_THR_CLASSES && s_bin[threadIdx.x]) atomicAdd(row_cnt + (size_t)m * COV_THR_CLASSES + threadIdx.x, s_bin[threadIdx.x]);
}

// ---- the scrub sweep: step 4's numbers at several min_fraction from one pass (include/strainer_kmer.h has the rule) ----
// A row's class is the number of listed fractions whose informative set holds it; the sets are nested, so the numbers at fraction q
// are sums over the non-zero rows of class >= q + 1.  covacc_class_finish bins a member's non-zero rows by exact class into
// {rows, sum of depth} pairs and the host takes the suffix sums.  All rows of a workgroup fall into at most 16 bins, so the lanes of
// a wave first reduce count and sum per class present among them and one lane adds each (wave, class) to the LDS bins; every
// workgroup ends with one pair of 64-bit adds per non-empty bin.
#define COV_CLS_NONE 0xFFu

// rows[i] of the member gets cls[i]; out is the member's (zeroed before).  The host has checked both ranges already.
__global__ void covacc_class_scatter(const uint32_t *__restrict__ rows, const uint8_t *__restrict__ cls, uint64_t n, uint32_t nrows,
                                     uint32_t ncls, uint8_t *__restrict__ out)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint32_t r = rows[i], c = cls[i];
        if (r < nrows && c >= 1u && c <= ncls) out[r] = (uint8_t)c;
    }
}

__device__ __forceinline__ unsigned long long cov_wave_sum(unsigned long long v)
{
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned lo = (unsigned)__shfl_down((int)(unsigned)v, off), hi = (unsigned)__shfl_down((int)(unsigned)(v >> 32), off);
        v += ((unsigned long long)hi << 32) | lo;
    }
    return v;
}

// blockIdx.y = member: out[(m * MAX + c - 1) * 2 + {0, 1}] += the member's non-zero rows of class c and the sum of their depths;
// *stray += its non-zero rows of class 0 or above ncls[m].  A member with ncls[m] = 0 is skipped.  Nothing is written but out and stray.
__global__ void __launch_bounds__(256) covacc_class_finish(const uint32_t *__restrict__ depth, const uint64_t *__restrict__ row_base,
                                                           const uint32_t *__restrict__ nrows, const uint8_t *__restrict__ cls,
                                                           const uint32_t *__restrict__ ncls, unsigned long long *__restrict__ out,
                                                           unsigned long long *__restrict__ stray)
{
    __shared__ unsigned long long s_cnt[SK_SCRUB_SWEEP_MAX], s_sum[SK_SCRUB_SWEEP_MAX];
    __shared__ uint32_t s_bad;
    const uint32_t m = blockIdx.y, n = nrows[m], lane = threadIdx.x & 63u;
    const uint32_t nc = ncls[m] < SK_SCRUB_SWEEP_MAX ? ncls[m] : SK_SCRUB_SWEEP_MAX;
    if (!nc) return;                                          // (the whole workgroup)
    const uint32_t *d = depth + row_base[m];
    const uint8_t *cl = cls + row_base[m];
    if (threadIdx.x < SK_SCRUB_SWEEP_MAX) { s_cnt[threadIdx.x] = 0ull; s_sum[threadIdx.x] = 0ull; }
    if (threadIdx.x == 0) s_bad = 0u;
    __syncthreads();
    uint32_t bad = 0;
    for (uint64_t i0 = (uint64_t)blockIdx.x * 256u; i0 < n; i0 += (uint64_t)gridDim.x * 256u) {   // (i0 is the workgroup's: every wave stays whole)
        const uint64_t i = i0 + threadIdx.x;
        uint32_t v = 0, c = COV_CLS_NONE;
        if (i < n && (v = d[i]) != 0u) {
            c = cl[i];
            if (c < 1u || c > nc) { bad++; c = COV_CLS_NONE; }
        }
        unsigned long long todo = __ballot(c != COV_CLS_NONE);
        while (todo) {                                        // one round per class present in the wave
            const uint32_t lead = (uint32_t)__builtin_ctzll(todo);
            const uint32_t c0 = (uint32_t)__shfl((int)c, (int)lead);
            const unsigned long long same = __ballot(c == c0);
            const unsigned long long sum = cov_wave_sum(c == c0 ? (unsigned long long)v : 0ull);
            if (lane == 0u && c0 >= 1u && c0 <= SK_SCRUB_SWEEP_MAX) {
                atomicAdd(&s_cnt[c0 - 1u], (unsigned long long)__popcll(same));
                atomicAdd(&s_sum[c0 - 1u], sum);
            }
            todo &= ~same;
        }
    }
    if (bad) atomicAdd(&s_bad, bad);
    __syncthreads();
    if (threadIdx.x < nc && s_cnt[threadIdx.x]) {
        unsigned long long *o = out + ((size_t)m * SK_SCRUB_SWEEP_MAX + threadIdx.x) * 2u;
        atomicAdd(o, s_cnt[threadIdx.x]);
        atomicAdd(o + 1, s_sum[threadIdx.x]);
    }
    if (threadIdx.x == 0 && s_bad) atomicAdd(stray, (unsigned long long)s_bad);
}

// ---- support: the read pairs behind step 4's numbers, per member and across the members of a launch (include/strainer_kmer.h) ----
// An emission of (pair j, member m) in a folded run is tot[j, m] > min_hits with inf[j, m] >= 1, its lines L = inf[j, m] (both mates'
// informative tallies).  Three steps inside the fold:
//   mark   covacc_scatter_sup is covacc_scatter, and a record with inf > 0 also adds inf to sinf[pair * members + member] and sets bit
//          member (side 0: PE1) or 32 + member (side 1: PE2) of word[pair] with a 64-bit atomicOr that returns nothing.  Both arrays
//          are all zero between folds, as tot[] is.
//   take   covacc_take, behind a kernel boundary: every record with inf > 0 exchanges its pair's word for 0; the one lane that gets a
//          non-zero word owns the pair.  At most 2 x members records meet on one word and the pairs are spread over the run, so the
//          returning atomic is not the one-address queue that cost sk_union_compact 587 us.  The owner masks the word by "member
//          passes tot > min_hits" -- S = (PE1 | PE2) & pass, both = PE1 & PE2 & pass -- and adds to the workgroup's LDS tables: per
//          member {pairs, lines, both}, per ordered (a, b) of S x S {pairs, lines of a}; the diagonal takes only pairs with |S| = 1
//          (the exclusive ones).  Two 32 x 32 tables of 64-bit cells plus 32 x 3: sk_union_share's layout.  A pair that supports all
//          32 members costs its owner 32 x 31 x 2 LDS adds in a divergent loop; real pairs support one member or two.  Each workgroup
//          adds its non-zero cells to the target's accumulators once, with 64-bit global atomics.
//   clear  the clearing scatter also zeroes the sinf cells; the words are zero after the take.
#define COV_SUP_M SK_UNION_MAX

__global__ void covacc_scatter_sup(const uint32_t *__restrict__ recs, uint64_t n, uint32_t ns, uint32_t nrec, uint32_t r0, uint32_t step,
                                   uint32_t npairs, uint32_t *__restrict__ tot, uint32_t *__restrict__ sinf,
                                   unsigned long long *__restrict__ word, uint32_t side, int clear)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint32_t key = recs[3 * i], rec = key / ns, m = key - rec * ns;
        if (rec >= nrec) continue;
        const uint32_t j = cov_pair(rec, r0, step, npairs);
        if (j >= npairs) continue;
        const size_t cell = (size_t)j * ns + m;
        if (clear) { tot[cell] = 0u; sinf[cell] = 0u; continue; }
        atomicAdd(tot + cell, recs[3 * i + 1]);                // (exactly covacc_scatter up to here)
        const uint32_t inf = recs[3 * i + 2];
        if (inf && m < COV_SUP_M) {                           // (m >= COV_SUP_M never: the host refuses launches of more members; no bit stands for it)
            atomicAdd(sinf + cell, inf);
            atomicOr(word + j, (unsigned long long)(1u << m) << (side ? 32u : 0u));
        }
    }
}

// acc: [nm x 3] {pairs, lines, both} per member, then [nm x nm] shared pairs, then [nm x nm] lines of the row's member; the launch's
// members are members member0 .. member0 + ns - 1 of the accumulator's nm (the host has checked that they fit, and ns <= COV_SUP_M)
__global__ void __launch_bounds__(256) covacc_take(const uint32_t *__restrict__ recs, uint64_t n, uint32_t ns, uint32_t nrec, uint32_t r0,
                                                   uint32_t step, uint32_t npairs, const uint32_t *__restrict__ tot,
                                                   const uint32_t *__restrict__ sinf, unsigned long long *__restrict__ word,
                                                   long long min_hits, uint32_t member0, uint32_t nm, unsigned long long *__restrict__ acc)
{
    __shared__ unsigned long long s_pairs[COV_SUP_M * COV_SUP_M], s_lines[COV_SUP_M * COV_SUP_M], s_mem[COV_SUP_M * 3u];
    for (uint32_t c = threadIdx.x; c < COV_SUP_M * COV_SUP_M; c += 256u) { s_pairs[c] = 0ull; s_lines[c] = 0ull; }
    if (threadIdx.x < COV_SUP_M * 3u) s_mem[threadIdx.x] = 0ull;
    __syncthreads();
    if (ns > COV_SUP_M || member0 >= nm || ns > nm - member0) return;     // (never; the whole workgroup)
    const uint32_t all = ns >= 32u ? 0xFFFFFFFFu : (1u << ns) - 1u;
    const uint64_t stride = (uint64_t)gridDim.x * 256u;
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n; i += stride) {
        if (!recs[3 * i + 2]) continue;
        const uint32_t key = recs[3 * i], rec = key / ns;
        if (rec >= nrec) continue;
        const uint32_t j = cov_pair(rec, r0, step, npairs);
        if (j >= npairs) continue;
        const unsigned long long w = atomicExch(word + j, 0ull);
        if (!w) continue;                                     // another lane owns the pair (or owned it)
        const uint32_t lo = (uint32_t)w & all, hi = (uint32_t)(w >> 32) & all;
        const uint32_t *t = tot + (size_t)j * ns, *li = sinf + (size_t)j * ns;
        uint32_t pass = 0;
        for (uint32_t b = lo | hi; b; b &= b - 1u) {
            const uint32_t m = (uint32_t)__builtin_ctz(b);
            if ((long long)t[m] > min_hits) pass |= 1u << m;
        }
        const uint32_t S = (lo | hi) & pass, both = lo & hi & pass;
        if (!S) continue;
        const bool alone = (S & (S - 1u)) == 0u;
        for (uint32_t x = S; x; x &= x - 1u) {
            const uint32_t a = (uint32_t)__builtin_ctz(x);
            const unsigned long long L = li[a];
            atomicAdd(&s_mem[a * 3u], 1ull);
            atomicAdd(&s_mem[a * 3u + 1u], L);
            if (both & (1u << a)) atomicAdd(&s_mem[a * 3u + 2u], 1ull);
            if (alone) { atomicAdd(&s_pairs[a * COV_SUP_M + a], 1ull); atomicAdd(&s_lines[a * COV_SUP_M + a], L); continue; }
            for (uint32_t y = S & ~(1u << a); y; y &= y - 1u) {
                const uint32_t b = (uint32_t)__builtin_ctz(y);
                atomicAdd(&s_pairs[a * COV_SUP_M + b], 1ull);
                atomicAdd(&s_lines[a * COV_SUP_M + b], L);
            }
        }
    }
    __syncthreads();
    unsigned long long *g_pairs = acc + (size_t)nm * 3u, *g_lines = g_pairs + (size_t)nm * nm;
    for (uint32_t c = threadIdx.x; c < COV_SUP_M * COV_SUP_M; c += 256u) {
        const uint32_t a = c / COV_SUP_M, b = c - a * COV_SUP_M;
        if (a >= ns || b >= ns || !s_pairs[c]) continue;
        const size_t g = (size_t)(member0 + a) * nm + member0 + b;
        atomicAdd(g_pairs + g, s_pairs[c]);
        if (s_lines[c]) atomicAdd(g_lines + g, s_lines[c]);
    }
    if (threadIdx.x < COV_SUP_M * 3u && threadIdx.x / 3u < ns && s_mem[threadIdx.x])
        atomicAdd(acc + (size_t)member0 * 3u + threadIdx.x, s_mem[threadIdx.x]);
}

// ---- rarefaction: step 4's numbers at nested subsamples of the read pairs, from one pass (include/strainer_kmer.h has the rule) ----
// Pair i of the target draws u(i), a function of its ordinal and the seed alone; it is in subsample q iff u(i) < T[q], and its class is
// the number of listed q that hold it (T descends, so those are q = 0 .. class - 1).  The structure is the thresholds': every counted
// line of a pair of class c >= 1 adds to rar_cnt[member][c] (LDS bins, cov_bin_add) and raises rar_max[row] to c; covacc_thr_finish --
// the same 17 bins -- turns rar_max[] into rows per class, and the host takes suffix sums.  covacc_rar_hits is a pass of its own over a
// side's log, between the scatters and the clearing scatter: it writes no depth counter, so it stands behind covacc_hits,
// covacc_hits_thr and the support take alike, and a run with rarefaction off launches none of this.  covacc_rar_pairs bins the run's
// pairs themselves, once per run.
#define COV_RAR_CLASSES (SK_COVACC_RAREFACTION_MAX + 1u)
static_assert(COV_RAR_CLASSES == COV_THR_CLASSES, "covacc_thr_finish bins both tables' row classes");
struct cov_rar { unsigned long long t[SK_COVACC_RAREFACTION_MAX]; uint32_t n, seed; };

__device__ __forceinline__ uint32_t cov_rar_draw(unsigned long long i, uint32_t seed)
{
    uint32_t x = (uint32_t)i ^ ((uint32_t)(i >> 32) * 0x9E3779B9u) ^ seed;
    x ^= x >> 16; x *= 0x85EBCA6Bu;
    x ^= x >> 13; x *= 0xC2B2AE35u;
    x ^= x >> 16;
    return x;
}

__device__ __forceinline__ uint32_t cov_rar_class(const cov_rar &rf, unsigned long long pair)
{
    const unsigned long long u = cov_rar_draw(pair, rf.seed);
    const uint32_t n = rf.n < SK_COVACC_RAREFACTION_MAX ? rf.n : SK_COVACC_RAREFACTION_MAX;
    uint32_t c = 0;
    for (uint32_t q = 0; q < n; q++) c += u < rf.t[q] ? 1u : 0u;
    return c;
}

// every log entry of a side whose pair's total passes: the pair's class to rar_max[row] and to the (member, class) bin.  An entry no
// table row stands behind is left out here; the fold in front of this pass has reported it.
__global__ void __launch_bounds__(256) covacc_rar_hits(const sk_hit *__restrict__ hits, uint64_t n, const uint32_t *__restrict__ rec_start,
                                                       uint32_t nrec, uint32_t ns, int is_union, uint32_t r0, uint32_t step, uint32_t npairs,
                                                       const uint32_t *__restrict__ tot, long long min_hits,
                                                       const uint64_t *__restrict__ row_base, const uint32_t *__restrict__ nrows,
                                                       cov_rar rf, unsigned long long pair_base, uint32_t *__restrict__ rar_max,
                                                       unsigned long long *__restrict__ rar_cnt)
{
    __shared__ unsigned long long s_bin[COV_THR_LDS_MEMBERS * COV_RAR_CLASSES];
    const bool in_lds = ns <= COV_THR_LDS_MEMBERS;
    const uint32_t nbins = in_lds ? ns * COV_RAR_CLASSES : 0u;
    for (uint32_t b = threadIdx.x; b < nbins; b += 256u) s_bin[b] = 0ull;
    __syncthreads();
    const uint64_t stride = (uint64_t)gridDim.x * 256u;
    for (uint64_t i0 = (uint64_t)blockIdx.x * 256u; i0 < n; i0 += stride) {      // (i0 is the workgroup's: every wave stays whole)
        const uint64_t i = i0 + threadIdx.x;
        uint32_t bin = 0xFFFFFFFFu;
        if (i < n) {
            const sk_hit e = hits[i];
            uint32_t lo = 0, hi = nrec;
            while (hi - lo > 1u) { const uint32_t mid = lo + ((hi - lo) >> 1); if (rec_start[mid] <= e.pos) lo = mid; else hi = mid; }
            const uint32_t m = is_union ? e.row >> SK_UNION_ROW_BITS : 0u;
            const uint32_t row = is_union ? e.row & ((1u << SK_UNION_ROW_BITS) - 1u) : e.row;
            if (rec_start[lo] <= e.pos && m < ns && row < nrows[m]) {
                const uint32_t j = cov_pair(lo, r0, step, npairs);
                if (j < npairs && (long long)tot[(size_t)j * ns + m] > min_hits) {
                    const uint32_t c = cov_rar_class(rf, pair_base + j);
                    if (c) {
                        atomicMax(rar_max + row_base[m] + row, c);
                        if (in_lds) bin = m * COV_RAR_CLASSES + c;
                        else atomicAdd(rar_cnt + (size_t)m * COV_RAR_CLASSES + c, 1ull);
                    }
                }
            }
        }
        if (in_lds) cov_bin_add(s_bin, nbins, bin);
    }
    __syncthreads();
    for (uint32_t b = threadIdx.x; b < nbins; b += 256u)
        if (s_bin[b]) atomicAdd(rar_cnt + b, s_bin[b]);
}

// pairs first .. first + n - 1 of the target, binned by class into pair_cnt[COV_RAR_CLASSES]
__global__ void __launch_bounds__(256) covacc_rar_pairs(unsigned long long first, uint64_t n, cov_rar rf, unsigned long long *__restrict__ pair_cnt)
{
    __shared__ unsigned long long s_bin[COV_RAR_CLASSES];
    if (threadIdx.x < COV_RAR_CLASSES) s_bin[threadIdx.x] = 0ull;
    __syncthreads();
    const uint64_t stride = (uint64_t)gridDim.x * 256u;
    for (uint64_t i0 = (uint64_t)blockIdx.x * 256u; i0 < n; i0 += stride) {
        const uint64_t i = i0 + threadIdx.x;
        uint32_t bin = 0xFFFFFFFFu;
        if (i < n) { const uint32_t c = cov_rar_class(rf, first + i); if (c) bin = c; }
        cov_bin_add(s_bin, COV_RAR_CLASSES, bin);
    }
    __syncthreads();
    if (threadIdx.x < COV_RAR_CLASSES && s_bin[threadIdx.x]) atomicAdd(pair_cnt + threadIdx.x, s_bin[threadIdx.x]);
}

// host-replayed entries of one member, unfiltered, each with its pair's total and its pair's ordinal: the classification only
// (covacc_rows_hits in front of it has the counters); rar_max is the member's, rar_cnt its COV_RAR_CLASSES bins
__global__ void __launch_bounds__(256) covacc_rows_rar(const uint32_t *__restrict__ rows, const uint32_t *__restrict__ totals,
                                                       const unsigned long long *__restrict__ pairs, uint64_t n, uint32_t nrows,
                                                       long long min_hits, cov_rar rf, uint32_t *__restrict__ rar_max,
                                                       unsigned long long *__restrict__ rar_cnt)
{
    __shared__ unsigned long long s_bin[COV_RAR_CLASSES];
    if (threadIdx.x < COV_RAR_CLASSES) s_bin[threadIdx.x] = 0ull;
    __syncthreads();
    const uint64_t stride = (uint64_t)gridDim.x * 256u;
    for (uint64_t i0 = (uint64_t)blockIdx.x * 256u; i0 < n; i0 += stride) {
        const uint64_t i = i0 + threadIdx.x;
        uint32_t bin = 0xFFFFFFFFu;
        if (i < n && rows[i] < nrows && (long long)totals[i] > min_hits) {
            const uint32_t c = cov_rar_class(rf, pairs[i]);
            if (c) { atomicMax(rar_max + rows[i], c); bin = c; }
        }
        cov_bin_add(s_bin, COV_RAR_CLASSES, bin);
    }
    __syncthreads();
    if (threadIdx.x < COV_RAR_CLASSES && s_bin[threadIdx.x]) atomicAdd(rar_cnt + threadIdx.x, s_bin[threadIdx.x]);
}

struct sk_covacc {
    sk_ctx *ctx; int device;
    hipStream_t stream;
    uint32_t nm; long long min_hits;
    std::vector<uint32_t> nrows; std::vector<uint64_t> base;
    uint64_t total_rows; uint32_t max_rows;
    uint32_t *d_depth; uint64_t *d_base; uint32_t *d_nrows; unsigned long long *d_out;
    uint32_t *d_tot; size_t tot_cap;                        // all zero between folds
    uint32_t *d_rows; size_t rows_cap;                      // sk_covacc_add_rows' upload
    uint32_t *h_bad, *d_bad;                                // page-locked: a log entry that named no row
    // the held launch (sk_covacc_hold)
    void *h_recs, *h_hits, *h_rs; size_t h_recs_cap, h_hits_cap, h_rs_cap;
    bool held; cov_side hs; uint32_t held_members;
    bool hold_kept;                                         // the buffers still hold the launch last held (sk_covacc_fetch_hold, pick)
    void *p_recs, *p_hits; uint32_t *p_cnt; size_t p_recs_cap, p_hits_cap, p_cnt_cap;   // sk_covacc_pick's landing area
    // the fold by region: nothing of it exists until sk_covacc_set_regions or sk_covacc_finish_target_regions is called
    std::vector<uint32_t> nreg; std::vector<uint64_t> reg_base; uint64_t total_bins;
    uint32_t *d_region;                                     // [total_rows] each row's region
    uint32_t *d_nreg; uint64_t *d_reg_base;                 // [nm]
    void *d_reg_out; size_t reg_out_cap;                    // [total_bins] pairs
    void *d_fp, *d_starts; size_t fp_cap, starts_cap;       // set_regions' scratch: first positions (region_rows: the type column), region starts
    // the depth spectrum: off (spec_d = 0) until sk_covacc_set_spectrum
    uint32_t spec_d; void *d_spec; size_t spec_cap;         // [nm x (spec_d + 1)] bins, then [nm] deep sums
    // device time of the folds and of the targets' sweeps, kept only when somebody asked (sk_covacc_timing_)
    bool timed; hipEvent_t ev0, ev1; double ms_fold, ms_sweep, ms_mark;
    // recurrence: nothing of it exists until sk_covacc_set_recurrence is called
    uint32_t *d_irank;                                      // [total_rows] each row's bit of its member's planes, 0xFFFFFFFF: none
    std::vector<uint32_t> rec_nbits; uint32_t *d_rec_nbits; // [nm] informative rows per member (0: never set)
    void *d_blk; size_t blk_cap;                            // set_recurrence's scratch: the blocks' counts
    unsigned long long *d_stray;
    // thresholds: nothing of it exists until sk_covacc_set_thresholds is called with a list
    cov_thr thr;                                            // thr.n = 0: off
    uint32_t *d_thr_max;                                    // [total_rows] each row's highest class since the last finish
    unsigned long long *d_thr_cnt;                          // [nm x COV_THR_CLASSES] entries per class, then as many: rows per class
    uint32_t *d_tots; size_t tots_cap;                      // sk_covacc_add_rows_hits' upload of the totals
    bool thr_dirty; double ms_thr;                          // something was classified since the last finish; the finishing passes' device time
    // the scrub sweep: nothing of it exists until sk_covacc_set_classes is called with classes
    uint8_t *d_cls;                                         // [total_rows] each row's class, 0: in no set
    std::vector<uint32_t> ncls; uint32_t *d_ncls;           // [nm] the member's number of fractions (0: off)
    uint8_t *d_cls_up; size_t cls_up_cap;                   // set_classes' upload of the sparse list's classes
    unsigned long long *d_cls_out;                          // [nm x SK_SCRUB_SWEEP_MAX] pairs, then the stray count
    double ms_cls;                                          // the class passes' device time
    // support: nothing of it exists until sk_covacc_set_support switches it on
    bool sup_on;
    uint32_t *d_sinf; size_t sinf_cap;                      // [pairs x members] summed informative tallies; all zero between folds
    unsigned long long *d_sword; size_t sword_cap;          // [pairs] PE1 members | PE2 members << 32; all zero between folds
    unsigned long long *d_sup; size_t sup_cells;            // the target's accumulators (covacc_take has the layout); zero after a finish
    hipEvent_t ev2, ev3; bool sup_timed; double ms_take, ms_supfin;   // the takes' and the finishes' device time
    // rarefaction: nothing of it exists until sk_covacc_set_rarefaction is called with a list
    cov_rar rar;                                            // rar.n = 0: off
    unsigned long long pair_base;                           // the ordinal of pair 0 of the next sk_covacc_add's run
    uint32_t *d_rar_max;                                    // [total_rows] each row's highest class since the last finish
    unsigned long long *d_rar_cnt;                          // [nm x COV_RAR_CLASSES] lines per class, as many: rows per class, then [COV_RAR_CLASSES] pairs
    unsigned long long *d_pairs; size_t pairs_cap;          // sk_covacc_add_rows_hits_pairs' upload of the ordinals
    bool rar_dirty;                                         // something was classified or counted since the last finish
    hipEvent_t ev4, ev5; bool rar_timed; double ms_rar, ms_rarfin;    // the classifying passes' and the finishing passes' device time
};

static void cov_t0(sk_covacc *a) { if (a->timed) (void)hipEventRecord(a->ev0, a->stream); }
static void cov_t1(sk_covacc *a, double *sum)
{
    float ms = 0.f;
    if (!a->timed) return;
    if (hipEventRecord(a->ev1, a->stream) == hipSuccess && hipEventSynchronize(a->ev1) == hipSuccess &&
        hipEventElapsedTime(&ms, a->ev0, a->ev1) == hipSuccess) *sum += (double)ms;
}
// on != 0 starts the clocks (events around every fold and every sweep from here on); ms_fold / ms_sweep (NULL: not wanted): the sums so far
extern "C" int sk_covacc_timing_(sk_covacc *a, int on, double *ms_fold, double *ms_sweep)
{
    if (!a) return SK_E_ARG;
    if (on && !a->timed) {
        if (hipSetDevice(a->device) != hipSuccess || hipEventCreate(&a->ev0) != hipSuccess) return SK_E_HIP;
        if (hipEventCreate(&a->ev1) != hipSuccess) { (void)hipEventDestroy(a->ev0); return SK_E_HIP; }
        a->timed = true;
    }
    if (ms_fold) *ms_fold = a->ms_fold;
    if (ms_sweep) *ms_sweep = a->ms_sweep;
    return SK_OK;
}
extern "C" int sk_covacc_mark_timing_(sk_covacc *a, double *ms_mark)
{
    if (!a || !ms_mark) return SK_E_ARG;
    *ms_mark = a->ms_mark;
    return SK_OK;
}
extern "C" int sk_covacc_thresholds_timing_(sk_covacc *a, double *ms_thr)
{
    if (!a || !ms_thr) return SK_E_ARG;
    *ms_thr = a->ms_thr;
    return SK_OK;
}

extern "C" int sk_covacc_classes_timing_(sk_covacc *a, double *ms_cls)
{
    if (!a || !ms_cls) return SK_E_ARG;
    *ms_cls = a->ms_cls;
    return SK_OK;
}

// ms_take: the takes' device time inside the folds (the mark rides in the fold's scatter and is part of ms_fold only); ms_finish: the
// copies home.  Both are kept only while sk_covacc_timing_ is on.
extern "C" int sk_covacc_support_timing_(sk_covacc *a, double *ms_take, double *ms_finish)
{
    if (!a || !ms_take || !ms_finish) return SK_E_ARG;
    *ms_take = a->ms_take; *ms_finish = a->ms_supfin;
    return SK_OK;
}

// ms_class: the classifying passes' device time inside the folds (pair counts included); ms_finish: the finishing passes'.  Both
// are kept only while sk_covacc_timing_ is on.
extern "C" int sk_covacc_rarefaction_timing_(sk_covacc *a, double *ms_class, double *ms_finish)
{
    if (!a || !ms_class || !ms_finish) return SK_E_ARG;
    *ms_class = a->ms_rar; *ms_finish = a->ms_rarfin;
    return SK_OK;
}

#define CA_HIP(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return sk_fail_(a->ctx, SK_E_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); } while (0)

static unsigned cov_grid(uint64_t n) { const uint64_t g = (n + 255u) / 256u; return (unsigned)(g < 1u ? 1u : g > 4096u ? 4096u : g); }

static int cov_room(sk_covacc *a, void **p, size_t *cap, size_t need, bool zeroed)
{
    if (need <= *cap) return SK_OK;
    if (*p) { CA_HIP(hipStreamSynchronize(a->stream)); (void)hipFree(*p); *p = NULL; *cap = 0; }
    const size_t want = need + need / 4 + 4096;
    CA_HIP(hipMalloc(p, want));
    if (zeroed) CA_HIP(hipMemsetAsync(*p, 0, want, a->stream));
    *cap = want;
    return SK_OK;
}

extern "C" void sk_covacc_destroy(sk_covacc *a)
{
    if (!a) return;
    (void)hipSetDevice(a->device);
    if (a->stream) (void)hipStreamSynchronize(a->stream);
    (void)hipFree(a->d_depth); (void)hipFree(a->d_base); (void)hipFree(a->d_nrows); (void)hipFree(a->d_out);
    (void)hipFree(a->d_tot); (void)hipFree(a->d_rows); (void)hipFree(a->h_recs); (void)hipFree(a->h_hits); (void)hipFree(a->h_rs);
    (void)hipFree(a->p_recs); (void)hipFree(a->p_hits); (void)hipFree(a->p_cnt);
    (void)hipFree(a->d_region); (void)hipFree(a->d_nreg); (void)hipFree(a->d_reg_base); (void)hipFree(a->d_reg_out);
    (void)hipFree(a->d_fp); (void)hipFree(a->d_starts); (void)hipFree(a->d_spec);
    (void)hipFree(a->d_irank); (void)hipFree(a->d_rec_nbits); (void)hipFree(a->d_blk); (void)hipFree(a->d_stray);
    (void)hipFree(a->d_thr_max); (void)hipFree(a->d_thr_cnt); (void)hipFree(a->d_tots);
    (void)hipFree(a->d_cls); (void)hipFree(a->d_ncls); (void)hipFree(a->d_cls_up); (void)hipFree(a->d_cls_out);
    (void)hipFree(a->d_sinf); (void)hipFree(a->d_sword); (void)hipFree(a->d_sup);
    (void)hipFree(a->d_rar_max); (void)hipFree(a->d_rar_cnt); (void)hipFree(a->d_pairs);
    if (a->rar_timed) { (void)hipEventDestroy(a->ev4); (void)hipEventDestroy(a->ev5); }
    if (a->sup_timed) { (void)hipEventDestroy(a->ev2); (void)hipEventDestroy(a->ev3); }
    if (a->timed) { (void)hipEventDestroy(a->ev0); (void)hipEventDestroy(a->ev1); }
    if (a->h_bad) (void)hipHostFree(a->h_bad);
    if (a->stream) (void)hipStreamDestroy(a->stream);
    delete a;
}

static int cov_create_steps(sk_covacc *a)
{
    CA_HIP(hipSetDevice(a->device));
    CA_HIP(hipStreamCreateWithFlags(&a->stream, hipStreamNonBlocking));
    CA_HIP(hipMalloc((void **)&a->d_depth, (size_t)(a->total_rows ? a->total_rows : 1u) * 4u));
    CA_HIP(hipMalloc((void **)&a->d_base, (size_t)a->nm * 8u));
    CA_HIP(hipMalloc((void **)&a->d_nrows, (size_t)a->nm * 4u));
    CA_HIP(hipMalloc((void **)&a->d_out, (size_t)a->nm * 16u));
    CA_HIP(hipHostMalloc((void **)&a->h_bad, 64, hipHostMallocDefault));
    *a->h_bad = 0u;
    CA_HIP(hipHostGetDevicePointer((void **)&a->d_bad, a->h_bad, 0));
    CA_HIP(hipMemsetAsync(a->d_depth, 0, (size_t)(a->total_rows ? a->total_rows : 1u) * 4u, a->stream));
    CA_HIP(hipMemcpyAsync(a->d_base, a->base.data(), (size_t)a->nm * 8u, hipMemcpyHostToDevice, a->stream));
    CA_HIP(hipMemcpyAsync(a->d_nrows, a->nrows.data(), (size_t)a->nm * 4u, hipMemcpyHostToDevice, a->stream));
    CA_HIP(hipStreamSynchronize(a->stream));
    return SK_OK;
}

extern "C" int sk_covacc_create(sk_ctx *ctx, uint32_t nmembers, const uint32_t *nrows, int64_t min_kmer_hits, sk_covacc **out)
{
    if (!ctx || !out || !nrows || nmembers < 1u || nmembers > 4096u) return SK_E_ARG;
    *out = NULL;
    sk_covacc *a = new (std::nothrow) sk_covacc();
    if (!a) return SK_E_NOMEM;
    a->ctx = ctx; a->device = sk_ctx_device_(ctx); a->nm = nmembers; a->min_hits = (long long)min_kmer_hits;
    a->nrows.assign(nrows, nrows + nmembers);
    a->base.resize(nmembers);
    for (uint32_t m = 0; m < nmembers; m++) {
        a->base[m] = a->total_rows;
        a->total_rows += nrows[m];
        if (nrows[m] > a->max_rows) a->max_rows = nrows[m];
    }
    const int rc = cov_create_steps(a);
    if (rc != SK_OK) { sk_covacc_destroy(a); return rc; }
    *out = a;
    return SK_OK;
}

// the held results of a launch as one side of a fold; `members` of the launch come back through *ns (1 for a single context)
static int cov_view(sk_covacc *a, sk_ctx *ctx, sk_union *u, cov_side *s, uint32_t *members)
{
    sk_tally_view v;
    if ((!ctx && !u) || (ctx && u)) return sk_fail_(a->ctx, SK_E_ARG, "name a context or a union");
    const int rc = sk_tally_view_(ctx, u, &v);
    if (rc != SK_OK) return sk_fail_(a->ctx, rc, "%s", sk_last_error(u ? sk_union_context(u) : ctx));
    if (v.device != a->device) return sk_fail_(a->ctx, SK_E_ARG, "the launch ran on another device");
    s->recs = v.d_recs; s->nrecs = v.nrecs; s->hits = v.d_hits; s->nhits = v.nhits; s->rec_start = v.d_rec_start; s->nrec = v.nrec;
    s->r0 = 0; s->step = 1;
    *members = v.members;
    return SK_OK;
}

extern "C" int sk_covacc_hold(sk_covacc *a, sk_ctx *ctx, sk_union *u)
{
    if (!a) return SK_E_ARG;
    cov_side s; uint32_t members = 0;
    int rc = cov_view(a, ctx, u, &s, &members);
    if (rc != SK_OK) return rc;
    CA_HIP(hipSetDevice(a->device));
    a->held = false; a->hold_kept = false;
    if ((rc = cov_room(a, &a->h_recs, &a->h_recs_cap, (size_t)s.nrecs * 12u + 16u, false)) != SK_OK) return rc;
    if ((rc = cov_room(a, &a->h_hits, &a->h_hits_cap, (size_t)s.nhits * sizeof(sk_hit) + 16u, false)) != SK_OK) return rc;
    if ((rc = cov_room(a, &a->h_rs, &a->h_rs_cap, (size_t)s.nrec * 4u + 16u, false)) != SK_OK) return rc;
    if (s.nrecs) CA_HIP(hipMemcpyAsync(a->h_recs, s.recs, (size_t)s.nrecs * 12u, hipMemcpyDeviceToDevice, a->stream));
    if (s.nhits) CA_HIP(hipMemcpyAsync(a->h_hits, s.hits, (size_t)s.nhits * sizeof(sk_hit), hipMemcpyDeviceToDevice, a->stream));
    CA_HIP(hipMemcpyAsync(a->h_rs, s.rec_start, (size_t)s.nrec * 4u, hipMemcpyDeviceToDevice, a->stream));
    CA_HIP(hipStreamSynchronize(a->stream));
    a->hs = s;
    a->hs.recs = (const uint32_t *)a->h_recs; a->hs.hits = (const sk_hit *)a->h_hits; a->hs.rec_start = (const uint32_t *)a->h_rs;
    a->held_members = members; a->held = true; a->hold_kept = true;
    return SK_OK;
}

// what sk_covacc_hold copied, brought home in the collect calls' form (a held launch whose mate's launch cannot be folded after all)
extern "C" int sk_covacc_fetch_hold(sk_covacc *a, sk_tally_rec *out, uint64_t cap, uint64_t *n, sk_hit *out_hits, uint64_t hits_cap,
                                    uint64_t *out_nhits)
{
    if (!a || !n || !out_nhits) return SK_E_ARG;
    if (!a->hold_kept) return sk_fail_(a->ctx, SK_E_STATE, "no launch held (sk_covacc_hold)");
    *n = a->hs.nrecs; *out_nhits = a->hs.nhits;
    if (a->hs.nrecs > cap || a->hs.nhits > hits_cap) return SK_OK;       // (the counts say how much room it takes)
    if ((a->hs.nrecs && !out) || (a->hs.nhits && !out_hits)) return SK_E_ARG;
    CA_HIP(hipSetDevice(a->device));
    if (a->hs.nrecs) CA_HIP(hipMemcpy(out, a->hs.recs, (size_t)a->hs.nrecs * 12u, hipMemcpyDeviceToHost));
    if (a->hs.nhits) CA_HIP(hipMemcpy(out_hits, a->hs.hits, (size_t)a->hs.nhits * sizeof(sk_hit), hipMemcpyDeviceToHost));
    return SK_OK;
}

extern "C" int sk_covacc_pick(sk_covacc *a, sk_ctx *ctx, sk_union *u, int from_hold, int first, uint32_t ntail,
                              sk_tally_rec *out, uint64_t cap, uint64_t *n, sk_hit *out_hits, uint64_t hits_cap, uint64_t *out_nhits)
{
    if (!a || !n || !out_nhits || (cap && !out) || (hits_cap && !out_hits) || cap > 0x7FFFFFFFu || hits_cap > 0x7FFFFFFFu) return SK_E_ARG;
    cov_side s; uint32_t members = 0;
    int rc;
    if (from_hold) {
        if (!a->hold_kept) return sk_fail_(a->ctx, SK_E_STATE, "no launch held (sk_covacc_hold)");
        s = a->hs; members = a->held_members;
    } else if ((rc = cov_view(a, ctx, u, &s, &members)) != SK_OK) return rc;
    *n = 0; *out_nhits = 0;
    if (!s.nrec || !(s.nrecs + s.nhits)) return SK_OK;
    CA_HIP(hipSetDevice(a->device));
    if ((rc = cov_room(a, &a->p_recs, &a->p_recs_cap, (size_t)cap * 12u + 16u, false)) != SK_OK) return rc;
    if ((rc = cov_room(a, &a->p_hits, &a->p_hits_cap, (size_t)hits_cap * sizeof(sk_hit) + 16u, false)) != SK_OK) return rc;
    if ((rc = cov_room(a, (void **)&a->p_cnt, &a->p_cnt_cap, 8u, false)) != SK_OK) return rc;
    CA_HIP(hipMemsetAsync(a->p_cnt, 0, 8u, a->stream));
    hipLaunchKernelGGL(covacc_pick, dim3(cov_grid(s.nrecs + s.nhits)), dim3(256), 0, a->stream, s.recs, s.nrecs, s.hits, s.nhits,
                       s.rec_start, s.nrec, members ? members : 1u, first, ntail < s.nrec ? s.nrec - ntail : 0u,
                       (uint32_t *)a->p_recs, (uint32_t)cap, (sk_hit *)a->p_hits, (uint32_t)hits_cap, a->p_cnt);
    CA_HIP(hipGetLastError());
    uint32_t cnt[2];
    CA_HIP(hipMemcpyAsync(cnt, a->p_cnt, 8u, hipMemcpyDeviceToHost, a->stream));
    CA_HIP(hipStreamSynchronize(a->stream));
    *n = cnt[0]; *out_nhits = cnt[1];
    if (cnt[0] > cap || cnt[1] > hits_cap) return SK_OK;                  // (the counts say how much room it takes: pick again)
    if (cnt[0]) CA_HIP(hipMemcpy(out, a->p_recs, (size_t)cnt[0] * 12u, hipMemcpyDeviceToHost));
    if (cnt[1]) CA_HIP(hipMemcpy(out_hits, a->p_hits, (size_t)cnt[1] * sizeof(sk_hit), hipMemcpyDeviceToHost));
    return SK_OK;
}

extern "C" int sk_covacc_add(sk_covacc *a, sk_ctx *ctx, sk_union *u, uint32_t member0, uint32_t a0, uint32_t astep, uint32_t npairs,
                             const sk_covacc_mate *mate)
{
    if (!a) return SK_E_ARG;
    cov_side side[2]; uint32_t members = 0, nsides = 1;
    int rc = cov_view(a, ctx, u, &side[0], &members);
    if (rc != SK_OK) return rc;
    const uint32_t ns = members ? members : 1u;
    if (member0 >= a->nm || ns > a->nm - member0) return sk_fail_(a->ctx, SK_E_ARG, "members %u..%u: the accumulator has %u", member0, member0 + ns - 1u, a->nm);
    if (!npairs) return SK_OK;
    side[0].r0 = a0; side[0].step = astep;
    if (mate) {
        if (mate->held) {
            if (!a->held) return sk_fail_(a->ctx, SK_E_STATE, "no launch held (sk_covacc_hold)");
            if (a->held_members != members) return sk_fail_(a->ctx, SK_E_ARG, "the held launch had other members");
            side[1] = a->hs;
        } else side[1] = side[0];
        side[1].r0 = mate->b0; side[1].step = mate->bstep;
        nsides = 2;
    }
    for (uint32_t k = 0; k < nsides; k++)
        if (!side[k].step || !side[k].nrec || side[k].r0 >= side[k].nrec ||
            (uint64_t)side[k].r0 + (uint64_t)(npairs - 1u) * side[k].step >= side[k].nrec)
            return sk_fail_(a->ctx, SK_E_ARG, "the run leaves the batch (records %u + %u x %u of %u)", side[k].r0, npairs, side[k].step, side[k].nrec);
    if ((uint64_t)npairs * ns > 0x3FFFFFF0ull) return sk_fail_(a->ctx, SK_E_ARG, "too many pairs x members");
    CA_HIP(hipSetDevice(a->device));
    if ((rc = cov_room(a, (void **)&a->d_tot, &a->tot_cap, (size_t)npairs * ns * 4u, true)) != SK_OK) return rc;
    const bool sup = a->sup_on;
    if (sup) {
        if (ns > COV_SUP_M) return sk_fail_(a->ctx, SK_E_ARG, "support is on: a launch of %u members, at most %u", ns, COV_SUP_M);
        if ((rc = cov_room(a, (void **)&a->d_sinf, &a->sinf_cap, (size_t)npairs * ns * 4u, true)) != SK_OK) return rc;
        if ((rc = cov_room(a, (void **)&a->d_sword, &a->sword_cap, (size_t)npairs * 8u, true)) != SK_OK) return rc;
        if (a->timed && !a->sup_timed) {
            CA_HIP(hipEventCreate(&a->ev2));
            if (hipEventCreate(&a->ev3) != hipSuccess) { (void)hipEventDestroy(a->ev2); return sk_fail_(a->ctx, SK_E_HIP, "no event for the take"); }
            a->sup_timed = true;
        }
    }
    const bool rar = a->rar.n != 0u;
    if (rar && a->timed && !a->rar_timed) {
        CA_HIP(hipEventCreate(&a->ev4));
        if (hipEventCreate(&a->ev5) != hipSuccess) { (void)hipEventDestroy(a->ev4); return sk_fail_(a->ctx, SK_E_HIP, "no event for the classifying pass"); }
        a->rar_timed = true;
    }
    cov_t0(a);
    for (int clear = 0; clear < 2; clear++) {
        for (uint32_t k = 0; k < nsides; k++)
            if (side[k].nrecs && sup)
                hipLaunchKernelGGL(covacc_scatter_sup, dim3(cov_grid(side[k].nrecs)), dim3(256), 0, a->stream, side[k].recs, side[k].nrecs, ns,
                                   side[k].nrec, side[k].r0, side[k].step, npairs, a->d_tot, a->d_sinf, a->d_sword, k, clear);
            else if (side[k].nrecs)
                hipLaunchKernelGGL(covacc_scatter, dim3(cov_grid(side[k].nrecs)), dim3(256), 0, a->stream, side[k].recs, side[k].nrecs, ns,
                                   side[k].nrec, side[k].r0, side[k].step, npairs, a->d_tot, clear);
        if (sup && !clear) {                                  // the take: behind every side's marks, in front of the clearing scatter
            if (a->sup_timed) (void)hipEventRecord(a->ev2, a->stream);
            for (uint32_t k = 0; k < nsides; k++)
                if (side[k].nrecs) {
                    const unsigned g = cov_grid(side[k].nrecs);
                    hipLaunchKernelGGL(covacc_take, dim3(g > 256u ? 256u : g), dim3(256), 0, a->stream, side[k].recs, side[k].nrecs, ns,
                                       side[k].nrec, side[k].r0, side[k].step, npairs, (const uint32_t *)a->d_tot,
                                       (const uint32_t *)a->d_sinf, a->d_sword, a->min_hits, member0, a->nm, a->d_sup);
                }
            if (a->sup_timed) (void)hipEventRecord(a->ev3, a->stream);
        }
        for (uint32_t k = 0; k < nsides && !clear; k++)
            if (side[k].nhits && a->thr.n) {                  // (thresholds: the same fold, every entry classified as well)
                hipLaunchKernelGGL(covacc_hits_thr, dim3(cov_grid(side[k].nhits)), dim3(256), 0, a->stream, side[k].hits, side[k].nhits,
                                   side[k].rec_start, side[k].nrec, ns, members ? 1 : 0, side[k].r0, side[k].step, npairs,
                                   (const uint32_t *)a->d_tot, a->min_hits, a->d_depth, (const uint64_t *)a->d_base + member0,
                                   (const uint32_t *)a->d_nrows + member0, a->d_bad, a->thr, a->d_thr_max,
                                   a->d_thr_cnt + (size_t)member0 * COV_THR_CLASSES);
                a->thr_dirty = true;
            } else if (side[k].nhits)
                hipLaunchKernelGGL(covacc_hits, dim3(cov_grid(side[k].nhits)), dim3(256), 0, a->stream, side[k].hits, side[k].nhits,
                                   side[k].rec_start, side[k].nrec, ns, members ? 1 : 0, side[k].r0, side[k].step, npairs,
                                   (const uint32_t *)a->d_tot, a->min_hits, a->d_depth, (const uint64_t *)a->d_base + member0,
                                   (const uint32_t *)a->d_nrows + member0, a->d_bad);
        if (rar && !clear) {                                  // the classifying pass: behind the scatters, in front of the clearing ones
            if (a->rar_timed) (void)hipEventRecord(a->ev4, a->stream);
            for (uint32_t k = 0; k < nsides; k++)
                if (side[k].nhits)
                    hipLaunchKernelGGL(covacc_rar_hits, dim3(cov_grid(side[k].nhits)), dim3(256), 0, a->stream, side[k].hits, side[k].nhits,
                                       side[k].rec_start, side[k].nrec, ns, members ? 1 : 0, side[k].r0, side[k].step, npairs,
                                       (const uint32_t *)a->d_tot, a->min_hits, (const uint64_t *)a->d_base + member0,
                                       (const uint32_t *)a->d_nrows + member0, a->rar, a->pair_base, a->d_rar_max,
                                       a->d_rar_cnt + (size_t)member0 * COV_RAR_CLASSES);
            {   // the run's pairs, once per run
                const unsigned g = cov_grid(npairs);
                hipLaunchKernelGGL(covacc_rar_pairs, dim3(g > 256u ? 256u : g), dim3(256), 0, a->stream, a->pair_base, (uint64_t)npairs,
                                   a->rar, a->d_rar_cnt + (size_t)a->nm * COV_RAR_CLASSES * 2u);
            }
            if (a->rar_timed) (void)hipEventRecord(a->ev5, a->stream);
            a->rar_dirty = true;
        }
    }
    {   // a fold that fails half way leaves tot[] (and support's cells and words) as they must be between folds: all zero
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(a->stream);
        if (e != hipSuccess) {
            (void)hipMemset(a->d_tot, 0, a->tot_cap);
            if (a->d_sinf) (void)hipMemset(a->d_sinf, 0, a->sinf_cap);
            if (a->d_sword) (void)hipMemset(a->d_sword, 0, a->sword_cap);
            return sk_fail_(a->ctx, SK_E_HIP, "the fold failed: %s", hipGetErrorString(e));
        }
    }
    cov_t1(a, &a->ms_fold);
    if (sup && a->sup_timed) { float ms = 0.f; if (hipEventElapsedTime(&ms, a->ev2, a->ev3) == hipSuccess) a->ms_take += (double)ms; }
    if (rar && a->rar_timed) { float ms = 0.f; if (hipEventElapsedTime(&ms, a->ev4, a->ev5) == hipSuccess) a->ms_rar += (double)ms; }
    if (mate && mate->held) a->held = false;
    if (*(volatile uint32_t *)a->h_bad) { *a->h_bad = 0u; return sk_fail_(a->ctx, SK_E_STATE, "a hit log entry names no row of its member"); }
    return SK_OK;
}

// ---- support ----
extern "C" int sk_covacc_set_support(sk_covacc *a, int on)
{
    if (!a) return SK_E_ARG;
    if (on && !a->d_sup) {
        if (a->nm > SK_COVACC_SUPPORT_MEMBERS_MAX) return sk_fail_(a->ctx, SK_E_ARG, "support: %u members, at most %u", a->nm, SK_COVACC_SUPPORT_MEMBERS_MAX);
        CA_HIP(hipSetDevice(a->device));
        const size_t cells = (size_t)a->nm * 3u + (size_t)a->nm * a->nm * 2u;
        unsigned long long *p = NULL;
        CA_HIP(hipMalloc((void **)&p, cells * 8u));
        if (hipMemsetAsync(p, 0, cells * 8u, a->stream) != hipSuccess || hipStreamSynchronize(a->stream) != hipSuccess) {
            (void)hipFree(p);
            return sk_fail_(a->ctx, SK_E_HIP, "no room for the support accumulators");
        }
        a->d_sup = p; a->sup_cells = cells;
    }
    a->sup_on = on != 0;
    return SK_OK;
}

extern "C" int sk_covacc_finish_target_support(sk_covacc *a, uint64_t *out_pairs, uint64_t *out_lines, uint64_t *out_both,
                                               uint64_t *out_shared, uint64_t *out_lines_a)
{
    if (!a || !out_pairs || !out_lines || !out_both || !out_shared || !out_lines_a) return SK_E_ARG;
    if (!a->sup_on) return sk_fail_(a->ctx, SK_E_STATE, "support is off (sk_covacc_set_support)");
    CA_HIP(hipSetDevice(a->device));
    std::vector<unsigned long long> h(a->sup_cells);
    cov_t0(a);
    CA_HIP(hipMemcpyAsync(h.data(), a->d_sup, a->sup_cells * 8u, hipMemcpyDeviceToHost, a->stream));
    CA_HIP(hipMemsetAsync(a->d_sup, 0, a->sup_cells * 8u, a->stream));
    CA_HIP(hipStreamSynchronize(a->stream));
    cov_t1(a, &a->ms_supfin);
    const size_t nn = (size_t)a->nm * a->nm;
    for (uint32_t m = 0; m < a->nm; m++) { out_pairs[m] = h[3u * m]; out_lines[m] = h[3u * m + 1u]; out_both[m] = h[3u * m + 2u]; }
    for (size_t c = 0; c < nn; c++) { out_shared[c] = h[(size_t)a->nm * 3u + c]; out_lines_a[c] = h[(size_t)a->nm * 3u + nn + c]; }
    return SK_OK;
}

extern "C" int sk_covacc_add_rows(sk_covacc *a, uint32_t member, const uint32_t *rows, uint64_t n)
{
    if (!a || (n && !rows)) return SK_E_ARG;
    if (member >= a->nm) return sk_fail_(a->ctx, SK_E_ARG, "member %u: the accumulator has %u", member, a->nm);
    if (a->thr.n) return sk_fail_(a->ctx, SK_E_STATE, "thresholds are on: filtered rows carry no totals (sk_covacc_add_rows_hits)");
    if (!n) return SK_OK;
    for (uint64_t i = 0; i < n; i++)
        if (rows[i] >= a->nrows[member]) return sk_fail_(a->ctx, SK_E_ARG, "row %u: member %u has %u", rows[i], member, a->nrows[member]);
    CA_HIP(hipSetDevice(a->device));
    const int rc = cov_room(a, (void **)&a->d_rows, &a->rows_cap, (size_t)n * 4u, false);
    if (rc != SK_OK) return rc;
    cov_t0(a);
    CA_HIP(hipMemcpyAsync(a->d_rows, rows, (size_t)n * 4u, hipMemcpyHostToDevice, a->stream));
    hipLaunchKernelGGL(covacc_rows, dim3(cov_grid(n)), dim3(256), 0, a->stream, (const uint32_t *)a->d_rows, n, a->nrows[member],
                       a->d_depth + a->base[member]);
    CA_HIP(hipGetLastError());
    CA_HIP(hipStreamSynchronize(a->stream));
    cov_t1(a, &a->ms_fold);
    return SK_OK;
}

extern "C" int sk_covacc_add_rows_hits(sk_covacc *a, uint32_t member, const uint32_t *rows, const uint32_t *total_hits, uint64_t n)
{
    if (!a || (n && (!rows || !total_hits))) return SK_E_ARG;
    if (member >= a->nm) return sk_fail_(a->ctx, SK_E_ARG, "member %u: the accumulator has %u", member, a->nm);
    if (!n) return SK_OK;
    for (uint64_t i = 0; i < n; i++)
        if (rows[i] >= a->nrows[member]) return sk_fail_(a->ctx, SK_E_ARG, "row %u: member %u has %u", rows[i], member, a->nrows[member]);
    CA_HIP(hipSetDevice(a->device));
    int rc = cov_room(a, (void **)&a->d_rows, &a->rows_cap, (size_t)n * 4u, false);
    if (rc == SK_OK) rc = cov_room(a, (void **)&a->d_tots, &a->tots_cap, (size_t)n * 4u, false);
    if (rc != SK_OK) return rc;
    cov_t0(a);
    CA_HIP(hipMemcpyAsync(a->d_rows, rows, (size_t)n * 4u, hipMemcpyHostToDevice, a->stream));
    CA_HIP(hipMemcpyAsync(a->d_tots, total_hits, (size_t)n * 4u, hipMemcpyHostToDevice, a->stream));
    hipLaunchKernelGGL(covacc_rows_hits, dim3(cov_grid(n)), dim3(256), 0, a->stream, (const uint32_t *)a->d_rows, (const uint32_t *)a->d_tots, n,
                       a->nrows[member], a->min_hits, a->d_depth + a->base[member], a->thr,
                       a->thr.n ? a->d_thr_max + a->base[member] : (uint32_t *)NULL,
                       a->thr.n ? a->d_thr_cnt + (size_t)member * COV_THR_CLASSES : (unsigned long long *)NULL);
    CA_HIP(hipGetLastError());
    CA_HIP(hipStreamSynchronize(a->stream));
    cov_t1(a, &a->ms_fold);
    if (a->thr.n) a->thr_dirty = true;
    return SK_OK;
}

extern "C" int sk_covacc_finish_target(sk_covacc *a, uint64_t *out_unique, uint64_t *out_total)
{
    if (!a || !out_unique || !out_total) return SK_E_ARG;
    CA_HIP(hipSetDevice(a->device));
    std::vector<unsigned long long> h((size_t)a->nm * 2u);
    cov_t0(a);
    CA_HIP(hipMemsetAsync(a->d_out, 0, (size_t)a->nm * 16u, a->stream));
    unsigned gx = (a->max_rows + 255u) / 256u;
    gx = gx < 1u ? 1u : gx > 256u ? 256u : gx;
    hipLaunchKernelGGL(covacc_finish, dim3(gx, a->nm), dim3(256), 0, a->stream, a->d_depth, (const uint64_t *)a->d_base,
                       (const uint32_t *)a->d_nrows, a->d_out);
    CA_HIP(hipGetLastError());
    CA_HIP(hipMemcpyAsync(h.data(), a->d_out, (size_t)a->nm * 16u, hipMemcpyDeviceToHost, a->stream));
    CA_HIP(hipStreamSynchronize(a->stream));
    cov_t1(a, &a->ms_sweep);
    for (uint32_t m = 0; m < a->nm; m++) { out_unique[m] = h[2u * m]; out_total[m] = h[2u * m + 1u]; }
    return SK_OK;
}

extern "C" int sk_covacc_rows(sk_covacc *a, uint32_t member, uint32_t *out)
{
    if (!a || !out) return SK_E_ARG;
    if (member >= a->nm) return sk_fail_(a->ctx, SK_E_ARG, "member %u: the accumulator has %u", member, a->nm);
    CA_HIP(hipSetDevice(a->device));
    CA_HIP(hipStreamSynchronize(a->stream));
    if (a->nrows[member]) CA_HIP(hipMemcpy(out, a->d_depth + a->base[member], (size_t)a->nrows[member] * 4u, hipMemcpyDeviceToHost));
    return SK_OK;
}

// ---- the fold by region ----
// the regions' state on the device as the host's vectors have it: every member's region count and where its pairs begin
static int cov_regions_sync(sk_covacc *a)
{
    if (a->nreg.empty()) { a->nreg.assign(a->nm, 0u); a->reg_base.assign(a->nm, 0u); }
    a->total_bins = 0;
    for (uint32_t m = 0; m < a->nm; m++) { a->reg_base[m] = a->total_bins; a->total_bins += (uint64_t)a->nreg[m] + 1u; }
    if (!a->d_region) {                                   // all zero: a member whose regions were never set has one, "unplaced"
        const size_t bytes = (size_t)(a->total_rows ? a->total_rows : 1u) * 4u;
        CA_HIP(hipMalloc((void **)&a->d_region, bytes));
        CA_HIP(hipMemsetAsync(a->d_region, 0, bytes, a->stream));
        CA_HIP(hipMalloc((void **)&a->d_nreg, (size_t)a->nm * 4u));
        CA_HIP(hipMalloc((void **)&a->d_reg_base, (size_t)a->nm * 8u));
    }
    const int rc = cov_room(a, &a->d_reg_out, &a->reg_out_cap, (size_t)a->total_bins * 16u, false);
    if (rc != SK_OK) return rc;
    CA_HIP(hipMemcpyAsync(a->d_nreg, a->nreg.data(), (size_t)a->nm * 4u, hipMemcpyHostToDevice, a->stream));
    CA_HIP(hipMemcpyAsync(a->d_reg_base, a->reg_base.data(), (size_t)a->nm * 8u, hipMemcpyHostToDevice, a->stream));
    CA_HIP(hipStreamSynchronize(a->stream));
    return SK_OK;
}

static int cov_member_ctx(sk_covacc *a, uint32_t member, sk_ctx *ctx)
{
    if (member >= a->nm) return sk_fail_(a->ctx, SK_E_ARG, "member %u: the accumulator has %u", member, a->nm);
    if (sk_ctx_device_(ctx) != a->device) return sk_fail_(a->ctx, SK_E_ARG, "the table is on another device");
    if (sk_table_rows(ctx) != a->nrows[member]) return sk_fail_(a->ctx, SK_E_ARG, "member %u has %u rows, the table %u", member, a->nrows[member], sk_table_rows(ctx));
    return SK_OK;
}

extern "C" int sk_covacc_set_regions(sk_covacc *a, uint32_t member, sk_ctx *ctx, const uint32_t *region_start, uint32_t nregions)
{
    if (!a || !ctx || (nregions && !region_start)) return SK_E_ARG;
    int rc = cov_member_ctx(a, member, ctx);
    if (rc != SK_OK) return rc;
    if (nregions > SKH_REGIONS_MAX) return sk_fail_(a->ctx, SK_E_ARG, "%u regions: at most %u", nregions, SKH_REGIONS_MAX);
    for (uint32_t r = 1; r < nregions; r++)
        if (region_start[r] < region_start[r - 1]) return sk_fail_(a->ctx, SK_E_ARG, "region starts must ascend");
    CA_HIP(hipSetDevice(a->device));
    if (a->nreg.empty()) { a->nreg.assign(a->nm, 0u); a->reg_base.assign(a->nm, 0u); }
    const uint32_t before = a->nreg[member];
    a->nreg[member] = nregions;
    if ((rc = cov_regions_sync(a)) != SK_OK) { a->nreg[member] = before; return rc; }
    const uint32_t n = a->nrows[member];
    if (!n) return SK_OK;
    if ((rc = cov_room(a, &a->d_fp, &a->fp_cap, (size_t)n * 4u, false)) != SK_OK) return rc;
    if ((rc = cov_room(a, &a->d_starts, &a->starts_cap, (size_t)nregions * 4u + 4u, false)) != SK_OK) return rc;
    rc = sk_table_first_pos_to_device_(ctx, (uint32_t *)a->d_fp);         // (on the table's stream; complete on return)
    if (rc != SK_OK) return sk_fail_(a->ctx, rc, "%s", sk_last_error(ctx));
    if (nregions) CA_HIP(hipMemcpyAsync(a->d_starts, region_start, (size_t)nregions * 4u, hipMemcpyHostToDevice, a->stream));
    hipLaunchKernelGGL(covacc_map_regions, dim3(cov_grid(n)), dim3(256), 0, a->stream, (const uint32_t *)a->d_fp, n,
                       (const uint32_t *)a->d_starts, nregions, a->d_region + a->base[member]);
    CA_HIP(hipGetLastError());
    CA_HIP(hipStreamSynchronize(a->stream));
    return SK_OK;
}

extern "C" int sk_covacc_region_rows(sk_covacc *a, uint32_t member, sk_ctx *ctx, uint32_t type_col, uint32_t informative_value,
                                     uint64_t *out_rows, uint64_t *out_informative)
{
    if (!a || !ctx || !out_rows || !out_informative) return SK_E_ARG;
    int rc = cov_member_ctx(a, member, ctx);
    if (rc != SK_OK) return rc;
    CA_HIP(hipSetDevice(a->device));
    if (!a->d_region && (rc = cov_regions_sync(a)) != SK_OK) return rc;
    const uint32_t n = a->nrows[member], nb = a->nreg[member] + 1u;
    std::vector<unsigned long long> h((size_t)nb * 2u, 0ull);
    if (n) {
        if ((rc = cov_room(a, &a->d_fp, &a->fp_cap, (size_t)n * 4u, false)) != SK_OK) return rc;
        rc = sk_counts_rows_to_device_(ctx, type_col, (uint32_t *)a->d_fp);   // (the column in the caller's row order; complete on return)
        if (rc != SK_OK) return sk_fail_(a->ctx, rc, "%s", sk_last_error(ctx));
        unsigned long long *ro = (unsigned long long *)a->d_reg_out + 2ull * a->reg_base[member];
        CA_HIP(hipMemsetAsync(ro, 0, (size_t)nb * 16u, a->stream));
        unsigned gx = (n + 255u) / 256u;
        gx = gx > 256u ? 256u : gx;
        hipLaunchKernelGGL(covacc_region_rows, dim3(gx), dim3(256), 0, a->stream, (const uint32_t *)(a->d_region + a->base[member]), n,
                           (const uint32_t *)a->d_fp, informative_value, nb, ro);
        CA_HIP(hipGetLastError());
        CA_HIP(hipMemcpyAsync(h.data(), ro, (size_t)nb * 16u, hipMemcpyDeviceToHost, a->stream));
        CA_HIP(hipStreamSynchronize(a->stream));
    }
    for (uint32_t r = 0; r < nb; r++) { out_rows[r] = h[2u * r]; out_informative[r] = h[2u * r + 1u]; }
    return SK_OK;
}

extern "C" int sk_covacc_finish_target_regions(sk_covacc *a, uint64_t *out_unique, uint64_t *out_total, uint64_t *reg_unique, uint64_t *reg_total)
{
    if (!a || !out_unique || !out_total || !reg_unique || !reg_total) return SK_E_ARG;
    CA_HIP(hipSetDevice(a->device));
    int rc;
    if (!a->d_region && (rc = cov_regions_sync(a)) != SK_OK) return rc;
    std::vector<unsigned long long> h((size_t)a->nm * 2u), hr((size_t)a->total_bins * 2u);
    cov_t0(a);
    CA_HIP(hipMemsetAsync(a->d_out, 0, (size_t)a->nm * 16u, a->stream));
    CA_HIP(hipMemsetAsync(a->d_reg_out, 0, (size_t)a->total_bins * 16u, a->stream));
    unsigned gx = (a->max_rows + 255u) / 256u;
    gx = gx < 1u ? 1u : gx > 256u ? 256u : gx;
    hipLaunchKernelGGL(covacc_finish_regions, dim3(gx, a->nm), dim3(256), 0, a->stream, a->d_depth, (const uint64_t *)a->d_base,
                       (const uint32_t *)a->d_nrows, (const uint32_t *)a->d_region, (const uint32_t *)a->d_nreg,
                       (const uint64_t *)a->d_reg_base, a->d_out, (unsigned long long *)a->d_reg_out);
    CA_HIP(hipGetLastError());
    CA_HIP(hipMemcpyAsync(h.data(), a->d_out, (size_t)a->nm * 16u, hipMemcpyDeviceToHost, a->stream));
    CA_HIP(hipMemcpyAsync(hr.data(), a->d_reg_out, (size_t)a->total_bins * 16u, hipMemcpyDeviceToHost, a->stream));
    CA_HIP(hipStreamSynchronize(a->stream));
    cov_t1(a, &a->ms_sweep);
    for (uint32_t m = 0; m < a->nm; m++) { out_unique[m] = h[2u * m]; out_total[m] = h[2u * m + 1u]; }
    for (uint64_t r = 0; r < a->total_bins; r++) { reg_unique[r] = hr[2u * r]; reg_total[r] = hr[2u * r + 1u]; }
    return SK_OK;
}

// ---- the depth spectrum ----
extern "C" int sk_covacc_set_spectrum(sk_covacc *a, uint32_t max_depth)
{
    if (!a || max_depth > SK_COVACC_SPECTRUM_MAX) return SK_E_ARG;
    if (max_depth) {
        CA_HIP(hipSetDevice(a->device));
        const int rc = cov_room(a, &a->d_spec, &a->spec_cap, ((size_t)a->nm * (max_depth + 1u) + a->nm) * 8u, false);
        if (rc != SK_OK) return rc;
    }
    a->spec_d = max_depth;
    return SK_OK;
}

extern "C" int sk_covacc_finish_target_spectrum(sk_covacc *a, uint64_t *out_unique, uint64_t *out_total, uint64_t *spec, uint64_t *deep_total,
                                                uint64_t *reg_unique, uint64_t *reg_total)
{
    if (!a || !out_unique || !out_total || !spec || !deep_total || (!reg_unique) != (!reg_total)) return SK_E_ARG;
    if (!a->spec_d) return sk_fail_(a->ctx, SK_E_STATE, "the spectrum is off (sk_covacc_set_spectrum)");
    CA_HIP(hipSetDevice(a->device));
    const bool regions = reg_unique != NULL;
    int rc;
    if (regions && !a->d_region && (rc = cov_regions_sync(a)) != SK_OK) return rc;
    const size_t nspec = (size_t)a->nm * (a->spec_d + 1u), nall = nspec + a->nm;
    std::vector<unsigned long long> h((size_t)a->nm * 2u), hs(nall), hr(regions ? (size_t)a->total_bins * 2u : 0u);
    unsigned long long *d_spec = (unsigned long long *)a->d_spec;
    cov_t0(a);
    CA_HIP(hipMemsetAsync(a->d_out, 0, (size_t)a->nm * 16u, a->stream));
    CA_HIP(hipMemsetAsync(a->d_spec, 0, nall * 8u, a->stream));
    if (regions) CA_HIP(hipMemsetAsync(a->d_reg_out, 0, (size_t)a->total_bins * 16u, a->stream));
    unsigned gx = (a->max_rows + 255u) / 256u;
    gx = gx < 1u ? 1u : gx > 256u ? 256u : gx;
    if (regions)
        hipLaunchKernelGGL(covacc_finish_spectrum<true>, dim3(gx, a->nm), dim3(256), 0, a->stream, a->d_depth, (const uint64_t *)a->d_base,
                           (const uint32_t *)a->d_nrows, (const uint32_t *)a->d_region, (const uint32_t *)a->d_nreg,
                           (const uint64_t *)a->d_reg_base, a->d_out, (unsigned long long *)a->d_reg_out, a->spec_d, d_spec, d_spec + nspec);
    else
        hipLaunchKernelGGL(covacc_finish_spectrum<false>, dim3(gx, a->nm), dim3(256), 0, a->stream, a->d_depth, (const uint64_t *)a->d_base,
                           (const uint32_t *)a->d_nrows, (const uint32_t *)NULL, (const uint32_t *)NULL, (const uint64_t *)NULL, a->d_out,
                           (unsigned long long *)NULL, a->spec_d, d_spec, d_spec + nspec);
    CA_HIP(hipGetLastError());
    CA_HIP(hipMemcpyAsync(h.data(), a->d_out, (size_t)a->nm * 16u, hipMemcpyDeviceToHost, a->stream));
    CA_HIP(hipMemcpyAsync(hs.data(), a->d_spec, nall * 8u, hipMemcpyDeviceToHost, a->stream));
    if (regions && a->total_bins) CA_HIP(hipMemcpyAsync(hr.data(), a->d_reg_out, (size_t)a->total_bins * 16u, hipMemcpyDeviceToHost, a->stream));
    CA_HIP(hipStreamSynchronize(a->stream));
    cov_t1(a, &a->ms_sweep);
    for (uint32_t m = 0; m < a->nm; m++) { out_unique[m] = h[2u * m]; out_total[m] = h[2u * m + 1u]; deep_total[m] = hs[nspec + m]; }
    for (size_t i = 0; i < nspec; i++) spec[i] = hs[i];
    for (uint64_t r = 0; regions && r < a->total_bins; r++) { reg_unique[r] = hr[2u * r]; reg_total[r] = hr[2u * r + 1u]; }
    return SK_OK;
}

// ---- recurrence ----
extern "C" int sk_covacc_set_recurrence(sk_covacc *a, uint32_t member, sk_ctx *ctx, uint32_t type_col, uint32_t informative_value,
                                        uint32_t *out_informative)
{
    if (!a || !ctx || !out_informative) return SK_E_ARG;
    int rc = cov_member_ctx(a, member, ctx);
    if (rc != SK_OK) return rc;
    CA_HIP(hipSetDevice(a->device));
    if (!a->d_irank) {                                    // all ones: a member never set has no informative row
        const size_t bytes = (size_t)(a->total_rows ? a->total_rows : 1u) * 4u;
        uint32_t *p = NULL, *q = NULL; unsigned long long *st = NULL;
        CA_HIP(hipMalloc((void **)&p, bytes));
        if (hipMalloc((void **)&q, (size_t)a->nm * 4u) != hipSuccess || hipMalloc((void **)&st, 8u) != hipSuccess) {
            (void)hipFree(p); (void)hipFree(q);
            return sk_fail_(a->ctx, SK_E_HIP, "no room for the rank map");
        }
        a->d_irank = p; a->d_rec_nbits = q; a->d_stray = st;
        a->rec_nbits.assign(a->nm, 0u);
        CA_HIP(hipMemsetAsync(a->d_irank, 0xFF, bytes, a->stream));
        CA_HIP(hipMemsetAsync(a->d_rec_nbits, 0, (size_t)a->nm * 4u, a->stream));
    }
    const uint32_t n = a->nrows[member];
    uint32_t inf = 0;
    if (n) {
        const uint32_t nblk = (uint32_t)(((uint64_t)n + 255u) / 256u);
        if ((rc = cov_room(a, &a->d_fp, &a->fp_cap, (size_t)n * 4u, false)) != SK_OK) return rc;
        if ((rc = cov_room(a, &a->d_blk, &a->blk_cap, ((size_t)nblk + 1u) * 4u, false)) != SK_OK) return rc;
        rc = sk_counts_rows_to_device_(ctx, type_col, (uint32_t *)a->d_fp);   // (the column in the caller's row order; complete on return)
        if (rc != SK_OK) return sk_fail_(a->ctx, rc, "%s", sk_last_error(ctx));
        hipLaunchKernelGGL(covacc_rank_count, dim3(nblk), dim3(256), 0, a->stream, (const uint32_t *)a->d_fp, n, informative_value,
                           (uint32_t *)a->d_blk);
        hipLaunchKernelGGL(covacc_rank_scan, dim3(1), dim3(256), 0, a->stream, (uint32_t *)a->d_blk, nblk);
        hipLaunchKernelGGL(covacc_rank_write, dim3(nblk), dim3(256), 0, a->stream, (const uint32_t *)a->d_fp, n, informative_value,
                           (const uint32_t *)a->d_blk, a->d_irank + a->base[member]);
        CA_HIP(hipGetLastError());
        CA_HIP(hipMemcpyAsync(&inf, (uint32_t *)a->d_blk + nblk, 4u, hipMemcpyDeviceToHost, a->stream));
        CA_HIP(hipStreamSynchronize(a->stream));
    }
    a->rec_nbits[member] = inf;
    CA_HIP(hipMemcpy(a->d_rec_nbits + member, &inf, 4u, hipMemcpyHostToDevice));
    *out_informative = inf;
    return SK_OK;
}

extern "C" int sk_covacc_mark_target(sk_covacc *a, sk_recur *r, uint32_t sample, uint64_t *out_stray)
{
    if (!a || !r || !out_stray) return SK_E_ARG;
    sk_recur_view v;
    if (sk_recur_view_(r, &v) != SK_OK) return SK_E_ARG;
    if (!a->d_irank) return sk_fail_(a->ctx, SK_E_STATE, "no rank map (sk_covacc_set_recurrence)");
    if (v.device != a->device) return sk_fail_(a->ctx, SK_E_ARG, "the planes are on another device");
    if (v.nmembers != a->nm) return sk_fail_(a->ctx, SK_E_ARG, "the planes have %u members, the accumulator %u", v.nmembers, a->nm);
    for (uint32_t m = 0; m < a->nm; m++)
        if (v.nbits[m] != a->rec_nbits[m])
            return sk_fail_(a->ctx, SK_E_ARG, "member %u: %u bits in the planes, %u informative rows", m, v.nbits[m], a->rec_nbits[m]);
    if (sample >= v.nsamples) return sk_fail_(a->ctx, SK_E_ARG, "sample %u: the planes have %u", sample, v.nsamples);
    CA_HIP(hipSetDevice(a->device));
    unsigned long long stray = 0;
    cov_t0(a);
    CA_HIP(hipMemsetAsync(a->d_stray, 0, 8u, a->stream));
    unsigned gx = (a->max_rows + 255u) / 256u;
    gx = gx < 1u ? 1u : gx > 256u ? 256u : gx;
    hipLaunchKernelGGL(covacc_mark, dim3(gx, a->nm), dim3(256), 0, a->stream, (const uint32_t *)a->d_depth, (const uint64_t *)a->d_base,
                       (const uint32_t *)a->d_nrows, (const uint32_t *)a->d_irank, (const uint32_t *)a->d_rec_nbits, v.d_word_base,
                       v.d_planes + (size_t)sample * v.words, a->d_stray);
    CA_HIP(hipGetLastError());
    CA_HIP(hipMemcpyAsync(&stray, a->d_stray, 8u, hipMemcpyDeviceToHost, a->stream));
    CA_HIP(hipStreamSynchronize(a->stream));
    cov_t1(a, &a->ms_mark);
    *out_stray = stray;
    return SK_OK;
}

// ---- thresholds ----
static int cov_thr_clear(sk_covacc *a)
{
    if (a->d_thr_max && a->thr_dirty) {
        CA_HIP(hipMemsetAsync(a->d_thr_max, 0, (size_t)(a->total_rows ? a->total_rows : 1u) * 4u, a->stream));
        CA_HIP(hipMemsetAsync(a->d_thr_cnt, 0, (size_t)a->nm * COV_THR_CLASSES * 16u, a->stream));
        CA_HIP(hipStreamSynchronize(a->stream));
    }
    a->thr_dirty = false;
    return SK_OK;
}

extern "C" int sk_covacc_set_thresholds(sk_covacc *a, const int64_t *t, uint32_t n)
{
    if (!a || n > SK_COVACC_THRESHOLDS_MAX || (n && !t)) return SK_E_ARG;
    for (uint32_t q = 0; q < n; q++)
        if (t[q] < 0 || t[q] > 0x7FFFFFFEll || (q && t[q] <= t[q - 1])) return SK_E_ARG;
    CA_HIP(hipSetDevice(a->device));
    if (n && !a->d_thr_max) {                             // all zero: no row has an entry of any class
        const size_t bytes = (size_t)(a->total_rows ? a->total_rows : 1u) * 4u, cb = (size_t)a->nm * COV_THR_CLASSES * 16u;
        uint32_t *p = NULL; unsigned long long *c = NULL;
        CA_HIP(hipMalloc((void **)&p, bytes));
        if (hipMalloc((void **)&c, cb) != hipSuccess) { (void)hipFree(p); return sk_fail_(a->ctx, SK_E_HIP, "no room for the class counts"); }
        a->d_thr_max = p; a->d_thr_cnt = c;
        CA_HIP(hipMemsetAsync(a->d_thr_max, 0, bytes, a->stream));
        CA_HIP(hipMemsetAsync(a->d_thr_cnt, 0, cb, a->stream));
        CA_HIP(hipStreamSynchronize(a->stream));
        a->thr_dirty = false;
    }
    const int rc = cov_thr_clear(a);                      // (whatever was classified under the old list is gone)
    if (rc != SK_OK) return rc;
    memset(&a->thr, 0, sizeof a->thr);
    for (uint32_t q = 0; q < n; q++) a->thr.t[q] = (long long)t[q];
    a->thr.n = n;
    return SK_OK;
}

extern "C" int sk_covacc_finish_target_thresholds(sk_covacc *a, uint64_t *thr_unique, uint64_t *thr_total)
{
    if (!a || !thr_unique || !thr_total) return SK_E_ARG;
    if (!a->thr.n) return sk_fail_(a->ctx, SK_E_STATE, "thresholds are off (sk_covacc_set_thresholds)");
    CA_HIP(hipSetDevice(a->device));
    const size_t ncell = (size_t)a->nm * COV_THR_CLASSES;
    std::vector<unsigned long long> h(ncell * 2u, 0ull);
    if (a->thr_dirty) {                                   // (nothing classified since the last finish: every number is zero)
        cov_t0(a);
        unsigned gx = (a->max_rows + 255u) / 256u;
        gx = gx < 1u ? 1u : gx > 256u ? 256u : gx;
        hipLaunchKernelGGL(covacc_thr_finish, dim3(gx, a->nm), dim3(256), 0, a->stream, a->d_thr_max, (const uint64_t *)a->d_base,
                           (const uint32_t *)a->d_nrows, a->d_thr_cnt + ncell);
        CA_HIP(hipGetLastError());
        CA_HIP(hipMemcpyAsync(h.data(), a->d_thr_cnt, ncell * 16u, hipMemcpyDeviceToHost, a->stream));
        CA_HIP(hipMemsetAsync(a->d_thr_cnt, 0, ncell * 16u, a->stream));
        CA_HIP(hipStreamSynchronize(a->stream));
        cov_t1(a, &a->ms_thr);
        a->thr_dirty = false;
    }
    for (uint32_t m = 0; m < a->nm; m++) {                // class c counts for the thresholds 0 .. c - 1: suffix sums
        unsigned long long u = 0, t = 0;
        for (uint32_t q = a->thr.n; q-- > 0u; ) {
            t += h[(size_t)m * COV_THR_CLASSES + q + 1u];
            u += h[ncell + (size_t)m * COV_THR_CLASSES + q + 1u];
            thr_unique[(size_t)m * a->thr.n + q] = u; thr_total[(size_t)m * a->thr.n + q] = t;
        }
    }
    return SK_OK;
}

// ---- the scrub sweep ----
extern "C" int sk_covacc_set_classes(sk_covacc *a, uint32_t member, const uint32_t *rows, const uint8_t *cls, uint64_t n, uint32_t ncls)
{
    if (!a || (n && (!rows || !cls))) return SK_E_ARG;
    if (member >= a->nm) return sk_fail_(a->ctx, SK_E_ARG, "member %u: the accumulator has %u", member, a->nm);
    if (ncls > SK_SCRUB_SWEEP_MAX) return sk_fail_(a->ctx, SK_E_ARG, "%u classes: at most %u", ncls, SK_SCRUB_SWEEP_MAX);
    if (!ncls && n) return sk_fail_(a->ctx, SK_E_ARG, "rows with classes, and no class");
    for (uint64_t i = 0; i < n; i++) {
        if (rows[i] >= a->nrows[member]) return sk_fail_(a->ctx, SK_E_ARG, "row %u: member %u has %u", rows[i], member, a->nrows[member]);
        if (cls[i] < 1u || cls[i] > ncls) return sk_fail_(a->ctx, SK_E_ARG, "class %u of row %u: 1 to %u", cls[i], rows[i], ncls);
    }
    if (!ncls && !a->d_cls) return SK_OK;                 // (off, and never on)
    CA_HIP(hipSetDevice(a->device));
    if (!a->d_cls) {                                      // all zero: no row is in any set, no member has classes
        const size_t bytes = (size_t)(a->total_rows ? a->total_rows : 1u), ob = ((size_t)a->nm * SK_SCRUB_SWEEP_MAX * 2u + 1u) * 8u;
        uint8_t *p = NULL; uint32_t *q = NULL; unsigned long long *o = NULL;
        CA_HIP(hipMalloc((void **)&p, bytes));
        if (hipMalloc((void **)&q, (size_t)a->nm * 4u) != hipSuccess || hipMalloc((void **)&o, ob) != hipSuccess) {
            (void)hipFree(p); (void)hipFree(q);
            return sk_fail_(a->ctx, SK_E_HIP, "no room for the class bytes");
        }
        a->d_cls = p; a->d_ncls = q; a->d_cls_out = o;
        a->ncls.assign(a->nm, 0u);
        CA_HIP(hipMemsetAsync(a->d_cls, 0, bytes, a->stream));
        CA_HIP(hipMemsetAsync(a->d_ncls, 0, (size_t)a->nm * 4u, a->stream));
    }
    if (a->nrows[member]) CA_HIP(hipMemsetAsync(a->d_cls + a->base[member], 0, a->nrows[member], a->stream));
    if (n) {
        int rc = cov_room(a, (void **)&a->d_rows, &a->rows_cap, (size_t)n * 4u, false);
        if (rc == SK_OK) rc = cov_room(a, (void **)&a->d_cls_up, &a->cls_up_cap, (size_t)n, false);
        if (rc != SK_OK) return rc;
        CA_HIP(hipMemcpyAsync(a->d_rows, rows, (size_t)n * 4u, hipMemcpyHostToDevice, a->stream));
        CA_HIP(hipMemcpyAsync(a->d_cls_up, cls, (size_t)n, hipMemcpyHostToDevice, a->stream));
        hipLaunchKernelGGL(covacc_class_scatter, dim3(cov_grid(n)), dim3(256), 0, a->stream, (const uint32_t *)a->d_rows,
                           (const uint8_t *)a->d_cls_up, n, a->nrows[member], ncls, a->d_cls + a->base[member]);
        CA_HIP(hipGetLastError());
    }
    CA_HIP(hipMemcpyAsync(a->d_ncls + member, &ncls, 4u, hipMemcpyHostToDevice, a->stream));
    CA_HIP(hipStreamSynchronize(a->stream));
    a->ncls[member] = ncls;
    return SK_OK;
}

extern "C" int sk_covacc_finish_target_classes(sk_covacc *a, uint64_t *out_unique, uint64_t *out_total, uint64_t *out_stray)
{
    if (!a || !out_unique || !out_total || !out_stray) return SK_E_ARG;
    uint32_t F = 0;
    for (uint32_t m = 0; m < a->nm && !a->ncls.empty(); m++) if (a->ncls[m] > F) F = a->ncls[m];
    if (!F) return sk_fail_(a->ctx, SK_E_STATE, "no member has classes (sk_covacc_set_classes)");
    CA_HIP(hipSetDevice(a->device));
    const size_t ncell = (size_t)a->nm * SK_SCRUB_SWEEP_MAX * 2u;
    std::vector<unsigned long long> h(ncell + 1u, 0ull);
    cov_t0(a);
    CA_HIP(hipMemsetAsync(a->d_cls_out, 0, (ncell + 1u) * 8u, a->stream));
    unsigned gx = (a->max_rows + 255u) / 256u;
    gx = gx < 1u ? 1u : gx > 256u ? 256u : gx;
    hipLaunchKernelGGL(covacc_class_finish, dim3(gx, a->nm), dim3(256), 0, a->stream, (const uint32_t *)a->d_depth,
                       (const uint64_t *)a->d_base, (const uint32_t *)a->d_nrows, (const uint8_t *)a->d_cls, (const uint32_t *)a->d_ncls,
                       a->d_cls_out, a->d_cls_out + ncell);
    CA_HIP(hipGetLastError());
    CA_HIP(hipMemcpyAsync(h.data(), a->d_cls_out, (ncell + 1u) * 8u, hipMemcpyDeviceToHost, a->stream));
    CA_HIP(hipStreamSynchronize(a->stream));
    cov_t1(a, &a->ms_cls);
    for (uint32_t m = 0; m < a->nm; m++) {                // class c counts for the fractions 0 .. c - 1: suffix sums
        unsigned long long u = 0, t = 0;
        for (uint32_t q = F; q-- > 0u; ) {
            if (q < a->ncls[m]) { u += h[((size_t)m * SK_SCRUB_SWEEP_MAX + q) * 2u]; t += h[((size_t)m * SK_SCRUB_SWEEP_MAX + q) * 2u + 1u]; }
            out_unique[(size_t)m * F + q] = u; out_total[(size_t)m * F + q] = t;
        }
    }
    *out_stray = h[ncell];
    return SK_OK;
}

// ---- rarefaction ----
static int cov_rar_clear(sk_covacc *a)
{
    if (a->d_rar_max && a->rar_dirty) {
        CA_HIP(hipMemsetAsync(a->d_rar_max, 0, (size_t)(a->total_rows ? a->total_rows : 1u) * 4u, a->stream));
        CA_HIP(hipMemsetAsync(a->d_rar_cnt, 0, ((size_t)a->nm * 2u + 1u) * COV_RAR_CLASSES * 8u, a->stream));
        CA_HIP(hipStreamSynchronize(a->stream));
    }
    a->rar_dirty = false;
    return SK_OK;
}

extern "C" int sk_covacc_set_rarefaction(sk_covacc *a, const uint64_t *T, uint32_t n, uint32_t seed)
{
    if (!a || n > SK_COVACC_RAREFACTION_MAX || (n && !T)) return SK_E_ARG;
    for (uint32_t q = 0; q < n; q++)
        if (T[q] > 0x100000000ull || (q && T[q] >= T[q - 1])) return SK_E_ARG;   // (T = 0, a fraction below 2^-32, holds no pair)
    CA_HIP(hipSetDevice(a->device));
    if (n && !a->d_rar_max) {                             // all zero: no row has a line of any class, no pair was counted
        const size_t bytes = (size_t)(a->total_rows ? a->total_rows : 1u) * 4u, cb = ((size_t)a->nm * 2u + 1u) * COV_RAR_CLASSES * 8u;
        uint32_t *p = NULL; unsigned long long *c = NULL;
        CA_HIP(hipMalloc((void **)&p, bytes));
        if (hipMalloc((void **)&c, cb) != hipSuccess) { (void)hipFree(p); return sk_fail_(a->ctx, SK_E_HIP, "no room for the class counts"); }
        a->d_rar_max = p; a->d_rar_cnt = c;
        CA_HIP(hipMemsetAsync(a->d_rar_max, 0, bytes, a->stream));
        CA_HIP(hipMemsetAsync(a->d_rar_cnt, 0, cb, a->stream));
        CA_HIP(hipStreamSynchronize(a->stream));
        a->rar_dirty = false;
    }
    const int rc = cov_rar_clear(a);                      // (whatever was classified under the old list is gone)
    if (rc != SK_OK) return rc;
    memset(&a->rar, 0, sizeof a->rar);
    for (uint32_t q = 0; q < n; q++) a->rar.t[q] = (unsigned long long)T[q];
    a->rar.n = n; a->rar.seed = seed;
    return SK_OK;
}

extern "C" int sk_covacc_set_pair_base(sk_covacc *a, uint64_t first_pair)
{
    if (!a) return SK_E_ARG;
    a->pair_base = (unsigned long long)first_pair;
    return SK_OK;
}

extern "C" int sk_covacc_add_pairs(sk_covacc *a, uint64_t first, uint64_t n)
{
    if (!a) return SK_E_ARG;
    if (!a->rar.n) return sk_fail_(a->ctx, SK_E_STATE, "rarefaction is off (sk_covacc_set_rarefaction)");
    if (!n) return SK_OK;
    CA_HIP(hipSetDevice(a->device));
    const unsigned g = cov_grid(n);
    hipLaunchKernelGGL(covacc_rar_pairs, dim3(g > 256u ? 256u : g), dim3(256), 0, a->stream, (unsigned long long)first, n, a->rar,
                       a->d_rar_cnt + (size_t)a->nm * COV_RAR_CLASSES * 2u);
    CA_HIP(hipGetLastError());
    CA_HIP(hipStreamSynchronize(a->stream));
    a->rar_dirty = true;
    return SK_OK;
}

extern "C" int sk_covacc_add_rows_hits_pairs(sk_covacc *a, uint32_t member, const uint32_t *rows, const uint32_t *total_hits,
                                             const uint64_t *pair_ordinal, uint64_t n)
{
    if (!a || (n && (!rows || !total_hits || !pair_ordinal))) return SK_E_ARG;
    if (!a->rar.n) return sk_fail_(a->ctx, SK_E_STATE, "rarefaction is off (sk_covacc_set_rarefaction)");
    int rc = sk_covacc_add_rows_hits(a, member, rows, total_hits, n);     // (the counters and the thresholds, every argument checked)
    if (rc != SK_OK || !n) return rc;
    if ((rc = cov_room(a, (void **)&a->d_pairs, &a->pairs_cap, (size_t)n * 8u, false)) != SK_OK) return rc;
    cov_t0(a);
    CA_HIP(hipMemcpyAsync(a->d_pairs, pair_ordinal, (size_t)n * 8u, hipMemcpyHostToDevice, a->stream));
    hipLaunchKernelGGL(covacc_rows_rar, dim3(cov_grid(n)), dim3(256), 0, a->stream, (const uint32_t *)a->d_rows, (const uint32_t *)a->d_tots,
                       (const unsigned long long *)a->d_pairs, n, a->nrows[member], a->min_hits, a->rar, a->d_rar_max + a->base[member],
                       a->d_rar_cnt + (size_t)member * COV_RAR_CLASSES);
    CA_HIP(hipGetLastError());
    CA_HIP(hipStreamSynchronize(a->stream));
    cov_t1(a, &a->ms_fold);
    a->rar_dirty = true;
    return SK_OK;
}

extern "C" int sk_covacc_finish_target_rarefaction(sk_covacc *a, uint64_t *out_pairs, uint64_t *out_unique, uint64_t *out_total)
{
    if (!a || !out_pairs || !out_unique || !out_total) return SK_E_ARG;
    if (!a->rar.n) return sk_fail_(a->ctx, SK_E_STATE, "rarefaction is off (sk_covacc_set_rarefaction)");
    CA_HIP(hipSetDevice(a->device));
    const size_t ncell = (size_t)a->nm * COV_RAR_CLASSES, nall = ncell * 2u + COV_RAR_CLASSES;
    std::vector<unsigned long long> h(nall, 0ull);
    if (a->rar_dirty) {                                   // (nothing classified since the last finish: every number is zero)
        cov_t0(a);
        unsigned gx = (a->max_rows + 255u) / 256u;
        gx = gx < 1u ? 1u : gx > 256u ? 256u : gx;
        hipLaunchKernelGGL(covacc_thr_finish, dim3(gx, a->nm), dim3(256), 0, a->stream, a->d_rar_max, (const uint64_t *)a->d_base,
                           (const uint32_t *)a->d_nrows, a->d_rar_cnt + ncell);
        CA_HIP(hipGetLastError());
        CA_HIP(hipMemcpyAsync(h.data(), a->d_rar_cnt, nall * 8u, hipMemcpyDeviceToHost, a->stream));
        CA_HIP(hipMemsetAsync(a->d_rar_cnt, 0, nall * 8u, a->stream));
        CA_HIP(hipStreamSynchronize(a->stream));
        cov_t1(a, &a->ms_rarfin);
        a->rar_dirty = false;
    }
    const uint32_t nq = a->rar.n;
    unsigned long long np = 0;
    for (uint32_t q = nq; q-- > 0u; ) { np += h[ncell * 2u + q + 1u]; out_pairs[q] = np; }
    for (uint32_t m = 0; m < a->nm; m++) {                // class c counts for the subsamples 0 .. c - 1: suffix sums
        unsigned long long u = 0, t = 0;
        for (uint32_t q = nq; q-- > 0u; ) {
            t += h[(size_t)m * COV_RAR_CLASSES + q + 1u];
            u += h[ncell + (size_t)m * COV_RAR_CLASSES + q + 1u];
            out_unique[(size_t)m * nq + q] = u; out_total[(size_t)m * nq + q] = t;
        }
    }
    return SK_OK;
}
