// The union table's kernels (one table for several resident strains) -- part of sk_device.hip (included there, in this order; not a translation unit of its own).

// ---------------------------------------------------------------------------------------------
// One table for several resident strains (strain_detect -S, BASELINE configs[4]: 32 strains per GPU against one
// metagenome).  Without it a batch of reads is scanned once per strain; with it once.  New relative to the reference,
// which holds one strain per process (src/strain_detect.c:137-146).
//
// The union is built on the device from the members' resident tables: global row g = base[s] + the member's counter
// index; the members' texts and rank maps are laid one behind the other (each padded to a multiple of 64 bases), so
// that seed-and-verify works on the union as it does on one strain.  A key that several strains hold gets ONE slot (the
// first member's: its row and text position), but every one of its global rows carries the same pair of masks
// {members that hold the key, members in which it is informative}: whichever row a hit comes out at -- the slot's, or
// the rank of a position in another member's text -- it names the same strains.  The hit log names, per informative
// strain, that member's own row (sk_union_post looks the key up in the member's table).
// ---------------------------------------------------------------------------------------------
struct sk_union_member { const sk_u4 *slots; uint32_t mask; const uint32_t *inv; };

__global__ void sk_union_insert(const sk_u4 *__restrict__ mslots, uint64_t nslots, uint32_t base, uint32_t tbase,
                                sk_u4 *slots, uint32_t mask, uint64_t *__restrict__ ukeys)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nslots; i += stride) {
        const sk_u4 e = mslots[i];
        const uint64_t k = sk_slot_key(e);
        if (k == SK_EMPTY64) continue;
        const uint32_t g = base + e.z;
        ukeys[g] = k;
        const uint32_t tp = e.w >> 1;
        const uint32_t w = tp == 0x7FFFFFFFu ? e.w : (((tbase + tp) << 1) | (e.w & 1u));
        uint32_t slot = sk_slot0(sk_khash(k), mask);
        for (;;) {
            const unsigned long long old = atomicCAS((unsigned long long *)&slots[slot], (unsigned long long)SK_EMPTY64, (unsigned long long)k);
            if (old == SK_EMPTY64) { ((uint32_t *)&slots[slot])[2] = g; ((uint32_t *)&slots[slot])[3] = w; break; }
            if (old == k) break;                           // an earlier member holds the key: its slot stands
            slot = (slot + 1u) & mask;
        }
    }
}

// pass A: every row finds its key's slot row ("canon") and sets its member's bits there
__global__ void sk_union_mask_a(const sk_u4 *__restrict__ mslots, uint64_t nslots, uint32_t base, uint32_t s,
                                const uint32_t *__restrict__ type, uint32_t inf_value,
                                const sk_u4 *__restrict__ slots, uint32_t mask, uint2 *umask, uint32_t *__restrict__ canon)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nslots; i += stride) {
        const sk_u4 e = mslots[i];
        const uint64_t k = sk_slot_key(e);
        if (k == SK_EMPTY64) continue;
        uint32_t slot = sk_slot0(sk_khash(k), mask), w = 0xFFFFFFFFu;
        for (;;) {
            const sk_u4 u = slots[slot];
            const uint64_t uk = sk_slot_key(u);
            if (uk == k) { w = u.z; break; }
            if (uk == SK_EMPTY64) break;                   // (cannot happen: every key was inserted)
            slot = (slot + 1u) & mask;
        }
        const uint32_t g = base + e.z;
        canon[g] = w == 0xFFFFFFFFu ? g : w;
        if (w == 0xFFFFFFFFu) continue;
        atomicOr(&umask[w].x, 1u << s);
        if (type[e.z] == inf_value) atomicOr(&umask[w].y, 1u << s);
    }
}

// pass B: the other rows of a key copy the pair
__global__ void sk_union_mask_b(uint2 *umask, const uint32_t *__restrict__ canon, uint32_t n)
{
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n) return;
    const uint32_t w = canon[g];
    if (w != g && w < n) umask[g] = umask[w];
}

// a member's rank map into the union's: counter indices move by the member's base
__global__ void sk_union_rank_copy(sk_u4 *__restrict__ dst, const sk_u4 *__restrict__ src, uint32_t nsrc, uint32_t ndst, uint32_t base, uint32_t after)
{
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= ndst) return;
    if (b < nsrc) { sk_u4 r = src[b]; r.x += base; dst[b] = r; }
    else dst[b] = (sk_u4){after, 0u, 0u, 0u};             // padding: no row starts here
}

// The scan logged (position, global row) once per informative hit.  Dealt out here: one entry per strain in which the row's key
// is informative, {position, strain << SK_UNION_ROW_BITS | that member's OWN row of the key} (a probe of the key in the member's
// table).  *nout counts every entry, stored or not (the caller asks again with more room if it exceeds cap_out).
struct sk_union_resolve_args {
    const uint2 *raw; const unsigned long long *nraw; unsigned long long cap_raw;
    uint2 *out; unsigned long long *nout; unsigned long long cap_out;
    const uint64_t *ukeys; const uint2 *umask; const sk_union_member *mem;
};
__device__ __forceinline__ void sk_union_resolve_block(const sk_union_resolve_args &a, uint32_t block, uint32_t nblocks)
{
    const uint2 *__restrict__ raw = a.raw; uint2 *__restrict__ out = a.out; unsigned long long *nout = a.nout;
    const unsigned long long cap_out = a.cap_out;
    const uint64_t *__restrict__ ukeys = a.ukeys; const uint2 *__restrict__ umask = a.umask; const sk_union_member *__restrict__ mem = a.mem;
    const unsigned long long n = *a.nraw < a.cap_raw ? *a.nraw : a.cap_raw;
    const unsigned long long stride = (unsigned long long)nblocks * blockDim.x;
    for (unsigned long long i = (unsigned long long)block * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint2 e = raw[i];
        uint32_t infm = umask[e.y].y;
        const uint64_t k = ukeys[e.y];
        unsigned long long at = atomicAdd(nout, (unsigned long long)__popc(infm));
        while (infm) {
            const uint32_t s = (uint32_t)__builtin_ctz(infm);
            infm &= infm - 1u;
            const sk_union_member m = mem[s];
            uint32_t slot = sk_slot0(sk_khash(k), m.mask), row = (1u << SK_UNION_ROW_BITS) - 1u;
            for (;;) {
                const sk_u4 u = m.slots[slot];
                const uint64_t uk = sk_slot_key(u);
                if (uk == k) { row = m.inv ? m.inv[u.z] : u.z; break; }
                if (uk == SK_EMPTY64) break;
                slot = (slot + 1u) & m.mask;
            }
            if (at < cap_out) out[at] = make_uint2(e.x, (s << SK_UNION_ROW_BITS) | row);
            at++;
        }
    }
}

// The (record, strain) tallies of a union scan live in a dense array that is ALL ZERO between launches: the scan marks the
// records it touched (one byte each), and this pass visits only those -- appends {record * ns + strain, all, informative} for
// the pairs that were hit, zeroes them again and clears the mark.  Its cost follows the reads that hit a strain, not
// records x strains (57 MB per 32 MiB batch of 150-base reads and 32 strains; zeroing and sweeping that much took longer
// than the scan itself).
#define SK_UC_SETS_MAX 16u                                          // at most this many sets of 64 records per wave (a workgroup of four waves: 4096 records)
__device__ __forceinline__ void sk_union_compact_block(uint2 *__restrict__ tally, uint8_t *__restrict__ flag, uint32_t nrec, uint32_t ns,
                                                       uint32_t *__restrict__ out, unsigned long long *n, uint32_t sets, uint32_t block)
{
    // A wave looks at 64 records' marks at once; the marked ones (about one in fifty) are then taken two at a time, half a wave
    // per record with one lane per strain: a row of 32 tallies is ONE 256-byte read and the non-zero ones find their places by
    // ballot and popcount.  The workgroup counts first, claims its room with ONE atomic, then writes: the room counter is one
    // address for the whole card, and the memory side does about 120 M returning atomics a second on one address -- with one
    // atomic per marked record (rounds 2-4) this kernel took 587 us for the 71 K pairs of a 512 MiB batch, 35 us for the 4 K of a
    // 32 MiB one, next to scans of 787 and 69 us (profiles/r04_union_launch_trace.txt).  `sets` trades the atomics (one per
    // workgroup) against the wave's chain of dependent reads (a set after the other): the host picks it for a few hundred workgroups.
    __shared__ uint32_t wcount[4];
    __shared__ unsigned long long wbase[4];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, half = lane >> 5, sl = lane & 31u;
    const uint32_t first = (block * 4u + wave) * (sets * 64u);                     // this wave's first record
    unsigned long long at = 0;
    for (int pass = 0; pass < 2; pass++) {
        uint32_t cnt = 0;
        for (uint32_t set = 0; set < sets; set++) {
            const uint32_t r0 = first + set * 64u, r = r0 + lane;
            if (r0 >= nrec) break;
            const bool marked = r < nrec && flag[r] != 0;
            uint64_t m = __ballot(marked);
            if (pass && marked) flag[r] = 0;
            while (m) {
                const uint32_t b0 = (uint32_t)__builtin_ctzll(m);
                m &= m - 1;
                uint32_t b1 = 64u;
                if (m) { b1 = (uint32_t)__builtin_ctzll(m); m &= m - 1; }
                const uint32_t mine = half ? b1 : b0;
                for (uint32_t sb = 0; sb < ns; sb += 32u) {        // (SK_UNION_MAX is 32: one round)
                    const uint32_t st = sb + sl;
                    const bool act = mine < 64u && st < ns;
                    uint2 *const cell = tally + (size_t)(r0 + (act ? mine : 0u)) * ns + (act ? st : 0u);
                    uint2 t = make_uint2(0u, 0u);
                    if (act) t = *cell;
                    const bool nz = act && (t.x | t.y) != 0u;
                    const uint64_t bm = __ballot(nz);
                    if (pass && nz) {
                        const unsigned long long o = at + cnt + (unsigned long long)__popcll(bm & ((1ull << lane) - 1ull));
                        out[3 * o] = (r0 + mine) * ns + st; out[3 * o + 1] = t.x; out[3 * o + 2] = t.y;
                        *cell = make_uint2(0u, 0u);
                    }
                    cnt += (uint32_t)__popcll(bm);
                }
            }
        }
        if (pass) break;
        if (lane == 0u) wcount[wave] = cnt;
        __syncthreads();
        if (threadIdx.x == 0u) {
            const uint32_t total = wcount[0] + wcount[1] + wcount[2] + wcount[3];
            unsigned long long base = total ? atomicAdd(n, (unsigned long long)total) : 0ull;
            for (uint32_t w = 0; w < 4u; w++) { wbase[w] = base; base += wcount[w]; }
        }
        __syncthreads();
        if (!cnt) break;                                           // (this wave has nothing to write; wave-uniform)
        at = wbase[wave];
    }
}

// Both of the above in one launch (they do not depend on each other, only on the scan): the first `ncompact` workgroups compact,
// the others deal the log out.
__global__ void __launch_bounds__(256) sk_union_post(uint2 *__restrict__ tally, uint8_t *__restrict__ flag, uint32_t nrec, uint32_t ns,
                                                     uint32_t *__restrict__ out, unsigned long long *n, uint32_t sets, uint32_t ncompact,
                                                     const sk_union_resolve_args ra)
{
    if (blockIdx.x < ncompact) sk_union_compact_block(tally, flag, nrec, ns, out, n, sets, blockIdx.x);
    else sk_union_resolve_block(ra, blockIdx.x - ncompact, gridDim.x - ncompact);
}

// The results' way home: the three counters, the first `eager` compacted pairs and log entries written straight into the page-locked
// landing area on the host (`land` is its device address), and the OTHER set of counters zeroed for the next launch.  One kernel
// where there were a memset and three copies, each its own trip through the runtime: 0.18 -> see profiles/r04_union_summary.txt.
__global__ void sk_union_ship(const unsigned long long *__restrict__ cnt, unsigned long long *__restrict__ cnt_next,
                              const uint32_t *__restrict__ compact, unsigned long long pairs_cap,
                              const uint2 *__restrict__ hits, unsigned long long hits_cap, uint32_t eager, uint8_t *__restrict__ land)
{
    const unsigned long long c0 = cnt[0], c1 = cnt[1], c2 = cnt[2];
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x, nt = gridDim.x * blockDim.x;
    unsigned long long nr = c1 < pairs_cap ? c1 : pairs_cap, nh = c2 < hits_cap ? c2 : hits_cap;
    if (nr > eager) nr = eager;
    if (nh > eager) nh = eager;
    uint32_t *lr = (uint32_t *)(land + 64);
    uint2 *lh = (uint2 *)(land + 64 + (size_t)eager * 12u);
    for (unsigned long long i = t; i < 3ull * nr; i += nt) lr[i] = compact[i];
    for (unsigned long long i = t; i < nh; i += nt) lh[i] = hits[i];
    if (t == 0) {
        unsigned long long *lc = (unsigned long long *)land;
        lc[0] = c0; lc[1] = c1; lc[2] = c2;
        cnt_next[0] = 0ull; cnt_next[1] = 0ull; cnt_next[2] = 0ull; cnt_next[3] = 0ull;
    }
}

// ---- COUNT on a union (kmer_scrub_count -S).  A scan into the union's column counts a window at the global row it was found
// at: the key's slot row when a probe found it, base[s] + the member's counter index when it was verified against member s's
// text.  Every row of a key names the same slot row ("canon", as in sk_union_mask_a); the fold adds the other rows' counts
// there and gives every member, for each of its counter indices, the count of the key's slot row.  Integer adds: bit-exact in
// any order, u32 wrap included.
__global__ void sk_union_canon_rows(const sk_u4 *__restrict__ mslots, uint64_t nslots, uint32_t base,
                                    const sk_u4 *__restrict__ slots, uint32_t mask, uint32_t *__restrict__ canon)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nslots; i += stride) {
        const sk_u4 e = mslots[i];
        const uint64_t k = sk_slot_key(e);
        if (k == SK_EMPTY64) continue;
        uint32_t slot = sk_slot0(sk_khash(k), mask), w = 0xFFFFFFFFu;
        for (;;) {
            const sk_u4 u = slots[slot];
            const uint64_t uk = sk_slot_key(u);
            if (uk == k) { w = u.z; break; }
            if (uk == SK_EMPTY64) break;                   // (cannot happen: every key was inserted)
            slot = (slot + 1u) & mask;
        }
        const uint32_t g = base + e.z;
        canon[g] = w == 0xFFFFFFFFu ? g : w;
    }
}

// every row that is not its key's slot row adds its count there (slot rows are never read here after they were written:
// canon[w] == w, so no row both gives and takes)
__global__ void sk_union_fold_canon(uint32_t *ucol, const uint32_t *__restrict__ canon, uint32_t n)
{
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n) return;
    const uint32_t w = canon[g];
    if (w != g && w < n) {
        const uint32_t v = ucol[g];
        if (v) atomicAdd(&ucol[w], v);
    }
}

// member column[i] +/-= the count of the slot row of global row base + i (i = the member's counter index)
__global__ void sk_union_fold_member(uint32_t *__restrict__ dst, const uint32_t *__restrict__ ucol, const uint32_t *__restrict__ canon,
                                     uint32_t base, uint32_t n, uint32_t subtract)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t v = ucol[canon[base + i]];
    dst[i] = subtract ? dst[i] - v : dst[i] + v;
}

// ---- the panel's shared keys (sk_union_share; strain_detect -S --panel-share).  New: the reference compares one pair of genomes
// per process (src/genome_compare.c); here every pair of members of union a and union b is counted in one sweep of a's slots.
// A non-empty slot is one distinct key; its row's pair of masks says which members of a hold it (xa) and in which it is
// informative (ya).  With b == a the key's masks in b are the same pair; with another union the key is probed in b's slots (the
// probe of sk_union_mask_a) and a key b lacks adds nothing.  out[0][i][j] += 1 for i in xa, j in xb; out[1] for i in ya, j in xb;
// out[2] for i in ya, j in yb.  As the coverage sweeps (sk_covacc.hip): counted in LDS first -- three 32 x 32 u32 matrices, 12 KiB
// a workgroup, which sees fewer than 2^32 keys -- then the non-zero cells go out with 64-bit atomics.
#define SK_SHARE_BLOCKS 512u                                        // at most this many workgroups of 256: two per CU
#define SK_SHARE_CELLS (3u * SK_UNION_MAX * SK_UNION_MAX)
__device__ __forceinline__ void sk_share_add(uint32_t *m, uint32_t rows, const uint32_t cols)
{
    while (rows) {
        const uint32_t i = (uint32_t)__builtin_ctz(rows);
        rows &= rows - 1u;
        for (uint32_t c = cols; c; c &= c - 1u) atomicAdd(&m[i * SK_UNION_MAX + (uint32_t)__builtin_ctz(c)], 1u);
    }
}
__global__ void __launch_bounds__(256) sk_union_share_sweep(const sk_u4 *__restrict__ aslots, uint64_t naslots, const uint2 *__restrict__ amask,
                                                            const sk_u4 *__restrict__ bslots, uint32_t bmask, const uint2 *__restrict__ bumask,
                                                            unsigned long long *__restrict__ out)
{
    __shared__ uint32_t acc[SK_SHARE_CELLS];
    for (uint32_t c = threadIdx.x; c < SK_SHARE_CELLS; c += blockDim.x) acc[c] = 0u;
    __syncthreads();
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < naslots; i += stride) {
        const sk_u4 e = aslots[i];
        const uint64_t k = sk_slot_key(e);
        if (k == SK_EMPTY64) continue;
        const uint2 ma = amask[e.z];
        uint2 mb = ma;
        if (bslots) {                                              // (uniform: a kernel argument)
            mb = make_uint2(0u, 0u);
            uint32_t slot = sk_slot0(sk_khash(k), bmask);
            for (uint32_t step = 0; ; step++) {
                const sk_u4 u = bslots[slot];
                const uint64_t uk = sk_slot_key(u);
                if (uk == k) { mb = bumask[u.z]; break; }
                if (uk == SK_EMPTY64 || step == bmask) break;      // b does not hold the key (step: a table without an empty slot)
                slot = (slot + 1u) & bmask;
            }
            if (!mb.x) continue;
        }
        sk_share_add(acc, ma.x, mb.x);
        sk_share_add(acc + SK_UNION_MAX * SK_UNION_MAX, ma.y, mb.x);
        sk_share_add(acc + 2u * SK_UNION_MAX * SK_UNION_MAX, ma.y, mb.y);
    }
    __syncthreads();
    for (uint32_t c = threadIdx.x; c < SK_SHARE_CELLS; c += blockDim.x) {
        const uint32_t v = acc[c];
        if (v) atomicAdd(out + c, (unsigned long long)v);
    }
}

// ---- the background of step 4's numbers on a union (sk_union_background_finish; include/strainer_kmer.h has the rule).  After
// sk_union_fold_canon a key's count stands on its slot row; one sweep over the union's SLOTS then sees each distinct key once, with
// its masks in hand (the shape of sk_union_share_sweep), and gives the count to every member of the hold mask, in the class its bit
// of the informative mask names (class 0 informative, 1 background).  Counted in LDS first, per (member, class): D + 2 u32 cells --
// depths 0..D and the rows above D -- then two u64, the hits above D and all hits; the non-zero cells go out once per workgroup with
// 64-bit atomics.  32 members at D = 255 are 32 x 2 x 257 u32 + 32 x 2 x 2 u64 = 66 KB, two workgroups per CU on 160 KiB: the host
// sizes the dynamic LDS to the union's members and the call's D.
// COUNT_KEYS (the first call on a union): the rows of every (member, class), whatever their count -- one uniform round per member
// with two ballots, so that the 64 keys of a wave, which related strains nearly all share, cost two LDS adds a member and not 64.
// Later calls take a key with count 0 for granted (rows at depth 0 = the class's rows - its covered rows, on the host): in a
// metagenome that does not hold the strains the sweep then makes no LDS add at all.
// out: per member SK_BACKGROUND_WORDS(D) u64 in sk_background_finish's layout; this kernel adds to total_hits, the two deep
// cells and the depth cells 1..D, and with COUNT_KEYS to nothing else but keys[member * 2 + class].
#define SK_UBG_BLOCKS 512u                                          // at most this many workgroups of 256: two per CU
template <bool COUNT_KEYS>
__global__ void __launch_bounds__(256) sk_union_background_sweep(const sk_u4 *__restrict__ slots, uint64_t nslots, const uint2 *__restrict__ umask,
                                                                 const uint32_t *__restrict__ ucol, uint32_t nrows, uint32_t ns, uint32_t D,
                                                                 unsigned long long *__restrict__ out, unsigned long long *__restrict__ keys)
{
    extern __shared__ unsigned long long ubg_lds[];                 // [ns * 2 * 2] u64, then [ns * 2 * (D + 2)] u32
    const uint32_t cells = ns * 2u, cw = D + 2u;
    unsigned long long *const wide = ubg_lds;                       // wide[2 * cell] hits above D, wide[2 * cell + 1] all hits
    uint32_t *const bins = (uint32_t *)(ubg_lds + 2u * cells);
    for (uint32_t i = threadIdx.x; i < 2u * cells; i += 256u) wide[i] = 0ull;
    for (uint32_t i = threadIdx.x; i < cells * cw; i += 256u) bins[i] = 0u;
    __syncthreads();
    const uint32_t live = ns >= 32u ? 0xFFFFFFFFu : (1u << ns) - 1u;
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t stride = (uint64_t)gridDim.x * 256u;
    for (uint64_t i0 = (uint64_t)blockIdx.x * 256u; i0 < nslots; i0 += stride) {       // (uniform: every lane makes the ballots below)
        const uint64_t i = i0 + threadIdx.x;
        uint2 m = make_uint2(0u, 0u);
        uint32_t v = 0u;
        if (i < nslots) {
            const sk_u4 e = slots[i];
            if (sk_slot_key(e) != SK_EMPTY64 && e.z < nrows) { m = umask[e.z]; m.x &= live; v = ucol[e.z]; }
        }
        if (COUNT_KEYS)
            for (uint32_t s = 0; s < ns; s++) {
                const bool has = (m.x >> s) & 1u, inf = (m.y >> s) & 1u;
                const unsigned long long bi = __ballot(has && inf), bb = __ballot(has && !inf);
                if (lane == 0u) {
                    if (bi) atomicAdd(&bins[(s * 2u) * cw], (uint32_t)__popcll(bi));
                    if (bb) atomicAdd(&bins[(s * 2u + 1u) * cw], (uint32_t)__popcll(bb));
                }
            }
        if (!v) continue;
        for (uint32_t x = m.x; x; x &= x - 1u) {
            const uint32_t s = (uint32_t)__builtin_ctz(x), cell = s * 2u + (((m.y >> s) & 1u) ? 0u : 1u);
            atomicAdd(&bins[cell * cw + (v <= D ? v : D + 1u)], 1u);
            if (v > D) atomicAdd(&wide[2u * cell], (unsigned long long)v);
            atomicAdd(&wide[2u * cell + 1u], (unsigned long long)v);
        }
    }
    __syncthreads();
    const uint32_t words = 2u * (5u + D + 1u), cwords = 5u + D + 1u;      // (SK_BACKGROUND_WORDS, SK_BACKGROUND_CLASS_WORDS)
    for (uint32_t i = threadIdx.x; i < cells * cw; i += 256u) {
        const uint32_t n = bins[i];
        if (!n) continue;
        const uint32_t cell = i / cw, d = i - cell * cw;
        unsigned long long *const o = out + (size_t)(cell >> 1) * words + (size_t)(cell & 1u) * cwords;
        if (d == 0u) { if (COUNT_KEYS) atomicAdd(keys + cell, (unsigned long long)n); }
        else if (d <= D) atomicAdd(o + 5u + d, (unsigned long long)n);
        else atomicAdd(o + 3u, (unsigned long long)n);
    }
    for (uint32_t i = threadIdx.x; i < 2u * cells; i += 256u) {
        const unsigned long long n = wide[i];
        if (!n) continue;
        const uint32_t cell = i >> 1;
        unsigned long long *const o = out + (size_t)(cell >> 1) * words + (size_t)(cell & 1u) * cwords;
        atomicAdd(o + ((i & 1u) ? 2u : 4u), n);
    }
}
