// sk_packdev.hip -- the record stream packed ON THE DEVICE into sk_pack_stream's layout (the list scan's packed input cache: a chunk
// that went up as bytes -- every chunk of a .gz item, whose decode threads have no cycles to spare -- is packed here, beside its scan,
// and the packed form copied home for the cache file).
//
// A translation unit of its own, as sk_text.hip is: its own stream and device buffers, the scan reached through sk_scan_device, so
// that the scan kernel's sources stay as they are.  The layout is sk_pack.h's: per 16-byte chunk of the stream a 32-bit word of
// sixteen 2-bit codes (A 0, C 1, G 2, T 3 in either case, first byte highest, 0 for any other byte) and a 16-bit mask of the bytes
// that are no A/C/G/T; (nbytes + 15) / 16 code words, then as many masks.  Bytes of the last chunk beyond nbytes are "no A/C/G/T" and
// never odd.  *odd: the stream holds a byte that is neither A/C/G/T, N/n nor '\n'.
#include <hip/hip_runtime.h>
#include <pthread.h>
#include <stdint.h>
#include <string.h>
#include <map>
#include <new>
#include <vector>

#include "../../include/strainer_kmer.h"
#include "sk_internal.h"

#define PK_THREADS 256
#define PK_MAX     ((64ull << 20) - 64u)        // what sk_scan_pinned takes

// one byte: bits 0-1 its code, bit 2 "no A/C/G/T", bit 3 "odd" (not even N/n or '\n')
__device__ __forceinline__ uint32_t pk_byte(uint32_t b)
{
    const uint32_t u = b & 0xDFu;
    const uint32_t code = u == 'C' ? 1u : u == 'G' ? 2u : u == 'T' ? 3u : 0u;
    const bool valid = (u == 'A') | (u == 'C') | (u == 'G') | (u == 'T');
    const bool fine = valid | (u == 'N') | (b == '\n');
    return valid ? code : (fine ? 4u : 12u);
}

// the 16 bytes of one chunk, first byte in the low byte of w[0]
__device__ __forceinline__ void pk_chunk(const uint32_t w[4], uint32_t &code32, uint32_t &inv16, uint32_t &odd)
{
    uint32_t c = 0u, m = 0u, o = 0u;
#pragma unroll
    for (int i = 0; i < 16; i++) {
        const uint32_t r = pk_byte((w[i >> 2] >> (8 * (i & 3))) & 0xFFu);
        c = (c << 2) | (r & 3u);
        m |= ((r >> 2) & 1u) << i;
        o |= r >> 3;
    }
    code32 = c; inv16 = m; odd = o;
}

// chunk g of the stream; a chunk the stream's end cuts is read byte by byte and filled with '\n' (no A/C/G/T, not odd): nothing
// at or beyond nbytes is read
__device__ __forceinline__ void pk_load(const uint8_t *__restrict__ stream, uint64_t nbytes, uint64_t g, uint32_t w[4])
{
    const uint64_t at = g * 16u;
    if (at + 16u <= nbytes) {
        const uint4 v = *(const uint4 *)(stream + at);
        w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
    } else {
        w[0] = w[1] = w[2] = w[3] = 0x0A0A0A0Au;
#pragma unroll
        for (uint32_t i = 0; i < 16u; i++)
            if (at + i < nbytes) w[i >> 2] = (w[i >> 2] & ~(0xFFu << (8u * (i & 3u)))) | ((uint32_t)stream[at + i] << (8u * (i & 3u)));
    }
}

// One lane, two chunks: two 16-byte loads, one uint2 of code words and one u32 of two masks out (codes is 8-byte aligned, so masks --
// 4 * nch bytes behind it -- is 4-byte aligned, and a pair starts at an even chunk).  The odd flag is a plain store of 1 by every
// lane that saw an odd byte: all of them write the same value.
__global__ __launch_bounds__(PK_THREADS) void sk_pack_chunks(const uint8_t *__restrict__ stream, uint64_t nbytes, uint32_t *__restrict__ codes,
                                                             uint16_t *__restrict__ masks, uint32_t *__restrict__ odd_flag)
{
    const uint64_t nch = (nbytes + 15u) >> 4, npair = (nch + 1u) >> 1;
    for (uint64_t p = (uint64_t)blockIdx.x * PK_THREADS + threadIdx.x; p < npair; p += (uint64_t)gridDim.x * PK_THREADS) {
        const uint64_t g = 2u * p;
        uint32_t w0[4], w1[4], c0, m0, o0, c1 = 0u, m1 = 0u, o1 = 0u;
        const bool two = g + 1u < nch;
        pk_load(stream, nbytes, g, w0);
        if (two) pk_load(stream, nbytes, g + 1u, w1);
        pk_chunk(w0, c0, m0, o0);
        if (two) {
            pk_chunk(w1, c1, m1, o1);
            *(uint2 *)(codes + g) = make_uint2(c0, c1);
            *(uint32_t *)(masks + g) = m0 | (m1 << 16);
        } else {
            codes[g] = c0;
            masks[g] = (uint16_t)m0;
        }
        if (o0 | o1) *odd_flag = 1u;
    }
}

struct pk_state {
    int          device = 0;
    hipStream_t  stream = NULL;
    uint64_t     cap = 0;                          // stream bytes d_bytes[b] holds
    uint8_t     *d_bytes[2] = {NULL, NULL}, *d_pk[2] = {NULL, NULL};
    uint32_t    *d_odd = NULL;                     // [0], [1]: the two buffers' flags; [2]: sk_pack_device's
    uint32_t    *h_odd = NULL;                     // page-locked landing place of [2]
    std::vector<sk_ctx *> readers[2];              // the contexts whose scans of d_bytes[b] have not been waited for
    int          cur = 0;
    hipEvent_t   up = NULL, home[64] = {};         // the upload is on the device; ticket t's packed form is home
    uint64_t     tickets = 0;
};
static pthread_mutex_t pk_mu = PTHREAD_MUTEX_INITIALIZER;
static std::map<sk_ctx *, pk_state *> pk_states;

#define PK_HIP(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return sk_fail_(ctx, SK_E_HIP, "%s failed: %s", #call, hipGetErrorString(e_)); } while (0)

static void pk_free_buffers(pk_state *s)
{
    for (int b = 0; b < 2; b++) { (void)hipFree(s->d_bytes[b]); (void)hipFree(s->d_pk[b]); s->d_bytes[b] = s->d_pk[b] = NULL; }
    s->cap = 0;
}

static void pk_free_device(pk_state *s)
{
    if (s->stream && hipSetDevice(s->device) == hipSuccess) {
        (void)hipStreamSynchronize(s->stream);
        pk_free_buffers(s);
        (void)hipFree(s->d_odd);
        (void)hipHostFree(s->h_odd);
        if (s->up) (void)hipEventDestroy(s->up);
        for (int i = 0; i < 64; i++) if (s->home[i]) (void)hipEventDestroy(s->home[i]);
        (void)hipStreamDestroy(s->stream);
    }
    s->stream = NULL; s->d_odd = NULL; s->h_odd = NULL; s->up = NULL;
    memset(s->home, 0, sizeof s->home);
    s->readers[0].clear(); s->readers[1].clear();
    s->tickets = 0;
}

static int pk_state_get(sk_ctx *ctx, pk_state **out)
{
    pthread_mutex_lock(&pk_mu);
    pk_state *&slot = pk_states[ctx];
    if (!slot) slot = new (std::nothrow) pk_state();
    pk_state *const s = slot;
    if (!s) pk_states.erase(ctx);
    pthread_mutex_unlock(&pk_mu);
    if (!s) return SK_E_NOMEM;
    *out = s;
    const int dev = sk_ctx_device_(ctx);
    if (s->stream && s->device != dev) pk_free_device(s);        // (a context made anew at the address of one that was never released)
    if (!s->stream) {
        PK_HIP(hipSetDevice(dev));
        s->device = dev;
        if (hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking) != hipSuccess || hipMalloc((void **)&s->d_odd, 4 * sizeof(uint32_t)) != hipSuccess ||
            hipHostMalloc((void **)&s->h_odd, 64, hipHostMallocDefault) != hipSuccess || hipEventCreateWithFlags(&s->up, hipEventDisableTiming) != hipSuccess) {
            if (s->up) (void)hipEventDestroy(s->up);
            if (s->h_odd) (void)hipHostFree(s->h_odd);
            (void)hipFree(s->d_odd);
            if (s->stream) (void)hipStreamDestroy(s->stream);
            s->stream = NULL; s->d_odd = NULL; s->h_odd = NULL; s->up = NULL;
            return sk_fail_(ctx, SK_E_HIP, "no stream or memory for the device pack");
        }
    }
    return SK_OK;
}

extern "C" void sk_pack_release(sk_ctx *ctx)
{
    pthread_mutex_lock(&pk_mu);
    pk_state *s = NULL;
    std::map<sk_ctx *, pk_state *>::iterator it = pk_states.find(ctx);
    if (it != pk_states.end()) { s = it->second; pk_states.erase(it); }
    pthread_mutex_unlock(&pk_mu);
    if (!s) return;
    pk_free_device(s);
    delete s;
}

// enqueued on s->stream: the flag cleared, the kernel
static int pk_enqueue(sk_ctx *ctx, pk_state *s, const void *dev_stream, uint64_t nbytes, void *dev_packed, uint32_t *d_odd)
{
    const uint64_t nch = (nbytes + 15u) >> 4, npair = (nch + 1u) >> 1;
    uint64_t blocks = (npair + PK_THREADS - 1u) / PK_THREADS;
    if (blocks > 2048u) blocks = 2048u;                          // (a memory-bound pass: the rest by grid stride)
    PK_HIP(hipMemsetAsync(d_odd, 0, sizeof(uint32_t), s->stream));
    if (!nch) return SK_OK;
    hipLaunchKernelGGL(sk_pack_chunks, dim3((uint32_t)blocks), dim3(PK_THREADS), 0, s->stream, (const uint8_t *)dev_stream, nbytes,
                       (uint32_t *)dev_packed, (uint16_t *)((uint8_t *)dev_packed + nch * 4u), d_odd);
    PK_HIP(hipGetLastError());
    return SK_OK;
}

extern "C" int sk_pack_device(sk_ctx *ctx, const void *dev_stream, uint64_t nbytes, void *dev_packed, int *odd)
{
    if (!ctx || !odd || (nbytes && (!dev_stream || !dev_packed))) return SK_E_ARG;
    if (((uintptr_t)dev_stream & 15u) || ((uintptr_t)dev_packed & 7u))
        return sk_fail_(ctx, SK_E_ARG, "the device stream must be 16-byte aligned, the packed form 8-byte aligned");
    pk_state *s;
    int rc = pk_state_get(ctx, &s);
    if (rc != SK_OK) return rc;
    PK_HIP(hipSetDevice(s->device));
    if ((rc = sk_sync(ctx)) != SK_OK) return rc;                  // (the stream may have been put there by work on the context's stream)
    if ((rc = pk_enqueue(ctx, s, dev_stream, nbytes, dev_packed, s->d_odd + 2)) != SK_OK) return rc;
    PK_HIP(hipMemcpyAsync(s->h_odd, s->d_odd + 2, sizeof(uint32_t), hipMemcpyDeviceToHost, s->stream));
    PK_HIP(hipStreamSynchronize(s->stream));
    *odd = s->h_odd[0] != 0u;
    return SK_OK;
}

// d_bytes[b] is about to be written: whoever may still read it is waited for (sk_text.hip's rule: a reader that is not one of this
// call's contexts may be gone by now and is not touched -- the whole device is waited for instead)
static int pk_wait_readers(sk_ctx *ctx, pk_state *s, int b, sk_ctx *const *ctxs, uint32_t nctx)
{
    bool all = false;
    for (sk_ctx *r : s->readers[b]) {
        bool mine = false;
        for (uint32_t i = 0; i < nctx; i++) mine |= ctxs[i] == r;
        if (!mine) all = true;
        else { const int rc = sk_sync(r); if (rc != SK_OK) return rc; }
    }
    s->readers[b].clear();
    if (all) PK_HIP(hipDeviceSynchronize());
    return SK_OK;
}

// One upload, n COUNT scans, one pack.  Two device buffers take turns: chunk n goes up and is packed on this unit's stream while the
// contexts still scan chunk n - 1 out of the other buffer; when the upload has landed every context is waited for -- which frees that
// other buffer for chunk n + 1 -- and its scan of chunk n queued (sk_scan_device).  On return `pinned` has been read; the packed form
// (sk_packed_bytes(nbytes) bytes) and the flag (one u32: non-zero = odd, the packed form is then of no use) are on their way into
// pinned_packed_out / pinned_odd_out and are there once sk_pack_ticket_wait(ctx[0], *ticket) has returned.
static int pk_scan_pack(sk_ctx *const *ctxs, uint32_t nctx, const uint8_t *pinned, uint64_t nbytes, uint32_t col,
                        void *pinned_packed_out, uint32_t *pinned_odd_out, uint64_t *ticket, pk_state **state)
{
    if (!ctxs || nctx < 1 || !ctxs[0] || !ticket || !pinned_odd_out || (nbytes && (!pinned || !pinned_packed_out))) return SK_E_ARG;
    sk_ctx *const ctx = ctxs[0];
    for (uint32_t i = 0; i < nctx; i++) {
        if (!ctxs[i]) return SK_E_ARG;
        if (sk_ctx_device_(ctxs[i]) != sk_ctx_device_(ctx)) return sk_fail_(ctx, SK_E_ARG, "context %u is on another device: one upload serves one device", i);
        if (col >= sk_table_cols(ctxs[i])) return sk_fail_(ctx, SK_E_ARG, "context %u: column %u out of range", i, col);
    }
    if (nbytes > PK_MAX) return sk_fail_(ctx, SK_E_ARG, "pinned batch larger than 64 MiB - 64 bytes");
    pk_state *s;
    int rc = pk_state_get(ctx, &s);
    if (rc != SK_OK) return rc;
    *state = s;
    PK_HIP(hipSetDevice(s->device));
    if (nbytes > s->cap) {
        for (int b = 0; b < 2; b++) if ((rc = pk_wait_readers(ctx, s, b, ctxs, nctx)) != SK_OK) return rc;     // (a scan may still read the old buffers)
        PK_HIP(hipStreamSynchronize(s->stream));
        pk_free_buffers(s);
        const uint64_t cap = (nbytes + ((1u << 20) - 1u)) & ~(uint64_t)((1u << 20) - 1u);
        for (int b = 0; b < 2; b++) {
            PK_HIP(hipMalloc((void **)&s->d_bytes[b], cap + 64u));
            PK_HIP(hipMalloc((void **)&s->d_pk[b], ((cap + 15u) >> 4) * 6u + 64u));
        }
        s->cap = cap;
    }
    // tickets and the ring's events are read by sk_pack_ticket_wait on other threads: both change under pk_mu only
    pthread_mutex_lock(&pk_mu);
    const uint64_t t = s->tickets;
    hipEvent_t ev = s->home[t & 63u];
    pthread_mutex_unlock(&pk_mu);
    if (ev) PK_HIP(hipEventSynchronize(ev));                      // (ring slot of ticket t - 64)
    else {
        PK_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        pthread_mutex_lock(&pk_mu);
        s->home[t & 63u] = ev;
        pthread_mutex_unlock(&pk_mu);
    }
    const int b = s->cur ^ 1;
    if ((rc = pk_wait_readers(ctx, s, b, ctxs, nctx)) != SK_OK) return rc;
    s->cur = b;
    if (nbytes) PK_HIP(hipMemcpyAsync(s->d_bytes[b], pinned, nbytes, hipMemcpyHostToDevice, s->stream));
    PK_HIP(hipEventRecord(s->up, s->stream));
    if ((rc = pk_enqueue(ctx, s, s->d_bytes[b], nbytes, s->d_pk[b], s->d_odd + b)) != SK_OK) return rc;
    if (nbytes) PK_HIP(hipMemcpyAsync(pinned_packed_out, s->d_pk[b], ((nbytes + 15u) >> 4) * 6u, hipMemcpyDeviceToHost, s->stream));
    PK_HIP(hipMemcpyAsync(pinned_odd_out, s->d_odd + b, sizeof(uint32_t), hipMemcpyDeviceToHost, s->stream));
    PK_HIP(hipEventRecord(ev, s->stream));
    pthread_mutex_lock(&pk_mu);
    s->tickets = t + 1;                                           // (issued only now: its event has been recorded)
    pthread_mutex_unlock(&pk_mu);
    *ticket = t;
    PK_HIP(hipEventSynchronize(s->up));                           // the bytes are on the device: the contexts' streams may read them
    for (uint32_t i = 0; nbytes && i < nctx; i++) {
        // the scan of the chunk before is waited for: this context no longer reads the other buffer
        std::vector<sk_ctx *> &other = s->readers[b ^ 1];
        if ((rc = sk_sync(ctxs[i])) != SK_OK) return rc;
        for (size_t k = 0; k < other.size(); ) { if (other[k] == ctxs[i]) other.erase(other.begin() + (long)k); else k++; }
        s->readers[b].push_back(ctxs[i]);                         // (before the launch: a scan that failed half-way may have queued work)
        if ((rc = sk_scan_device(ctxs[i], s->d_bytes[b], nbytes, col)) != SK_OK)
            return ctxs[i] == ctx ? rc : sk_fail_(ctx, rc, "context %u: %s", i, sk_last_error(ctxs[i]));
    }
    return SK_OK;
}

// A call that fails may have queued its copies home already: they are waited for here, so that the caller's page-locked buffers are
// its own again when it sees the error (no ticket comes with an error).
extern "C" int sk_scan_pinned_pack_many(sk_ctx *const *ctxs, uint32_t nctx, const uint8_t *pinned, uint64_t nbytes, uint32_t col,
                                        void *pinned_packed_out, uint32_t *pinned_odd_out, uint64_t *ticket)
{
    pk_state *s = NULL;
    const int rc = pk_scan_pack(ctxs, nctx, pinned, nbytes, col, pinned_packed_out, pinned_odd_out, ticket, &s);
    if (rc != SK_OK && s && s->stream && hipSetDevice(s->device) == hipSuccess) (void)hipStreamSynchronize(s->stream);
    return rc;
}

// strain_detect's target cache: the bytes a batch holds, packed where they lie.  Enqueued on the batch's OWN stream, so behind the
// upload of the current contents and behind its `ready` event -- the tallies wait for that event only, never for this -- and ahead of
// the next fill, which is what may overwrite the bytes.  The kernel is sk_pack_chunks as above: whole 16-byte chunks below nbytes by
// one load, the chunk the stream's end cuts byte by byte, so neither the batch's 16 bytes of slack nor what an earlier, longer fill
// left beyond nbytes is read.  Into the batch's own buffer (it grows with the batch's stream buffer), then sk_packed_bytes(nbytes)
// bytes and the flag (one u32: non-zero = odd) home; they are there once sk_batch_pack_wait has returned.
extern "C" int sk_batch_pack_home(sk_batch *b, void *pinned_packed_out, uint32_t *pinned_odd_out)
{
    if (!b || !pinned_packed_out || !pinned_odd_out) return SK_E_ARG;
    sk_batch_pack_hook hk;
    const int rc = sk_batch_pack_hook_(b, 1, &hk);
    if (rc != SK_OK) return rc;
    sk_ctx *const ctx = hk.owner;
    hipStream_t st = (hipStream_t)hk.stream;
    const uint64_t nch = (hk.nbytes + 15u) >> 4, npair = (nch + 1u) >> 1;
    uint64_t blocks = (npair + PK_THREADS - 1u) / PK_THREADS;
    if (blocks > 2048u) blocks = 2048u;
    PK_HIP(hipMemsetAsync(hk.d_odd, 0, sizeof(uint32_t), st));
    hipLaunchKernelGGL(sk_pack_chunks, dim3((uint32_t)blocks), dim3(PK_THREADS), 0, st, (const uint8_t *)hk.d_stream, hk.nbytes,
                       (uint32_t *)hk.d_pack, (uint16_t *)((uint8_t *)hk.d_pack + nch * 4u), hk.d_odd);
    PK_HIP(hipGetLastError());
    PK_HIP(hipMemcpyAsync(pinned_packed_out, hk.d_pack, nch * 6u, hipMemcpyDeviceToHost, st));
    PK_HIP(hipMemcpyAsync(pinned_odd_out, hk.d_odd, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    PK_HIP(hipEventRecord((hipEvent_t)hk.home, st));
    return SK_OK;
}

extern "C" int sk_batch_pack_wait(sk_batch *b)
{
    if (!b) return SK_E_ARG;
    sk_batch_pack_hook hk;
    const int rc = sk_batch_pack_hook_(b, 0, &hk);
    if (rc != SK_OK) return rc;
    sk_ctx *const ctx = hk.owner;
    if (!hk.home) return sk_fail_(ctx, SK_E_STATE, "no pack was asked of this batch");
    PK_HIP(hipEventSynchronize((hipEvent_t)hk.home));
    return SK_OK;
}

extern "C" int sk_pack_ticket_wait(sk_ctx *ctx, uint64_t ticket)
{
    if (!ctx) return SK_E_ARG;
    pthread_mutex_lock(&pk_mu);
    std::map<sk_ctx *, pk_state *>::iterator it = pk_states.find(ctx);
    pk_state *s = it != pk_states.end() ? it->second : NULL;
    const uint64_t issued = s ? s->tickets : 0;
    hipEvent_t ev = s && ticket < issued ? s->home[ticket & 63u] : NULL;
    pthread_mutex_unlock(&pk_mu);
    if (!s || !s->stream || ticket >= issued) return SK_E_ARG;
    if (issued - ticket > 64) return SK_OK;                       // its ring slot was recycled only after it completed
    PK_HIP(hipSetDevice(s->device));
    PK_HIP(hipEventSynchronize(ev));
    return SK_OK;
}
