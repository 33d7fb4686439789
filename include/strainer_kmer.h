/* strainer_kmer.h -- C-ABI of libstrainer_kmer.so: the MI355X (gfx950) k-mer scrub/count path.
 *
 * This is the drop-in boundary.  The reference (jeremiahfaith/strainer2, a plain C program)
 * has no FFI: its seam for this path is the internal call chain
 *
 *     GEN_hash_sequences_set_count_vec()   src/genome_compare.c:967-1030   (build the strain table)
 *     GEN_all_kmer_counts[_skip_file]()    src/genome_compare.c:149-177,115-146 (walk a file list)
 *     GEN_calculate_kmer_count()           src/genome_compare.c:179-236     (THE hot loop)
 *     BIO_searchHash()/BIO_getHashKeys()   src/BIO_hash.c:161-172,174-188   (lookup / row order)
 *     print_hash_counts()                  src/kmer_scrub_count.c:134-156   (TSV)
 *     quantify_hits_PE()/hash_scrubbed_kmers()/background_filter()   src/strain_detect.c:387-663,668-726,160-240
 *
 * and, either side of it in the workflow (test/example.sh), the two scripts scripts/kmer_scrub_filter.py and
 * scripts/coverage_depth.py, which are covered here too (sk_filter_*, sk_distinct_count, skh_*_main).
 *
 * The entry points below replace those calls one for one (each cites what it replaces).
 * Plain pointers and sizes only; no C++ or torch types.  Two layers:
 *
 *   sk_*   device layer  -- context, table residency, batch scan, counters, collective.
 *   skh_*  host layer    -- the reference's file/list/record semantics in C (kseq grammar,
 *                           canonical 2-bit packing, BIO_hash slot-order replay, TSV print),
 *                           driving the device layer.  kmer_scrub_count's main() is ~100 lines
 *                           on top of it.
 *
 * There is NO CPU compute fallback: every window lookup runs in a HIP kernel.  Without a
 * usable GPU sk_ctx_create() fails with SK_E_NODEVICE and callers must stop.
 *
 * Stream layout ("record stream") used by the scan entry points: the sequence bytes of the
 * records, verbatim as decoded (any case), records separated by one '\n'.  Bytes that are not
 * A/C/G/T (any case) break windows; '\n', 'N'/'n' and NUL never take part in any window.
 *
 * Thread-safety: one caller per sk_ctx at a time; distinct contexts are independent.
 */
#ifndef STRAINER_KMER_H
#define STRAINER_KMER_H

#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SK_K                 31            /* seed length: src/kmer_scrub_count.c:39, src/strain_detect.c:78 */
#define SK_REF_TABLE_SLOTS   8000000u      /* DEFAULT_GENOME_HASH_SIZE: src/genome_compare.h:20 */
#define SK_KEY_NONE          UINT64_MAX    /* "no packed key for this row" (row is a wide key) */
#define SK_ROWS_IN_STRAIN_ORDER UINT32_MAX /* skh_keyset_from_*: initial_slots value meaning "do not replay the reference's hash table: rows in
                                            * first-occurrence order along the strain" -- for callers whose output does not show the row order
                                            * (strain_detect: src/strain_detect.c prints k-mer text per hit, never walks the table) */
#define SK_LOCALITY_FWD      0x80000000u   /* locality[] flag: the key is the strain text itself at its first occurrence */

/* error codes (0 = success) */
#define SK_OK            0
#define SK_E_NODEVICE   -1   /* no HIP device / HIP runtime failure at init                  */
#define SK_E_HIP        -2   /* a HIP call failed; sk_last_error() has the text              */
#define SK_E_ARG        -3   /* bad argument                                                 */
#define SK_E_NOMEM      -4
#define SK_E_OPEN       -5   /* file could not be opened (host layer)                        */
#define SK_E_DUPKEY     -6   /* duplicate key passed to sk_table_load                        */
#define SK_E_STATE      -7   /* call out of order (e.g. scan before table load)              */
#define SK_E_RCCL       -8
#define SK_E_SPLIT      -9   /* a big text file could not be cut at record boundaries: the run fails rather than count something else */
#define SK_E_PLAN       -10  /* the ranks of a multi-GPU run computed different work plans for a list: every rank leaves */
#define SK_E_CACHE      -11  /* a packed input cache file failed its checksum after chunks of it were counted: the run fails.  (Host
                              * layer only: sk_strerror, which lives with the device layer, has no text of its own for it -- the line on
                              * `err` that names the file is the explanation; the Python binding supplies one.) */

typedef struct sk_ctx sk_ctx;

/* ----------------------------------------------------------------------------------------
 * device layer
 * -------------------------------------------------------------------------------------- */

/* Create a context on HIP device `device` (0-based).  Replaces BIO_initHash(): src/BIO_hash.c:14-37. */
int  sk_ctx_create(sk_ctx **out, int device);
/* Replaces BIO_destroyHashD(): src/BIO_hash.c:77-92. */
void sk_ctx_destroy(sk_ctx *ctx);
const char *sk_last_error(const sk_ctx *ctx);
const char *sk_strerror(int code);

/* Make a strain's key set resident in HBM and allocate ncols zeroed u32 counters per row.
 * keys[r] is the canonical 31-mer of row r packed 2 bits/base, A=0 C=1 G=2 T=3, first base in
 * the most significant position (bits 61..60), i.e. canonical = max(forward, revcomp) as
 * integers == the reference's orient_string() choice (src/genome_compare.c:1100-1141).
 * Rows whose key is not pure ACGT carry SK_KEY_NONE here and are supplied through
 * sk_table_load_wide().  Row order is the caller's (the host layer passes BIO_hash slot order).
 * Replaces the insert half of GEN_hash_sequences_set_count_vec(): src/genome_compare.c:1007-1019. */
int sk_table_load(sk_ctx *ctx, const uint64_t *keys, uint32_t nrows, uint32_t ncols);
/* Same, with a "locality" permutation: locality[r] = position of row r's key in an order in which
 * keys that follow each other in the strain are neighbours (the host layer passes first-occurrence
 * order), in the low 31 bits; bit 31 (SK_LOCALITY_FWD) says whether the key equals the strain text at
 * that occurrence or its reverse complement.  The device keeps its counters (and a copy of the keys)
 * in that order: the hits of one read land on adjacent counters (their atomics coalesce), and the
 * neighbours of a window that hit are first looked for next to it instead of through the hash.
 * Invisible through sk_counts_fetch/set and sk_tally_batch (they speak caller rows);
 * sk_counts_device_ptr/sk_counts_allreduce see the block in locality order, which is the same on
 * every rank that loaded the same key set. */
int sk_table_load_ex(sk_ctx *ctx, const uint64_t *keys, uint32_t nrows, uint32_t ncols, const uint32_t *locality);

/* Strain text for the scan's "seed and verify" stage (optional; after sk_table_load_ex).  text2 = the
 * strain's bases as the build phase read them, 2 bits each in the code of the keys, 16 bases per word with
 * the first base in the most significant position, records laid end to end, nbases in all (bytes that are
 * not A/C/G/T take any code).  first_pos[r] = text position of the first base of an all-ACGT window whose
 * canonical form is row r's key, or UINT32_MAX for rows without one (wide keys; keys that only occur
 * through a U).  Contract on the locality order given to sk_table_load_ex: the rows WITH a position come
 * first, in ascending position order (then the counter index of such a row is the rank of its position, which
 * the device recomputes from a bit per text position).  With the text resident, a window that hit the table
 * tells where the read lies on the strain; its neighbours are then compared with the strain's text at the
 * expected places (a 62-bit compare each, as exact as a table probe) instead of being probed one by one.
 * Replaces nothing in the reference: BIO_searchHash per window (src/BIO_hash.c:161-172) stays the meaning. */
int sk_table_load_text(sk_ctx *ctx, const uint32_t *text2, uint32_t nbases, const uint32_t *first_pos);
/* The whole table made ON THE DEVICE from the strain's text (new; strain_detect's opening): text2 = the bases, 2 bits each, records end
 * to end (as for sk_table_load_text); startok = one bit per position, set where a window of 31 A/C/G/T bases of one record starts
 * (nstarts of them) -- the windows src/genome_compare.c:1000-1019 makes keys of.  Rows are numbered by first occurrence along the
 * text; column 0 of every row = col0_value (src/strain_detect.c:139: default 1, increment 0); *nrows = distinct keys.  No byte-string
 * keys: a strain with U/IUPAC letters goes through skh_keyset_from_file + skh_keyset_load.  sk_table_export_keys: the keys in
 * row order, once.  Replaces GEN_hash_sequences_set_count_vec (src/genome_compare.c:967-1030) for strain_detect. */
int sk_table_build_from_text(sk_ctx *ctx, const uint32_t *text2, const uint32_t *startok, uint32_t nbases, uint32_t nstarts,
                             uint32_t ncols, uint32_t col0_value, uint32_t *nrows);
int sk_table_export_keys(sk_ctx *ctx, uint64_t *keys_out /* nrows */);
int sk_table_export_keys_of(sk_ctx *ctx, const uint32_t *rows, uint32_t n, uint64_t *keys_out /* n */);   /* ... of n chosen rows */

/* Wide keys: rows whose 31-byte upper-cased oriented key contains bytes other than ACGT
 * (IUPAC letters in the strain: SURVEY 8(a) a3/a6).  keys31 = nwide * 32 bytes, each key
 * 31 bytes + NUL; rows[i] = row index of key i. */
int sk_table_load_wide(sk_ctx *ctx, const char *keys31, const uint32_t *rows, uint32_t nwide);

/* Scan one batch of the record stream held in HOST memory: copy to HBM and count, both
 * asynchronous on the context's stream (the call returns once the batch is staged; the
 * caller may reuse `stream` immediately).  Adds 1 to counter column `col` of every row whose
 * key equals the canonical form of a window.  Replaces the window loop of
 * GEN_calculate_kmer_count(): src/genome_compare.c:213-229 + BIO_searchHash(). */
int sk_scan_stream(sk_ctx *ctx, const uint8_t *stream, uint64_t nbytes, uint32_t col);

/* Zero-copy variant for callers that fill pinned host buffers themselves (the host layer's decode
 * threads do): `pinned` comes from sk_pinned_alloc, holds at most 64 MiB - 64 bytes of record stream
 * made of WHOLE records or pieces cut with the k-1 overlap, and is DMA-read in place; it may be
 * rewritten once sk_ticket_wait(ctx, *ticket) has returned. */
int sk_pinned_alloc(sk_ctx *ctx, void **p, uint64_t nbytes);
int sk_pinned_free(sk_ctx *ctx, void *p);
int sk_scan_pinned(sk_ctx *ctx, const uint8_t *pinned, uint64_t nbytes, uint32_t col, uint64_t *ticket);
int sk_ticket_wait(sk_ctx *ctx, uint64_t ticket);

/* The host-side 2-bit pre-pack of a record stream (new; the reference moves bytes through memory only,
 * src/kseq.h:90-141).  sk_pack_stream makes, for every 16-byte chunk of `stream`, what the scan kernel's own first phase would
 * make of it -- a 32-bit word of sixteen 2-bit codes (A 0, C 1, G 2, T 3 in either case, first byte highest; 0 for any other byte)
 * and a 16-bit mask of the bytes that are no A/C/G/T -- into `packed` (sk_packed_bytes(nbytes) bytes: the code words, then the
 * masks): 6 bytes per 16 bases cross the PCIe link instead of 16.  *odd is set when the stream holds a byte that is neither
 * A/C/G/T, N/n nor '\n' (an IUPAC letter, U, '\r': only the exact byte-string kernel can judge its windows, a6 of SURVEY 8):
 * such a batch must go to sk_scan_pinned as bytes.  sk_scan_pinned_packed is sk_scan_pinned for a packed batch (`packed` in
 * memory from sk_pinned_alloc; nbytes = the length of the byte stream it was packed from); counts are the same, bit for bit. */
uint64_t sk_packed_bytes(uint64_t nbytes);
int sk_pack_stream(const uint8_t *stream, uint64_t nbytes, void *packed, int *odd);
int sk_scan_pinned_packed(sk_ctx *ctx, const void *packed, uint64_t nbytes, uint32_t col, uint64_t *ticket);
int sk_scan_device_packed(sk_ctx *ctx, const void *dev_packed, uint64_t nbytes, uint32_t col);   /* the packed batch already in device memory (4-byte aligned) */
/* ONE upload, n COUNT scans (new: several union tables fed by one decode of the lists, kmer_scrub_count -S).  The batch crosses
 * the link once, into ctx[0]'s staging ring under ctx[0]'s ticket; then every ctx[i] (a strain's context or a union's,
 * sk_union_context) scans it into its own column `col`, as sk_scan_pinned[_packed] would.  The staging buffer is reused only
 * after all n scans have read it, so sk_sync(ctx[0]), sk_pinned_free(ctx[0], ..) and sk_ticket_wait(ctx[0], *ticket) speak for
 * the whole group.  Counts equal n separate sk_scan_pinned[_packed] calls, bit for bit.  Refused (errors in ctx[0]): contexts
 * on different devices, a context without a table or count columns, `col` out of range for any of them.  One caller at a time
 * for the whole group. */
int sk_scan_pinned_many(sk_ctx *const *ctx, uint32_t n, const uint8_t *pinned, uint64_t nbytes, uint32_t col, uint64_t *ticket);
int sk_scan_pinned_packed_many(sk_ctx *const *ctx, uint32_t n, const void *packed, uint64_t nbytes, uint32_t col, uint64_t *ticket);
/* The same pack made ON THE DEVICE (new; sk_packdev.hip -- the list scan's packed input cache keeps a chunk that went up as bytes in
 * its packed form without spending a decode thread on it; the reference has no counterpart: it moves bytes through memory only,
 * src/kseq.h:90-141).  sk_pack_device: dev_stream[0..nbytes) (16-byte aligned) into dev_packed (8-byte aligned, sk_packed_bytes(nbytes)
 * bytes), byte for byte what sk_pack_stream writes, *odd as there; nothing at or beyond nbytes is read.  Synchronous.
 * sk_scan_pinned_pack_many: ONE upload of `pinned` (sk_pinned_alloc, at most 64 MiB - 64 bytes), n COUNT scans as sk_scan_pinned_many
 * does (counts equal it bit for bit), and the pack of the same device bytes; on return `pinned` has been read, and the packed form and
 * the flag (one u32, non-zero = odd) are in pinned_packed_out / pinned_odd_out (page-locked) once sk_pack_ticket_wait(ctx[0], *ticket)
 * has returned -- a ticket of this entry's own, not one for sk_ticket_wait.  Buffers and errors are ctx[0]'s; one caller at a time for
 * the whole group.  sk_pack_release frees a context's buffers (before sk_ctx_destroy). */
int sk_pack_device(sk_ctx *ctx, const void *dev_stream, uint64_t nbytes, void *dev_packed, int *odd);
int sk_scan_pinned_pack_many(sk_ctx *const *ctx, uint32_t n, const uint8_t *pinned, uint64_t nbytes, uint32_t col,
                             void *pinned_packed_out, uint32_t *pinned_odd_out, uint64_t *ticket);
int sk_pack_ticket_wait(sk_ctx *ctx, uint64_t ticket);
void sk_pack_release(sk_ctx *ctx);
/* Free and total HBM of the context's device (hipMemGetInfo). */
int sk_device_memory(sk_ctx *ctx, uint64_t *free_bytes, uint64_t *total_bytes);

/* Same, for a batch already resident in HBM (device pointer). */
int sk_scan_device(sk_ctx *ctx, const void *dev_stream, uint64_t nbytes, uint32_t col);

/* Plain FASTA/FASTQ text parsed ON THE DEVICE (new; opt-in for the list scan: option "device_parse", SK_DEVICE_PARSE=1).  Replaces the
 * reference's reader, src/kseq.h:171-211 (which the host layer restates in C), for text that is already in HBM: a line classifier and a
 * compaction instead of a CPU thread walking every byte.
 *   dev_text (16-byte aligned, at most 256 MiB: SK_E_ARG above, so offsets are 32-bit) begins at a record boundary: the start of a
 *   file, or `consumed` of the piece before it.  With status SK_TEXT_OK, dev_stream[0..stream_bytes) is byte for byte the record stream
 *   the reference's parser yields for text[0..consumed): every record's sequence followed by one '\n', records shorter than k and empty
 *   records included (the scan ignores them), case untouched, every byte value that is not line structure passed through;
 *   dev_rec_start[r] (NULL, or room for nrec_cap) = record r's offset in it.  is_eof == 0: a record counts as whole only if the piece
 *   itself shows its end -- FASTQ: all four lines with their '\n'; FASTA: the next record's header character at a line start inside
 *   the piece -- so consumed may be 0 (no progress: send a longer piece).  is_eof != 0: consumed == nbytes.
 *   SK_TEXT_DECLINED is not an error: the piece holds something the two device forms do not cover; consumed is 0, nothing was scanned,
 *   nothing in dev_stream may be used, and the caller parses from the piece's start on the host.
 * The forms, each exact by induction over verified records:
 *   SK_TEXT_FASTQ4  the piece starts with '@' and its third line with '+'.  Line i has kind i mod 4 (a quality line may start with
 *                   @, > or +); every record: line 0 starts with '@', line 1 is non-empty and starts with none of > @ +, line 2 starts
 *                   with '+', line 3 has line 1's length after the CR rule (src/kseq.h:136).  A record that fails declines the piece.
 *   SK_TEXT_FASTA   otherwise, when the piece starts with '>' or '@': a line starting with > or @ is a header, a line starting with
 *                   '+' declines (the reference reads quality from there), empty lines are skipped, every other line is sequence
 *                   with its '\n' dropped; a line of one CR is dropped after a sequence line and declines elsewhere.
 *   Anything else declines; so do a header cut by the end of the file and a FASTQ record cut by it.
 * sk_scan_text_pinned: `pinned_text` (sk_pinned_alloc) goes up, is parsed, and the stream is counted into column col as by
 * sk_scan_device; on return the buffer has been read (the scan itself may still run: sk_sync).  _many: one upload and one parse, the
 * stream scanned into every ctx[i] (one device); scratch, errors and sk_text_stats are ctx[0]'s.  The parser's scratch is made when a
 * context first parses, sized for that piece, and grows only for a longer one; sk_text_release frees it (before sk_ctx_destroy).
 * sk_text_stats: pieces sk_scan_text_pinned[_many] took since the last reset, and how many of them declined.
 * sk_text_option: the list scan's switch "device_parse" (0 default, 1 on, may be set at any time; a context that was never told follows
 * the environment variable SK_DEVICE_PARSE=1): whole plain-text items of skh_scan_file and skh_scan_list[_many] then go up as text, in
 * pieces (32 MiB; SK_TEXT_PIECE_BYTES), and a piece the device declines hands the rest of its file to the host parser.  It is a call of
 * its own because sk_set_option lives with the scan kernel, which this path leaves untouched.  sk_text_enabled: what holds for ctx. */
#define SK_TEXT_TILE      16384u        /* text bytes per workgroup of the line passes (tests aim at its boundaries) */
#define SK_TEXT_OK        0u
#define SK_TEXT_DECLINED  1u
#define SK_TEXT_FASTA     1u
#define SK_TEXT_FASTQ4    2u
typedef struct sk_text_info {
    uint32_t status;        /* SK_TEXT_OK | SK_TEXT_DECLINED */
    uint32_t form;          /* SK_TEXT_FASTA | SK_TEXT_FASTQ4 */
    uint64_t consumed;      /* bytes of text that are whole records; text[consumed..) is the caller's to send again */
    uint64_t stream_bytes;  /* bytes written to dev_stream */
    uint64_t nrecords;      /* records in it */
    uint64_t bases;         /* sum of their lengths, short and empty ones included */
} sk_text_info;
int sk_text_parse_device(sk_ctx *ctx, const void *dev_text, uint64_t nbytes, int is_eof,
                         void *dev_stream /* nbytes + 1 bytes */, uint32_t *dev_rec_start /* NULL or nrec_cap */,
                         uint64_t nrec_cap, sk_text_info *info);
int sk_scan_text_pinned(sk_ctx *ctx, const uint8_t *pinned_text, uint64_t nbytes, int is_eof, uint32_t col, sk_text_info *info);
int sk_scan_text_pinned_many(sk_ctx *const *ctx, uint32_t n, const uint8_t *pinned_text, uint64_t nbytes, int is_eof, uint32_t col,
                             sk_text_info *info);
int sk_text_stats(sk_ctx *ctx, uint64_t *pieces, uint64_t *declined, int reset);
void sk_text_release(sk_ctx *ctx);
int sk_text_option(sk_ctx *ctx, int on);
int sk_text_enabled(sk_ctx *ctx);
int sk_text_timing(sk_ctx *ctx, double *last_ms);   /* device time of the context's last parse (HIP events around its passes) */

/* strain_detect's per-READ view of the same scan (src/strain_detect.c:443-541): one batch of the
 * record stream whose records start at rec_start[0..nrec) (byte offsets into `stream`, ascending;
 * a record ends at the next start).  For record r: out_tally[2r] = windows that hit any key,
 * out_tally[2r+1] = windows that hit a key whose counter in column `type_col` equals
 * `informative_value`; each of the latter is also logged as {window-end offset, row} in out_hits
 * (unordered; *out_nhits may exceed hits_cap: then only hits_cap entries were stored).  Synchronous. */
typedef struct sk_hit { uint32_t pos, row; } sk_hit;
int sk_tally_batch(sk_ctx *ctx, const uint8_t *stream, uint64_t nbytes, const uint32_t *rec_start, uint32_t nrec,
                   uint32_t type_col, uint32_t informative_value, uint32_t *out_tally /* 2*nrec */,
                   sk_hit *out_hits, uint64_t hits_cap, uint64_t *out_nhits);

/* The same in pieces, for tallying ONE batch against MANY tables (several strains resident on one
 * device, one context each): upload the batch once, launch on every context (each on its own HIP
 * stream, so the launches overlap), then collect.  A batch may be refilled only after every launch on
 * it has been collected; a context has at most one launch in flight.  New: the reference runs one
 * strain per process and re-reads the metagenome for each. */
typedef struct sk_batch sk_batch;
int  sk_batch_create(sk_ctx *ctx, sk_batch **out);          /* on ctx's device; errors are reported through ctx */
void sk_batch_destroy(sk_batch *b);
int  sk_batch_sync(sk_batch *b);                               /* its uploads are done: the host memory it was filled from may be reused, the batch kept for the next file */
int  sk_batch_fill(sk_batch *b, const uint8_t *stream, uint64_t nbytes, const uint32_t *rec_start, uint32_t nrec);
int  sk_batch_fill_packed(sk_batch *b, const void *packed, uint64_t nbytes, const uint32_t *rec_start, uint32_t nrec);   /* the batch in sk_pack_stream's form (nbytes, rec_start: of the byte stream it was packed from) */
/* The bytes the batch holds (sk_batch_fill), packed on the device into sk_pack_stream's form and copied home -- strain_detect's target
 * cache.  Enqueued on the batch's own stream behind the upload: no tally waits for it.  sk_packed_bytes(nbytes) bytes go to
 * pinned_packed_out (nothing behind them is written) and one u32, non-zero = odd, to pinned_odd_out; both are there once
 * sk_batch_pack_wait has returned.  SK_E_STATE: the batch is packed already, was parsed from text, or is empty. */
int  sk_batch_pack_home(sk_batch *b, void *pinned_packed_out, uint32_t *pinned_odd_out);
int  sk_batch_pack_wait(sk_batch *b);
/* A batch filled from plain TEXT, parsed on the device (new; opt-in for strain_detect: option "device_parse", SK_DEVICE_PARSE=1): what
 * sk_batch_fill does with a record stream the host made, for a piece of FASTA/FASTQ text as it lies in the file.
 *   A piece is pinned_text[0..nbytes) (sk_pinned_alloc; at most 256 MiB), beginning at a record boundary as for sk_text_parse_device.
 *   is_eof == 0: a piece before the file's last; give it ONE byte of look-ahead -- the first byte of the piece that follows, inside
 *   nbytes -- so that both forms count its last record, and accept it only if consumed == nbytes - 1.  is_eof != 0: the last piece.
 *   sk_batch_fill_text enqueues on the batch's stream and returns at once: the upload, the parser's passes writing the record stream
 *   and every record's start into the batch, the tile index the TALLY scan reads (made on the device: only it knows the number of
 *   records), and the copies home.  The text must stay as it is until sk_batch_text_finish.  Every tally launched on the batch's
 *   previous contents must have been collected, as for sk_batch_fill.
 *   sk_batch_text_finish waits and fills *info (status, form, consumed, stream_bytes, nrecords, bases); *rec_start (may be NULL) points
 *   at the nrecords record starts in the batch's page-locked staging, valid until the batch is filled again: record i has
 *   (i + 1 < nrecords ? rec_start[i + 1] : stream_bytes) - rec_start[i] - 1 bases.  The batch holds EVERY record of the piece, in file
 *   order, records shorter than k and empty ones included: they have no window, so they tally 0 and log nothing, and a record's
 *   index in the tallies is its index in the piece.  The results equal those of sk_batch_fill with the host-made stream of the same
 *   records.
 *   The decline rule: SK_TEXT_DECLINED (not an error) for whatever the two device forms do not cover, and for a piece with more than
 *   2^22 records.  A declined piece, and one without records, leaves the batch unusable: a launch on it fails with SK_E_STATE until
 *   it is filled again.  The caller parses from the piece's start on the host. */
int  sk_batch_fill_text(sk_batch *b, const uint8_t *pinned_text, uint64_t nbytes, int is_eof);
int  sk_batch_text_finish(sk_batch *b, sk_text_info *info, const uint32_t **rec_start);
int  sk_tally_launch(sk_ctx *ctx, const sk_batch *b, uint32_t type_col, uint32_t informative_value, uint64_t hits_cap);
int  sk_tally_collect(sk_ctx *ctx, uint32_t *out_tally /* 2*nrec */, sk_hit *out_hits /* hits_cap */, uint64_t *out_nhits);
/* The same collection, sparse: only records with at least one hit, compacted on the device, as {record, all hits,
 * informative hits} in no particular order (*n of them; at most cap are stored).  What comes back over PCIe is then
 * proportional to the reads that hit this strain, not to the reads of the batch (many strains x one metagenome:
 * src/strain_detect.c:443-626 keeps two counters per read and strain). */
typedef struct sk_tally_rec { uint32_t rec, all, inf; } sk_tally_rec;
int  sk_tally_collect_sparse(sk_ctx *ctx, sk_tally_rec *out, uint64_t cap, uint64_t *n, sk_hit *out_hits /* hits_cap */, uint64_t *out_nhits);

/* ONE table for several resident strains: a batch is then scanned once, not once per strain (BASELINE configs[4]: 32
 * strains per GPU against one metagenome).  `members`: 1..SK_UNION_MAX contexts on one device, each with its table, text
 * stage and type column as they are to be used (the union is a snapshot: build it after the -a/-g flags are final; the
 * members stay as they are and must outlive it).  SK_E_STATE if a member has byte-string keys or no text stage -- the
 * caller then tallies member by member (sk_tally_launch).
 * sk_union_tally_collect: out[i] = {record * n + member, windows that hit a key of that member, those whose key is
 * informative_value in the member's type_col} for the (record, member) pairs with at least one hit, unordered;
 * out_hits[j] = {window-end offset, member << SK_UNION_ROW_BITS | the MEMBER's own row}, one per informative hit and member
 * (a member has fewer than 2^27 - 1 rows, else SK_E_STATE).  Batches of any size below 4 GiB.  New: the reference holds one
 * strain per process
 * (src/strain_detect.c:137-146) and re-reads the metagenome for each (:263-384). */
#define SK_UNION_MAX 32
#define SK_UNION_ROW_BITS 27
typedef struct sk_union sk_union;
int  sk_union_create(sk_ctx *const *members, uint32_t n, uint32_t type_col, uint32_t informative_value, sk_union **out); /* errors: members[0] */
void sk_union_destroy(sk_union *u);
int  sk_union_tally_launch(sk_union *u, const sk_batch *b, uint64_t hits_cap);
int  sk_union_tally_collect(sk_union *u, sk_tally_rec *out, uint64_t cap, uint64_t *n, sk_hit *out_hits /* hits_cap */, uint64_t *out_nhits);
int  sk_union_sync(sk_union *u);                               /* wait for a launch whose results will not be collected */
int  sk_union_scan_timing(sk_union *u, double *total_ms, uint64_t *launches, int reset);   /* sk_scan_timing of the union's scans */
const char *sk_union_last_error(const sk_union *u);          /* of launch/collect */
uint32_t sk_union_members(const sk_union *u);
uint32_t sk_union_rows(const sk_union *u);                   /* the members' rows added up */
/* COUNT on a union (kmer_scrub_count -S: many strains counted over ONE pass of the -A/-B/-C lists).  sk_union_count_enable gives
 * the union's context ncols (1..16) zeroed count columns of sk_union_rows() u32 each, the difference array the scan needs and the
 * map of every global row (base of member s + the member's counter index) to the row of its key's slot; calling it again with
 * the same ncols does nothing.  sk_union_context: that context (owned by the union: never destroy it), on which
 * sk_scan_stream / sk_scan_pinned[_packed] / sk_scan_device[_packed], skh_scan_file and skh_scan_list count into a union column;
 * without count columns they refuse it with SK_E_STATE.  sk_union_counts_fold: union column `ucol` is folded into column
 * `member_col` of every member whose bit is set in member_mask (subtract != 0: taken off, u32 wrapping -- a file counted
 * for all members is taken back from some), then zeroed; synchronous.  Afterwards each such member's column has changed
 * exactly as if the same batches had been scanned into it directly.  Replaces GEN_all_kmer_counts[_skip_file]()
 * (src/genome_compare.c:149-177,115-146) run once per strain process (src/kmer_scrub_count.c:87-99). */
int  sk_union_count_enable(sk_union *u, uint32_t ncols);
sk_ctx *sk_union_context(sk_union *u);
int  sk_union_counts_fold(sk_union *u, uint32_t ucol, uint32_t member_col, uint32_t member_mask, int subtract);
/* The k-mers the strains of a panel SHARE (new: strain_detect -S --panel-share=FILE): every pair of members at once, at the
 * workflow's k, from the masks every row of a union carries.  The reference has no counterpart: its genome_compare
 * (src/genome_compare.c) compares one pair of genomes per process at k = 20 and knows no informative sets.
 * out[3][SK_UNION_MAX][SK_UNION_MAX], u64, row = member of a, column = member of b (b == NULL: b is a):
 *   out[0][i][j] distinct keys that member i of a and member j of b both hold
 *   out[1][i][j] keys informative in member i of a that member j of b holds
 *   out[2][i][j] keys informative in both
 * cells of members that do not exist are 0.  "Informative" is what the union's snapshot holds (sk_union_create's type_col and
 * informative_value).  Synchronous.  SK_E_ARG: a and b on different devices.
 * The table of --panel-share: one file for the whole panel, integers, this header line and then one line per ORDERED pair of
 * strains, a == b included, in the order of the -S file (a outer, b inner):
 *   strain_a<TAB>strain_b<TAB>kmers_a<TAB>informative_a<TAB>shared_kmers<TAB>informative_a_in_b<TAB>informative_both
 * strain names are formed as the coverage tables' strain_name (the -o file's basename without a trailing ".kmer_hits.gz");
 * kmers_a = out[0] and informative_a = out[1] on the diagonal (a against itself), the other three columns are the pair's cells of
 * out[0], out[1], out[2].  Strains of different unions are compared by sk_union_share(u[g], u[h], ..) for g != h. */
int  sk_union_share(sk_union *a, sk_union *b_or_null, uint64_t *out /* 3 * SK_UNION_MAX * SK_UNION_MAX */);

/* The BACKGROUND of step 4's numbers (new: strain_detect --coverage-background; no counterpart in the reference, whose advice is to
 * decide presence "based on the frequency of the rare kmers in the metagenome" -- the frequency to expect depends on how deep the
 * organism is, which only ALL of the strain's k-mers show).  The rule, for strain s and target t:
 *   c[row] = the count step 1's scan (kmer_scrub_count) would give the row with t's files as its list: one per window of any record
 *   of any file of the target whose canonical 31-mer is the row's key.  The window rules are the COUNT scan's, unchanged (case
 *   folding, N, other bytes through the byte-string kernel); pairing, mates and --min-kmer-hits play no part; a record shorter than
 *   k has no window.
 *   A row is INFORMATIVE when its type column holds the informative value after -a/-g (exactly the set the TALLY scan uses),
 *   otherwise it is BACKGROUND.
 *   Per strain, target and class: kmers = rows of the class, covered_kmers = those with c > 0, total_hits = the sum of c (u64);
 *   with a spectrum, per depth d = 0..D the rows with c == d, and the rows and hits above D.
 * sk_scan_batch: a COUNT scan of batch b as it lies on the device (bytes, the packed form, or filled from text) into column `col` of
 *   ctx -- a strain's context, or sk_union_context(u) with count columns.  Ordered behind the batch's upload, on ctx's stream (never on
 *   the second scan lane sk_scan_device[_packed] may take), with the kernels those two launch; counts equal sk_scan_stream of the same byte stream, bit for bit.  It returns at
 *   once: the batch may be refilled only after the scan is done (sk_sync(ctx), or anything else that waits for ctx's stream).
 *   Refused as sk_tally_launch refuses: a batch on another device (SK_E_ARG), an empty or declined batch (SK_E_STATE).
 * sk_background_finish: one sweep over column `col` of ctx, each row classed by column type_col; then the column is zero again (a
 *   second call returns kmers and zeros).  out[SK_BACKGROUND_WORDS(max_depth)], u64: for class 0 (informative) and then class 1
 *   (background) the block {kmers, covered_kmers, total_hits, rows above D, hits above D, rows at depth 0, 1, .., D}.
 *   max_depth D <= SK_BACKGROUND_MAX_DEPTH (SK_E_ARG above); col == type_col is SK_E_ARG.  Synchronous.
 * sk_union_background_finish: the same for every member of a union from ONE count column of its context (the column every batch
 *   of the target went into with one sk_scan_batch each): every key's count is gathered on its slot row, then one sweep over the
 *   union's slots -- each distinct key once -- gives the count to every member that holds the key, in the class that member's bit
 *   of the informative mask names.  out[members][SK_BACKGROUND_WORDS(max_depth)].  The column is zero afterwards.  Nothing is
 *   folded into the members' own columns.  "Informative" is what the union's snapshot holds (sk_union_create).  Synchronous. */
#define SK_BACKGROUND_MAX_DEPTH 255u
#define SK_BACKGROUND_HEAD 5u                                 /* kmers, covered_kmers, total_hits, deep rows, deep hits */
#define SK_BACKGROUND_CLASS_WORDS(D) (SK_BACKGROUND_HEAD + (D) + 1u)
#define SK_BACKGROUND_WORDS(D) (2u * SK_BACKGROUND_CLASS_WORDS(D))
int  sk_scan_batch(sk_ctx *ctx, const sk_batch *b, uint32_t col);
int  sk_background_finish(sk_ctx *ctx, uint32_t col, uint32_t type_col, uint32_t informative_value, uint32_t max_depth,
                          uint64_t *out /* SK_BACKGROUND_WORDS(max_depth) */);
int  sk_union_background_finish(sk_union *u, uint32_t ucol, uint32_t max_depth, uint64_t *out /* members x SK_BACKGROUND_WORDS(max_depth) */);

/* PREVALENCE: in how many items of a list a k-mer occurs (new: kmer_scrub_count --prevalence; the reference has no counterpart).
 * Step 1 adds every file of a list into ONE number per key -- the reference's count[vec_column] += 1 for every window of every
 * file, src/genome_compare.c:220-223 -- and step 2 ranks by that sum, which a few deep samples or one sample that holds the strain
 * decide.  Here the same sum is split per item: for list item j, v_j[row] = the windows of item j alone whose canonical 31-mer is
 * the row's key (the COUNT scan's window rules, unchanged), so that
 *   count[row]      = sum over j of v_j[row]              (mod 2^32: bit for bit the column step 1 always made)
 *   prevalence[row] = the items j with v_j[row] >= min_count
 * and per item j the record {kmers_present = rows with v_j >= min_count, kmer_hits = sum over rows of v_j} (u64 each).
 * sk_item_slots: nslots pairs {scratch column u32[nrows], difference array u32[nrows + 2]} of the loaded table, all zero, and one
 *   block-sums buffer; 0 frees them; a call replaces what an earlier call made.  At most SK_ITEM_SLOTS_MAX.  SK_E_NOMEM / SK_E_HIP
 *   when they do not fit: nothing is kept and no HIP error is left behind.  SK_E_STATE without a table with count columns.  Loading
 *   another table frees the slots.  Nothing is allocated unless this is called.
 * sk_item_slot: from now on every COUNT scan of the context (sk_scan_stream, sk_scan_pinned[_packed][_many],
 *   sk_scan_pinned_pack_many, sk_scan_text_pinned[_many], sk_scan_device[_packed], sk_scan_batch) adds into that slot, whatever
 *   column it names; -1: into the column it names, as ever.  The column's own pending increments are left alone and stay pending.
 *   TALLY launches ignore the slot.  The state is the context's: callers that scan from several threads set it under the lock
 *   that orders their submits.
 * sk_item_fold: behind every scan of the slot on either lane, on the context's stream: per row v = the slot's value;
 *   counts[count_col][row] += v; counts[prev_col][row] += (v >= min_count); the slot is zero again; d_item_record[0] += the rows
 *   with v >= min_count, d_item_record[1] += the sum of v.  d_item_record: two u64 in DEVICE memory (sk_dev_alloc; 8-byte aligned;
 *   NULL: no record), zeroed by the caller, fetched when the caller likes after a sk_sync.  Asynchronous.  min_count >= 1 and
 *   count_col != prev_col, else SK_E_ARG.  Folding an empty slot changes nothing.
 * On a UNION (many strains over one pass of a list): sk_item_slots / sk_item_slot on sk_union_context(u), after
 *   sk_union_count_enable, send the union's COUNT scans into a slot of GLOBAL rows (8 bytes x sk_union_rows(u) a slot), and
 * sk_union_item_fold hands the slot to the members.  All arithmetic mod 2^32.  Per global row g, v_g = the slot's value; per
 *   distinct key, with w its slot row, V_w = the sum of v_g over the rows g of that key (the scan may credit any member's row of a
 *   key several members hold).  For every member s of member_mask and every row i of s, with V the V_w of that row's key:
 *   counts_s[count_col][i] += V; counts_s[prev_col][i] += (V >= min_count); d_records[2 s] += (V >= min_count);
 *   d_records[2 s + 1] += V.  Each such member's columns and record end exactly as sk_item_fold would leave them had the item been
 *   scanned into a slot of that member alone.  Members outside the mask are untouched, their records too; the whole slot is zero
 *   afterwards, also with member_mask 0 (an item that counts for nobody: a -C line equal to every member's genome).  The union's own
 *   count columns and its pending increments are left alone.  d_records: sk_union_members(u) x 2 u64 in DEVICE memory (8-byte
 *   aligned; NULL: no records), zeroed by the caller.  Asynchronous on the union's stream, behind every scan of the slot on either
 *   lane, and the host waits for nothing: five launches whatever the number of members.  While folds are in flight only the
 *   union's stream may touch the members' columns; the caller calls sk_sync(sk_union_context(u)) once where the list ends.
 *   SK_E_STATE without sk_union_count_enable; SK_E_ARG: no such slot, min_count 0, count_col == prev_col, a mask bit beyond the
 *   members, a masked member without the two columns. */
#define SK_ITEM_SLOTS_MAX 256u
int  sk_item_slots(sk_ctx *ctx, uint32_t nslots);
int  sk_item_slot(sk_ctx *ctx, int slot);
int  sk_item_fold(sk_ctx *ctx, uint32_t slot, uint32_t count_col, uint32_t prev_col, uint32_t min_count, uint64_t *d_item_record);
int  sk_union_item_fold(sk_union *u, uint32_t slot, uint32_t count_col, uint32_t prev_col, uint32_t member_mask, uint32_t min_count,
                        uint64_t *d_records /* [members][2] u64 in device memory, or NULL */);

/* Wait for all queued work of the context. */
int sk_sync(sk_ctx *ctx);

/* Counter access, in the caller's row order; u32, wrapping.  (On the device a column is
 * counts[col * nrows + i] with i = row, or i = locality[row] after sk_table_load_ex.)
 * fetch/set replace reads/writes of the reference's per-key count vectors
 * (src/kmer_scrub_count.c:144-151; src/genome_compare.c:1011-1016). */
int sk_counts_fetch(sk_ctx *ctx, uint32_t col, uint32_t *out /* nrows */);
int sk_counts_set(sk_ctx *ctx, uint32_t col, const uint32_t *in /* nrows */);
/* counts[col][rows[i]] = value, i < n: a sparse update (new; strain_detect's type column names 1 % of the rows informative) */
int sk_counts_set_rows(sk_ctx *ctx, uint32_t col, const uint32_t *rows, uint32_t n, uint32_t value);
int sk_counts_zero(sk_ctx *ctx, uint32_t col);
/* Device address of the whole counter block (ncols * nrows u32) for a caller-run collective
 * (torch.distributed / RCCL all-reduce over xGMI).  New: the reference is single-process. */
void    *sk_counts_device_ptr(sk_ctx *ctx);
uint32_t sk_table_rows(const sk_ctx *ctx);
uint32_t sk_table_cols(const sk_ctx *ctx);
/* Multi-GPU, one process per GPU (new: the reference is single-process).
 * sk_comm_init: rank 0 creates an RCCL unique id and publishes it through `id_file`, the other
 * ranks wait (at most timeout_s) for it; every rank then joins the communicator.
 * sk_comm_sum_u32: tiny all-reduce used to agree on failure before the big one.
 * sk_counts_allreduce: in-place sum (u32, wrapping) of the whole counter block over xGMI;
 * rccl_comm = an ncclComm_t, or NULL for the context's own communicator. */
int  sk_comm_init(sk_ctx *ctx, int rank, int world, const char *id_file, int timeout_s);
/* The same, with this rank's set-up status in the exchange that precedes the collective: setup_failed != 0 (ctx may then
 * be NULL: no device, no key set) makes EVERY rank return SK_E_RCCL before anyone blocks in RCCL.  The exchange proves
 * freshness (a file left by a crashed launch is ignored), every wait is bounded by timeout_s, and a watchdog ends the
 * process (exit status 3) if ncclCommInitRank itself does not return in that time.  id_file must be visible to all
 * ranks (node-local /tmp serves one node only). */
int  sk_comm_init_ex(sk_ctx *ctx, int rank, int world, const char *id_file, int timeout_s, int setup_failed);
/* The file exchange alone (no GPU, no RCCL): returns 0 = go, 1 = somebody failed, 2 = timed out, 3 = cannot write.
 * payload128: in on rank 0, out elsewhere.  Exported for the multi-process CPU tests of the protocol. */
int  sk_rendezvous_exchange(int rank, int world, const char *base_path, int my_status, unsigned char *payload128, double timeout_s);
void sk_comm_destroy(sk_ctx *ctx);
int  sk_comm_sum_u32(sk_ctx *ctx, uint32_t value, uint32_t *sum);
/* *agree = 1 iff every rank passed the same value (one max all-reduce of {v, ~v}); without a communicator: 1.
 * skh_scan_list uses it to compare the ranks' work plans before any of them scans. */
int  sk_comm_agree_u64(sk_ctx *ctx, uint64_t value, int *agree);
/* vals[i] = the maximum of vals[i] over all ranks, i < n (one all-reduce; above eight values through a device buffer made for the call: the items'
 * records of a list walk with prevalence); without a communicator: unchanged.  The list
 * walk's two agreements per list are built on it (skh_scan_list below): whatever happens to a rank locally, every rank issues
 * the same sequence of collectives.  sk_comm_world: ranks of the context's communicator, 0 without one. */
int  sk_comm_max_u64(sk_ctx *ctx, uint64_t *vals, uint32_t n);
int  sk_comm_world(const sk_ctx *ctx);
int  sk_counts_allreduce(sk_ctx *ctx, void *rccl_comm);

/* Device-side timing of the scan kernel, from HIP events recorded around every scan kernel since the last
 * reset: launch count, and the milliseconds the scan kernels kept the card busy.  Count scans of resident
 * batches run on two lanes ("scan_lanes") and overlap at their edges; such time is counted once (the length
 * of the union of the launches' intervals), so total_ms / launches is the time a launch ADDS, not how long
 * one kernel took from its first workgroup to its last.  With one lane the two are the same. */
int sk_scan_timing(sk_ctx *ctx, double *total_ms, uint64_t *launches, int reset);

/* Tunables (before sk_table_load).  name: "table_load_pct" (max load factor in percent), "grid_kib" (size of
 * the level-1 filter in KiB, -1 = automatic), "text_stage" (0 = stage 2 probes every window on its own even
 * when the strain's text is resident; for A/B runs and tests), "pipeline" (2 = the partitioned pipeline sk_bin ->
 * sk_lds_probe -> candidates-only scan, an experiment that measured slower than the default single kernel: DESIGN.md
 * section 4), "odd_list_cap" (tests), "scan_lanes" (may be set at any time; 2, the default: back-to-back sk_scan_device /
 * sk_scan_device_packed calls take two streams in turn, so that a launch starts while the one before it drains -- every
 * other call of the context waits for both, results are the same; 1 = all of them on the context's one stream, for A/B
 * runs and tests; the environment variable SK_SCAN_LANES=1 does the same for programs that set no options), "dev_alloc_uncached" (experiment:
 * non-zero = sk_dev_alloc hands out memory the L2 does not keep), "ablate" (accepted as 0 only: the kernel variants it chose were retired).
 * Unknown name -> SK_E_ARG.  Ranges: "table_load_pct" 5..90 (default 50); "grid_kib" -1 or 1..4194304 (the filter is never
 * smaller than 4 KiB); a value outside them -> SK_E_ARG and the option keeps what it had.  A union (sk_union_create) takes both from its
 * first member: its table is sized to that member's "table_load_pct", its level-1 filter to that member's "grid_kib" times the
 * number of members. */
int sk_set_option(sk_ctx *ctx, const char *name, long value);

/* Device buffer helpers so that FFI callers need no HIP binding of their own. */
int sk_dev_alloc(sk_ctx *ctx, void **dev, uint64_t nbytes);
int sk_dev_free(sk_ctx *ctx, void *dev);
int sk_dev_upload(sk_ctx *ctx, void *dev, const void *host, uint64_t nbytes);
int sk_dev_download(sk_ctx *ctx, void *host, const void *dev, uint64_t nbytes);

/* ----------------------------------------------------------------------------------------
 * host layer (C): the reference's file semantics around the device layer
 * -------------------------------------------------------------------------------------- */

typedef struct skh_keyset {
    uint32_t  nrows;        /* distinct oriented keys, in OUTPUT (BIO_hash slot) order          */
    uint32_t  nwide;        /* how many of them are wide (non-ACGT bytes)                       */
    uint64_t *packed;       /* [nrows] canonical packed key or SK_KEY_NONE                      */
    uint32_t *first_count;  /* [nrows] column-0 value after the build phase                     */
    uint32_t *locality;     /* [nrows] first-occurrence rank of each row's key along the strain    */
    char     *wide_keys;    /* [nwide*32]                                                       */
    uint32_t *wide_rows;    /* [nwide]                                                          */
    uint32_t  final_slots;  /* M of the replayed reference table                                */
    uint64_t  short_records;/* records skipped because shorter than k-1 (reference crashes)     */
    uint32_t *text2;        /* the strain's bases, 2 bits each (sk_table_load_text)             */
    uint32_t  text_bases;   /* how many                                                         */
    uint32_t *first_pos;    /* [nrows] text position of the row's first all-ACGT occurrence, or UINT32_MAX */
} skh_keyset;

/* Build phase.  Reads a FASTA/FASTQ(.gz) strain file with the reference parser's grammar
 * (src/kseq.h:166-211), upper-cases, extracts every window's oriented key that contains no
 * 'N', de-duplicates in first-occurrence order with column 0 = default_val + incr*(repeats)
 * and replays BIO_hash's insertion/doubling (src/BIO_hash.c:39-61,129-139,208-216) from
 * `initial_slots` to put the rows in the reference's output order.
 * Replaces GEN_hash_sequences_set_count_vec(): src/genome_compare.c:967-1030. */
int  skh_keyset_from_file(skh_keyset *ks, const char *path, uint32_t initial_slots,
                          uint32_t default_val, uint32_t incr);
int  skh_keyset_from_stream(skh_keyset *ks, const char *stream, size_t nbytes,
                            uint32_t initial_slots, uint32_t default_val, uint32_t incr);
void skh_keyset_free(skh_keyset *ks);
/* Decode row r's key to 31 ASCII bytes + NUL. */
void skh_keyset_key(const skh_keyset *ks, uint32_t row, char out[32]);
/* Load a keyset into a context (sk_table_load + sk_table_load_wide + column 0). */
int  skh_keyset_load(sk_ctx *ctx, const skh_keyset *ks, uint32_t ncols);

/* Scan one FASTA/FASTQ(.gz) file into column `col`; *bases (may be NULL) accumulates the
 * sequence bytes seen.  Replaces GEN_calculate_kmer_count(): src/genome_compare.c:179-236. */
int skh_scan_file(sk_ctx *ctx, const char *path, uint32_t col, uint64_t *bases);

/* Walk a newline-separated file list.  `skip` (may be NULL): a line equal to it is not
 * scanned and "skipping %s (identical match)" goes to `err`.  `progress` (may be NULL) gets
 * "<line>\t<asctime>".  On an unreadable list or file the reference's message is written to
 * `err` and SK_E_OPEN returned (the progress file then ends with the unreadable file's line and no later
 * skip message is printed, as in the reference, which exits there).  With world > 1 the list's items -- files,
 * or byte ranges of big plain-text files -- are dealt to the ranks by size and this rank scans its own; rank 0
 * writes the progress file and the messages (world=1, rank=0 for the single-GPU program).
 * Replaces GEN_all_kmer_counts(): src/genome_compare.c:149-177 and
 * GEN_all_kmer_counts_skip_file(): src/genome_compare.c:115-146. */
int skh_scan_list(sk_ctx *ctx, const char *list_path, const char *skip, uint32_t col,
                  FILE *progress, FILE *err, uint32_t rank, uint32_t world, uint64_t *bases);
/* What happens when a big text file's cut does not hold (a piece does not end between two records: SK_E_SPLIT inside).  One
 * process, or ranks that are all in the context's communicator (sk_comm_init): nothing the caller sees -- the column is put
 * back on every rank and the list scanned again uncut, every rank returning the same status (two small agreements per list
 * scan, sk_comm_max_u64: the same sequence of collectives on every rank whatever fails where).  Ranks WITHOUT the library's
 * communicator (a caller that reduces through torch.distributed): SK_E_SPLIT comes back and the caller does the same steps
 * itself -- copy the column before, agree after, sk_counts_set + skh_scan_list_uncut on every rank (strainer2_amd/dist.py:
 * scan_list_sharded).  skh_scan_list_uncut = skh_scan_list over the plan without byte-range pieces (SK_NO_SPLIT=1). */
int skh_scan_list_uncut(sk_ctx *ctx, const char *list_path, const char *skip, uint32_t col,
                        FILE *progress, FILE *err, uint32_t rank, uint32_t world, uint64_t *bases);
/* skh_scan_list with PREVALENCE (new: kmer_scrub_count --prevalence; the rule is at sk_item_fold): column `col` ends bit for bit as
 * skh_scan_list leaves it, column `prev_col` gets, per row, the ITEMS of the list in which the row was seen at least min_count
 * times, and *items_out one record per item in list order.  An ITEM is a list line whose file was opened: the line equal to
 * `skip` is none (skipped with skh_scan_list's message), a file that cannot be opened fails the scan as it always did (SK_E_OPEN:
 * nothing is handed out); a line listed twice is two items; an empty file is an item of no bases.  items_out->n is the
 * denominator of the column.
 * How: the list is planned UNCUT (skh_scan_list_uncut's plan, whatever the world: an item is whole on one rank); every decode
 * thread owns an item slot (sk_item_slots: as many as the walk has threads), names it before each of its submits -- its helper
 * threads of a split .gz item, the cache-served path, the pack-cache fill and the device text path included -- and enqueues the
 * item's sk_item_fold when the item ends, whether it was served, parsed or failed part-way.  With several ranks the prevalence
 * columns ride sk_counts_allreduce like any column; the items' records are merged by ONE sk_comm_max_u64 per list (a cell is
 * non-zero on its owner only), issued by every rank behind the agreement that closes the scan.  The setting enters the plan
 * hash: ranks that disagree about it, about prev_col or about min_count leave with SK_E_PLAN.
 * SK_E_ARG: min_count 0, col == prev_col, no items_out.  SK_E_STATE: a build whose device layer has no item slots.
 * skh_prev_items_free releases what a call handed out (and zeroes the struct). */
typedef struct { uint32_t line;            /* 1-based line of the list file */
                 char *path; uint64_t bases, kmers_present, kmer_hits; } skh_prev_item;
typedef struct { skh_prev_item *item; uint32_t n; } skh_prev_items;
int  skh_scan_list_prevalence(sk_ctx *ctx, const char *list_path, const char *skip, uint32_t col, uint32_t prev_col, uint32_t min_count,
                              skh_prev_items *items_out, FILE *progress, FILE *err, uint32_t rank, uint32_t world, uint64_t *bases);
void skh_prev_items_free(skh_prev_items *items);
/* PREVALENCE over n contexts on one device from ONE decode of the list (new: kmer_scrub_count -S --prevalence=SUFFIX; the contexts
 * are the resident unions' own, sk_union_context).  skh_scan_list_many's walk with skh_scan_list_prevalence's slots, and the folds
 * left to the caller, so that this layer never names a union: every ctx[i] has `nslots` item slots already (sk_item_slots, made
 * once for all the lists); the list is planned uncut; under the lock that orders the submits a decode thread names its slot on
 * EVERY context before each of its submits -- on all the paths skh_scan_list_prevalence names --, and where its item ends, served,
 * parsed or failed part-way, it calls fold(user, slot, line) under the same lock: line is the item's 0-based list line, and the
 * caller enqueues each context's fold of that slot there (sk_union_item_fold: asynchronous) into record cells of its own.  At most
 * nslots decode threads run: a thread owns a slot, so with fewer slots than SK_THREADS the other items wait for one.  Every line
 * is an item (the per-strain -C rule is the caller's fold mask).  When the call returns the folds are enqueued, not done: the
 * caller waits for each context once (sk_sync).  *items_out: one entry per line in list order with line, path and bases;
 * kmers_present and kmer_hits are 0 (they are in the caller's cells).  A hook that fails makes its item fail with what it returned
 * (a negative SK_E_*).  SK_E_ARG: no hook, no slots, no items_out; SK_E_STATE: a device layer without item slots. */
typedef int (*skh_item_fold_fn)(void *user, uint32_t slot, uint32_t line);
int  skh_scan_list_many_prevalence(sk_ctx *const *ctx, uint32_t n, const char *list_path, uint32_t col, uint32_t nslots,
                                   skh_item_fold_fn fold, void *user, skh_prev_items *items_out, FILE *progress, FILE *err, uint64_t *bases);
/* skh_scan_list into n contexts on one device over ONE decode of the list (new: kmer_scrub_count -S feeds every resident union
 * from one walk): each chunk goes up once and is scanned into column `col` of every ctx[i] (sk_scan_pinned[_packed]_many; packed
 * or bytes is decided once per chunk, for all of them).  A cut that does not hold puts back the column of EVERY context before the
 * uncut rescan.  Progress lines, messages and *bases are written once; the communicator (world > 1) is ctx[0]'s.  n = 1 is
 * skh_scan_list. */
int skh_scan_list_many(sk_ctx *const *ctx, uint32_t n, const char *list_path, const char *skip, uint32_t col,
                       FILE *progress, FILE *err, uint32_t rank, uint32_t world, uint64_t *bases);
/* The list scan's packed input cache (new, opt-in; the reference decodes every list item in every run, src/genome_compare.c:179-236).
 * With a directory set, skh_scan_file and skh_scan_list[_uncut|_many] keep for every list item what its decode handed to the device
 * -- the chunks of the record stream in sk_pack_stream's form, DIR/<basename>.<hash of the realpath>.skp (strainer2_amd/csrc/
 * sk_pcache.h has the format) -- and a later run whose item has the same size and mtime reads that file instead of inflating, parsing
 * and packing the source.  Every byte a run prints is the same with the cache off, filled or served.  mode "rw" (default, NULL) writes
 * what is missing or stale, "ro" only reads.  An empty dir switches it off for ctx; dir and mode both NULL make ctx follow the
 * process-wide default again (and forget its counters: call it before sk_ctx_destroy, as the programs do -- settings and counters are
 * kept by the context's address); ctx NULL sets that default, which is SK_PACK_CACHE / SK_PACK_CACHE_MODE until somebody sets it and
 * again after skh_pack_cache_set(NULL, NULL, NULL) (kmer_scrub_count --pack-cache DIR sets it for the length of that call).  A
 * source that is missing, or that this process cannot open for reading, is scanned -- and fails -- exactly as without the cache,
 * whatever the directory holds for it.  Not cached (and counted so):
 * items the plan cuts into byte ranges, items the device text parser takes, any run with world > 1 (the option is ignored there).
 * A directory that cannot be used gives one warning on `err` and the scan goes on uncached; a cache file whose payload fails its
 * checksum fails the run (SK_E_CACHE, the file named on `err`): chunks before it were counted already.
 * skh_pack_cache_stats: list items since the last reset that were served from the cache, written to it, found stale (or cut short,
 * or of another version), and scanned without being cached; each may be NULL. */
int skh_pack_cache_set(sk_ctx *ctx, const char *dir, const char *mode);
int skh_pack_cache_stats(sk_ctx *ctx, uint64_t *served, uint64_t *written, uint64_t *stale, uint64_t *not_cached, int reset);
/* strain_detect's target cache (new, opt-in: strain_detect --target-cache DIR, also behind --detect; or SK_TARGET_CACHE=DIR;
 * SK_TARGET_CACHE_MODE=rw|ro).  The metagenomes strain_detect reads (-b/-c, -B) are kept, one file per target, as the chunks its
 * decode side handed on: the record stream in sk_pack_stream's form, packed on the device beside the scans, and every record's length
 * -- DIR/<basename>.<hash of the realpath>.skt (sk_pcache.h, version 2).  A later run whose target has the same size and mtime is
 * served from that file by one thread: no inflate, no parser threads.  Every byte a run prints or writes is the same with the cache
 * off, filled or served.  A switch of its own: SK_PACK_CACHE goes on meaning the -g list only, and both may name one directory.  A
 * directory that cannot be used gives one warning and the run goes on uncached; a stale, mis-sized or other-version file is a miss
 * (replaced in rw mode); a file that fails a checksum or a structure check fails the run with SK_E_CACHE, the file named on `err`.
 * Not written: targets the device text parser may take, a target with a record of 2^32 bases or more, one that was not read to its
 * end.  skh_target_cache_stats: the process's targets since the last reset (the programs own their contexts, so there is no ctx). */
int skh_target_cache_stats(uint64_t *served, uint64_t *written, uint64_t *stale, uint64_t *not_cached, int reset);
/* Hash of the work plan skh_scan_list(list, skip, .., world) follows (items, byte ranges, file sizes, owners): a function
 * of the list, the files and `world` (and of SK_SPLIT_BYTES / SK_NO_SPLIT) only, never of a rank's thread count.  With the
 * library's own communicator skh_scan_list compares it across ranks itself (SK_E_PLAN); a caller that reduces the counters
 * through a collective of its own (torch.distributed) compares this value first.  New (the reference is one process). */
int skh_list_plan_hash(const char *list_path, const char *skip, uint32_t world, uint64_t *hash);
/* The same plan, line by line: owner[i] = the rank that scans list line i, SKH_PLAN_SKIPPED for the line equal to `skip`,
 * SKH_PLAN_SHARED for a big plain-text file whose byte ranges go to several ranks; *nlines = lines in the list (owner[]
 * is filled up to `cap`). */
#define SKH_PLAN_SKIPPED 0xFFFFFFFFu
#define SKH_PLAN_SHARED  0xFFFFFFFEu
int skh_list_plan_owners(const char *list_path, const char *skip, uint32_t world, uint32_t *owner, uint32_t cap, uint32_t *nlines);

/* Print the TSV: src/kmer_scrub_count.c:134-156 (5 header names always; 4 or 5 fields). */
int skh_print_counts(sk_ctx *ctx, const skh_keyset *ks, FILE *out, int with_drug_column);

/* The whole program with the reference's argv contract (src/kmer_scrub_count.c:29-131).
 * Extra environment: SK_DEVICE (default 0).  Returns the process exit status. */
int skh_kmer_scrub_count_main(int argc, char **argv, FILE *out, FILE *err);
/* kmer_scrub_count -S <strains file> -A <list> -B <list> [-C <list>] [-p <progress>] (no -r; new): every line of the strains
 * file is  <reference genome> TAB <outfile>  (empty lines and lines starting with '#' are skipped), and every outfile gets
 * exactly what `kmer_scrub_count -r <genome> -A .. -B .. [-C ..]` writes on stdout (gzip when its name ends in .gz).  Up to
 * SK_UNION_MAX strains share one union table (sk_union_count_enable / sk_union_counts_fold), and all the unions that fit in
 * HBM are fed by ONE decode of the lists (skh_scan_list_many); a -C line equal to a strain's genome is taken back from that
 * strain alone.  Environment: SK_SCRUB_GROUP=1..32 (strains per union), SK_SCRUB_UNIONS=n (at most n unions per decode; 1 =
 * a decode per union), SK_SCRUB_HBM_MB=m (the free HBM the residency plan assumes), SK_SCRUB_NO_UNION=1 (a pass per strain);
 * with WORLD_SIZE/RANK the strain lines are dealt to the ranks round-robin (no collective).  With "--scrub <min_fraction> [--independent] --detect <strain_detect arguments>" a line is
 * <genome> TAB <informative outfile> TAB <hits outfile> [TAB <-g list>]: the informative outfile gets what `-r <genome> ...
 * --scrub f [--independent]` prints (step 2 on the resident counts), and the strains go on into step 3 (and 4) together through
 * skh_strain_detect_resident_many.  --scrub without --detect is refused.
 * With "--prevalence=SUFFIX [--prevalence-items=SUFFIX] [--prevalence-min-count m]" every strain also gets, from the same decode,
 * its prevalence table at <its outfile><SUFFIX> and its item records at <its outfile><items SUFFIX>: byte for byte what `-r <genome>
 * .. --prevalence=F --prevalence-items=G --prevalence-min-count m` writes to F and G (the rule is at sk_item_fold).  The union's
 * scans go into item slots of its own context, made once per decode, and sk_union_item_fold hands each item to the members; a -C
 * line equal to a strain's genome is masked out of that strain's fold (no item of that strain), so nothing is rescanned and taken
 * back.  "--scrub f --scrub-by prevalence --detect .." ranks step 2 by the prevalence columns.  The bare --prevalence stays refused
 * (one file name cannot serve many strains), as are output names that coincide once the suffixes are applied.  Everything the run
 * wrote without the words stays the same bytes.  Returns the exit status. */
int skh_kmer_scrub_count_multi_main(int argc, char **argv, FILE *out, FILE *err);

/* The whole strain_detect program with the reference's argv contract (src/strain_detect.c:61-158):
 * -r -a -o and one of -b [-c] [-t SE|PE|PEI] / -B, optional -g.  Messages the reference prints on
 * stdout go to `out`, stderr texts to `err`; the -o file is gzip (members compressed in parallel; the
 * decompressed bytes are the reference's).  Returns the exit status. */
int skh_strain_detect_main(int argc, char **argv, FILE *out, FILE *err);
/* The same on a strain that is ALREADY resident (the table of step 1 serves step 3): ctx holds its table,
 * loaded with at least 6 columns, *ks its key set -- both are taken over and released by the call --; informative_path is
 * what -a would name.  argv = the rest of a strain_detect command line (-B/-b/-c/-t/-g/-o, --coverage-depth ...), argv[0]
 * ignored; -r and -a are implied.  `kmer_scrub_count ... --scrub m --detect <those arguments>` runs the reference's
 * steps 1 to 3 (4 with --coverage-depth) in one process this way. */
int skh_strain_detect_resident(sk_ctx *ctx, skh_keyset *ks, const char *informative_path, int argc, char **argv, FILE *out, FILE *err);
/* The same for n strains at once, as strain_detect -S runs them (one decode of the targets, union tables, SK_SD_GROUP):
 * ctx[i] and ks[i] are strain i's, loaded with at least 6 columns (all are taken over and released by the call, whatever
 * happens); informative[i], hits[i], glist[i] are what its -a, -o, -g would name (glist, or glist[i], NULL: no -g).  argv =
 * strain_detect's command line WITHOUT -r, -a, -o, -S, -g (-B/-b/-c/-t, --coverage-depth with no file name, --min-kmer-hits),
 * argv[0] ignored.  hits == NULL: n is 1 and -o, -g come from argv -- skh_strain_detect_resident is that case.  Used by
 * `kmer_scrub_count -S <strains> ... --scrub m --detect <those arguments>`. */
int skh_strain_detect_resident_many(uint32_t n, sk_ctx **ctx, skh_keyset *ks, const char *const *informative, const char *const *hits,
                                    const char *const *glist, int argc, char **argv, FILE *out, FILE *err);

/* Record reader exposed for tests: decode `path` into the record stream, calling `sink` with
 * successive chunks (records separated by '\n'; a long record may be cut with a k-1 overlap).
 * Returns number of records, or SK_E_OPEN. */
typedef int (*skh_sink_fn)(void *user, const uint8_t *chunk, uint64_t nbytes);
int64_t skh_decode_file(const char *path, uint64_t chunk_bytes, skh_sink_fn sink, void *user,
                        uint64_t *bases);

/* ------------------------------------------------------------------------------------------------
 * Scrub filter: the consumer of the count table (reference scripts/kmer_scrub_filter.py, step 2 of
 * test/example.sh).  The count columns live on the device, either uploaded from a parsed table
 * (sk_filter_load) or taken straight from the counters a scan has just filled (sk_filter_load_counts:
 * the table never becomes text); the ranking the script does with a full sort is a radix selection
 * there.  A "row" is one k-mer of the strain; rows marked gone do not take part (the script's drug
 * scrub, :62-69) but still count towards the column sums, as their dictionary entries do in the script.
 * ---------------------------------------------------------------------------------------------- */
typedef struct sk_filter sk_filter;
int  sk_filter_create(sk_ctx *ctx, sk_filter **out);
void sk_filter_destroy(sk_filter *f);
/* Counts as the table's text carries them (signed: a counter >= 2^31 was printed negative by %d and is
 * "not > 0" to the script). */
int  sk_filter_load(sk_filter *f, const int64_t *pan, const int64_t *meta, const uint8_t *gone /* may be NULL */, uint64_t n);
/* Columns of the context's resident counters, in row order; drug_col < 0: no drug column, else rows
 * with a positive drug count are gone.  Replaces print_hash_counts + the script's parse (:164-201). */
int  sk_filter_load_counts(sk_filter *f, uint32_t pan_col, uint32_t meta_col, int32_t drug_col);
/* Sums and sizes of the script's pangenome_hash / metagenome_hash (positive entries only) (:91-106,204). */
int  sk_filter_sums(sk_filter *f, int64_t *pan_sum, int64_t *meta_sum, uint64_t *n_pan, uint64_t *n_meta, uint64_t *n_gone);
/* Value histogram of one column (0 = pan, 1 = meta) over its positive entries: hist[b] = #{v == lo + b}
 * for b < nbins, hist[nbins] = #{v >= lo + nbins}.  Feeds scrub_max_kmers' threshold walk (:30-58). */
int  sk_filter_hist(sk_filter *f, int which, int64_t lo, uint32_t nbins, uint64_t *hist /* nbins + 1 */);
/* joint_scrub (:87-137): remove the n_scrub rows with the largest max(pan/pan_sum, meta/meta_sum),
 * equal scores in row order.  out[r] = 1 for every row that is NOT in the result (gone before, or
 * removed now). */
int  sk_filter_joint(sk_filter *f, int64_t pan_sum, int64_t meta_sum, uint64_t n_scrub, uint8_t *out /* n */);
/* independent_scrub (:72-84): remove rows whose pan count exceeds pan_thr or meta count meta_thr. */
int  sk_filter_above(sk_filter *f, int64_t pan_thr, int64_t meta_thr, uint8_t *out /* n */);
/* SCRUB SWEEP, step 2 (new: kmer_scrub_filter --min_fraction_list, kmer_scrub_count --scrub f0,f1,...): the informative sets of one
 * strain at several min_fraction from one run.  The rule, for a list f[0] > f[1] > ... > f[F-1]:
 *   list      1 to SK_SCRUB_SWEEP_MAX = 16 numbers in [0, 1], strictly descending; an empty field, a duplicate, an ascending pair,
 *             more than 16 entries, a value outside [0, 1] or a field that is no number is refused.  A fraction is printed
 *             everywhere as the text the user gave.
 *   set q     the informative list a run at f[q] alone prints.  The sets are nested, set 0 the largest: in the joint mode rows
 *             leave in one fixed order (descending score, ties in row order) while 1 - (n + 1) / all > min_fraction, so a smaller
 *             fraction removes a longer prefix of the same order (:87-137); in the independent mode the walked thresholds do not
 *             decrease with the fraction (:30-58, :72-84); the drug scrub does not depend on it (:62-68).
 *   class     of a row: the number of q whose set holds it, 0 .. F.  By nestedness a row is in set q iff class >= q + 1.
 * The class bytes are built on the device and only they come back: out_class[r] for all n rows (rows gone before have class 0),
 * kept[q] = the size of set q.
 *   sk_filter_classes_joint: n_scrub[q] is joint_scrub's row count at f[q] and must not decrease along the list (SK_E_ARG);
 *   ties at a cut go in row order until the quota is used, as in sk_filter_joint.  On an error (a cut beyond the rows that take part
 *   among them) kept[] is all zero and out_class is not written.
 *   sk_filter_classes_above: the pair of thresholds per fraction; neither may increase along the list (SK_E_ARG). */
#define SK_SCRUB_SWEEP_MAX 16u
int  sk_filter_classes_joint(sk_filter *f, int64_t pan_sum, int64_t meta_sum, const uint64_t *n_scrub /* F */, uint32_t F,
                             uint8_t *out_class /* n bytes */, uint64_t *kept /* F */);
int  sk_filter_classes_above(sk_filter *f, const int64_t *pan_thr /* F */, const int64_t *meta_thr /* F */, uint32_t F,
                             uint8_t *out_class /* n bytes */, uint64_t *kept /* F */);

/* The script's command line (-s/--scrub_count_file, -l/--scrub_count_list, -m/--min_fraction,
 * -i/--independent): same stdout bytes, same exit status, the same "kept ..." lines on stderr.
 * New: --min_fraction_list f0,f1,... --classes_out FILE (both or neither, not with -m; refused with status 2 otherwise, and for a
 * bad list): the run is the run at --min_fraction f0, stdout and stderr byte for byte, and FILE (gzip if its name ends in .gz)
 * gets the class file:
 *   #min_fractions<TAB>f0,f1,...
 *   #post_scrub_kmers<TAB>n0,n1,...
 *   kmer<TAB>class          one line per row of class >= 1, in the order of the informative list
 * A run that fails (where the run at f0 fails) writes no class file. */
int skh_scrub_filter_main(int argc, char **argv, FILE *out, FILE *err);
/* Fused step 1 -> step 2: what the script would print for the table skh_print_counts would print,
 * computed from the resident counters (columns 1, 2 and, with_drug_column, 3). */
int skh_scrub_filter_resident(sk_ctx *ctx, const skh_keyset *ks, int with_drug_column, double min_fraction,
                              int independent, FILE *out, FILE *err);
/* ... from three other columns {pangenome, metagenome, drug} of the resident table (new: kmer_scrub_count --scrub-by prevalence
 * hands in the prevalence columns): what the script would print for a table with those columns in place of the counts */
int skh_scrub_filter_resident_cols(sk_ctx *ctx, const skh_keyset *ks, int with_drug_column, const uint32_t cols[3], double min_fraction,
                                   int independent, FILE *out, FILE *err);
/* ... at a list of fractions "f0,f1,..." (the scrub sweep above): the run at f0, and the class file to classes_path; 1 for a bad list */
int skh_scrub_filter_resident_sweep(sk_ctx *ctx, const skh_keyset *ks, int with_drug_column, const char *fraction_list,
                                    int independent, const char *classes_path, FILE *out, FILE *err);

/* ------------------------------------------------------------------------------------------------
 * Coverage / depth: the consumer of strain_detect's hit list (reference scripts/coverage_depth.py,
 * step 4 of test/example.sh).
 * ---------------------------------------------------------------------------------------------- */
/* Per sample s < nsamples: out_total[s] = number of (sample, key) pairs with that sample,
 * out_unique[s] = number of different keys among them.  Replaces the script's unique_kmers_by_metagenome
 * / kmer_depth_count_by_metagenome bookkeeping (:64-93).  Keys are any u64 but 2^64-1.  Synchronous. */
int sk_distinct_count(sk_ctx *ctx, const uint64_t *keys, const uint32_t *sample, uint64_t n, uint32_t nsamples,
                      uint64_t *out_unique, uint64_t *out_total);
/* The same for hit lists whose k-mer text is not a fixed-length ACGT word: id[i] < nids numbers line i's
 * joined string <sample><k-mer> (file order); a string counts once, for the sample of the first line showing it,
 * as the script's global dictionary has it.  Synchronous. */
int sk_first_seen_count(sk_ctx *ctx, const uint32_t *id, const uint32_t *sample, uint64_t n, uint32_t nids, uint32_t nsamples,
                        uint64_t *out_unique, uint64_t *out_total);
/* The same two numbers per strain WITHOUT a hit list (new): a coverage accumulator on the device, fed by the results a TALLY launch
 * leaves in HBM.  What it computes is what scripts/coverage_depth.py:62-129 computes from the lines src/strain_detect.c:443-626
 * prints, under this rule: in a run of read pairs in which every record, of PE1 and of PE2, has at least k bases, the reference
 * prints one line per informative hit of either mate, all lines of a pair carry total_kmer = h1 + h2 (the "all hits" tallies of
 * the two mates; h2 = 0 for single reads), and the script counts a line iff h1 + h2 > min_kmer_hits.  So per member (strain) and
 * target: total = log entries of pairs that pass ("depth"), unique = distinct rows among them ("coverage").  A "record" below is a
 * record of the batch (sk_batch_fill's rec_start); runs with a record shorter than k (it carries the previous read's tallies and
 * rows in the reference) are the caller's to replay on the host and hand in through sk_covacc_add_rows.
 *   sk_covacc_create: nmembers (1..4096) strains with nrows[m] table rows each; one u32 counter per row and member, zeroed, on ctx's
 *   device.  Errors of every call are reported through ctx (sk_last_error).  One caller at a time.
 *   sk_tally_collect_counts / sk_union_tally_collect_counts: collect a launch WITHOUT copying its sparse records or its hit log
 *   home -- only the counters cross the link (a union's launch sends its first 16384 records and log entries home with its
 *   counters; sk_union_tally_launch_ex with results_stay != 0 is the launch that does not).  The results stay addressable on the
 *   device until the next launch on that context / union, and the batch must stay filled as it is until then (its record starts
 *   are part of them).  sk_tally_fetch_held / sk_union_tally_fetch_held copy them home
 *   after all, in sk_tally_collect_sparse's / sk_union_tally_collect's form (the host's fallback).  The existing collect calls and
 *   what they return are unchanged.
 *   sk_covacc_add: fold the held results of ctx's launch (u NULL; they go to member `member0`) or of u's launch (the union's member
 *   i goes to member0 + i).  The run: npairs pairs, pair j's PE1 read is record a0 + j * astep of the launch.  mate NULL: single
 *   reads.  mate->held == 0: pair j's mate is record b0 + j * bstep of the SAME launch (interleaved pairs: a0, b0 = a0 + 1, both
 *   steps 2).  mate->held != 0: it is record b0 + j * bstep of the launch saved by sk_covacc_hold.  SK_E_STATE if the launch's hit
 *   log overflowed (launch again with more room first), SK_E_ARG for a run that leaves the batch.  Synchronous.
 *   sk_covacc_hold: copy the held results of a launch (device to device) into buffers the accumulator owns, so that the launch's
 *   context, union and batch may go on -- two-file pairs: hold PE1's launch, add PE2's with mate->held.  One launch is held at a time,
 *   and the add that uses it must name the same ctx / u / member0 kind of launch (same number of members).
 *   sk_covacc_add_rows: n hits on these rows of `member`, already filtered by the caller (host-replayed runs).
 *   sk_covacc_finish_target: out_unique[m] = rows of member m with a non-zero counter, out_total[m] = their sum; every counter is
 *   zero again afterwards (a second call returns zeros).  sk_covacc_rows: member's counters as they stand (tests). */
typedef struct sk_covacc sk_covacc;
typedef struct sk_covacc_mate { int held; uint32_t b0, bstep; } sk_covacc_mate;
int  sk_covacc_create(sk_ctx *ctx, uint32_t nmembers, const uint32_t *nrows, int64_t min_kmer_hits, sk_covacc **out);
void sk_covacc_destroy(sk_covacc *a);
int  sk_tally_collect_counts(sk_ctx *ctx, uint64_t *n, uint64_t *out_nhits);
int  sk_tally_fetch_held(sk_ctx *ctx, sk_tally_rec *out, uint64_t cap, sk_hit *out_hits);
int  sk_union_tally_launch_ex(sk_union *u, const sk_batch *b, uint64_t hits_cap, int results_stay);
int  sk_union_tally_collect_counts(sk_union *u, uint64_t *n, uint64_t *out_nhits);
int  sk_union_tally_fetch_held(sk_union *u, sk_tally_rec *out, uint64_t cap, sk_hit *out_hits);
int  sk_covacc_hold(sk_covacc *a, sk_ctx *ctx_or_null, sk_union *u_or_null);
int  sk_covacc_add(sk_covacc *a, sk_ctx *ctx_or_null, sk_union *u_or_null, uint32_t member0,
                   uint32_t a0, uint32_t astep, uint32_t npairs, const sk_covacc_mate *mate);
int  sk_covacc_add_rows(sk_covacc *a, uint32_t member, const uint32_t *rows, uint64_t n);
/* The few results the host still needs of a launch it folds on the device: sk_covacc_pick copies home, in the collect calls' form,
 * the sparse records and log entries of record 0 (first != 0) and of the last ntail records of the held launch of ctx / u
 * (from_hold != 0: of the launch sk_covacc_hold copied) -- the tallies and rows a run's last pair leaves to the read after it,
 * and a record whose mate sits in another batch.  *n / *out_nhits are what matched; more than cap / hits_cap: nothing was copied,
 * pick again with room.  sk_covacc_fetch_hold brings the whole launch last held home, in the same form and with the same rule
 * (a held launch whose mate's launch turns out not to be foldable).  An add that finds a log entry naming no row of its member
 * returns SK_E_STATE after the other entries were counted: the target's counters are then of no use (finish_target clears them). */
int  sk_covacc_pick(sk_covacc *a, sk_ctx *ctx_or_null, sk_union *u_or_null, int from_hold, int first, uint32_t ntail,
                    sk_tally_rec *out, uint64_t cap, uint64_t *n, sk_hit *out_hits, uint64_t hits_cap, uint64_t *out_nhits);
int  sk_covacc_fetch_hold(sk_covacc *a, sk_tally_rec *out, uint64_t cap, uint64_t *n, sk_hit *out_hits, uint64_t hits_cap, uint64_t *out_nhits);
/* strain_detect --coverage-only, process-wide like skh_target_cache_stats: runs (chunks of a target) folded on the device, runs
 * replayed on the host (a read shorter than k, a missing mate, pairs across two chunks or unaligned chunks of two files), and
 * targets counted by the host accumulator (two targets of the run share a basename). */
void skh_coverage_only_stats(uint64_t *runs_on_device, uint64_t *runs_replayed, uint64_t *targets_host_accumulated, int reset);
int  sk_covacc_finish_target(sk_covacc *a, uint64_t *out_unique /* nmembers */, uint64_t *out_total /* nmembers */);
int  sk_covacc_rows(sk_covacc *a, uint32_t member, uint32_t *out /* nrows[member] */);
/* The same two numbers per REGION of the strain's genome (new: strain_detect --coverage-regions).  The two numbers of a strain and
 * target cannot tell a strain that is present (hits all over the genome) from a sample that carries one mobile element of it
 * (every hit on one plasmid, phage or island); the numbers per region can.  The rule:
 *   text     the strain's text is what both key-set builders use: the records of the strain file with at least k - 1 = 30 bases, in
 *            file order, end to end.
 *   record   records are numbered from 1 over EVERY record of the file, the skipped short ones included.
 *   region   each kept record is cut into windows of W bases: region j of a record holds its bases [jW, min((j + 1)W, len)); W = 0:
 *            one region per record.  Regions are numbered in text order.
 *   a row's region is the one that holds the FIRST base of the row's first occurrence along the text, on either strand (its
 *            first_pos): a 31-mer that starts on the last base of a window belongs to that window, a k-mer that occurs in two
 *            records to the first.
 *   unplaced rows without a text position (0xFFFFFFFF: byte-string keys of a strain with U or IUPAC letters, every row of a strain
 *            too long for the text stage) go to one extra region, the last: index nregions.
 *   limit    a strain has at most SKH_REGIONS_MAX regions.
 * skh_regions_from_file: the region table of a strain file (FASTA/FASTQ, plain or .gz; the record grammar of every other reader
 * here): per region its offset in the text, its record's number and name (the header up to the first white space), its offset in
 * the record and its length.  SK_E_OPEN: unreadable; SK_E_ARG with out->too_many set: more than SKH_REGIONS_MAX regions.
 * skh_regions_free releases it (and zeroes it).
 * sk_table_first_pos: every row's first text position as the table on the device has it, in the caller's row order, 0xFFFFFFFF for
 * none -- for a table of sk_table_build_from_text (rows in strain order, positions from the rank map) and one of sk_table_load_ex +
 * sk_table_load_text (any row order, through the locality permutation) alike; a table without a text stage has no positions.
 *   sk_covacc_set_regions: member's rows are the rows of ctx's table (same device, same row count); each row is mapped to the last
 *   region whose start is at or before its first position (region_start[]: nregions text offsets, ascending), rows without one to
 *   region nregions.  One u32 per row is kept.  A member whose regions were never set has nregions = 0: all its rows are unplaced.
 *   sk_covacc_region_rows: per region of member (nregions + 1 entries) its rows and those of them whose counter in column type_col
 *   of ctx's table equals informative_value -- the denominator of the ratios.
 *   sk_covacc_finish_target_regions: sk_covacc_finish_target, and in the same sweep of the counters every non-zero row adds 1 and
 *   its count to its region's pair: reg_unique / reg_total hold nregions[m] + 1 entries per member, member after member.  The
 *   members' sums over their regions are out_unique / out_total.  Every counter is zero afterwards. */
#define SKH_REGIONS_MAX (1u << 20)
typedef struct skh_regions {
    uint32_t  n;            /* regions, in text order                                          */
    uint32_t  nnames;       /* kept records                                                    */
    uint64_t  text_bases;   /* length of the text                                              */
    uint64_t *text_off;     /* [n] offset of the region's first base in the text               */
    uint32_t *record;       /* [n] number of its record in the file, from 1                    */
    uint64_t *rec_off;      /* [n] offset of its first base in the record                      */
    uint64_t *len;          /* [n] its bases                                                   */
    char    **name;         /* [n] its record's name (regions of a record share the string)    */
    char    **names;        /* [nnames] the strings themselves                                 */
    int       too_many;     /* set when the call failed for more than SKH_REGIONS_MAX regions  */
} skh_regions;
int  skh_regions_from_file(const char *path, uint64_t window, skh_regions *out);
void skh_regions_free(skh_regions *r);
int  sk_table_first_pos(sk_ctx *ctx, uint32_t *out /* nrows */);
int  sk_covacc_set_regions(sk_covacc *a, uint32_t member, sk_ctx *ctx, const uint32_t *region_start, uint32_t nregions);
int  sk_covacc_region_rows(sk_covacc *a, uint32_t member, sk_ctx *ctx, uint32_t type_col, uint32_t informative_value,
                           uint64_t *out_rows /* nregions + 1 */, uint64_t *out_informative /* nregions + 1 */);
int  sk_covacc_finish_target_regions(sk_covacc *a, uint64_t *out_unique /* nmembers */, uint64_t *out_total /* nmembers */,
                                     uint64_t *reg_unique /* sum of nregions[m] + 1 */, uint64_t *reg_total);
/* The DEPTH SPECTRUM (new: strain_detect --coverage-spectrum, coverage_depth --spectrum): per strain and target, how many
 * informative k-mers were seen 0, 1, 2, ... times.  kmer_coverage and kmer_depth do not say how the depth is distributed: a strain
 * present at mean depth L has its informative k-mers around L and about e^-L of them unseen; a related strain, a shared mobile
 * element or a few conserved high-copy k-mers leave most at depth 0 and a few very deep, with the same kmer_depth.  The rule, for a
 * strain, a sample and a maximum depth D (--spectrum-max, 1 <= D <= SK_COVACC_SPECTRUM_MAX = 1023, default 255):
 *   sample    a target's basename, as in the script.
 *   depth of a row = the number of hit lines on that row that pass the script's read filter (total_kmer > min_kmer_hits): what
 *             sk_covacc's counter holds before the sweep, and the number of times the host accumulator's list holds (sample, row).
 *   n[d]      for 1 <= d <= D: rows with depth exactly d.       n[>D]: rows with depth above D.
 *   hits[d]   = d * n[d].                                        hits[>D]: the sum of the depths above D (u64).
 *   n[0]      = I - sum over d >= 1 of n[d], hits[0] = 0; I = the strain's informative rows, the value of the
 *             total_genome_informative_kmers trailer.  Only informative rows are ever logged, so the host subtracts and no device
 *             pass over the type column is needed.
 *   invariants  the n[d] with d >= 1 sum to unique_observed_informative_kmers and the hits to total_observed_informative_kmers of
 *             the main table's line for that sample.
 *   table     a header line, then one line per sample and non-empty bin, samples in the main table's order; the 0 line is
 *             printed whenever I is known, even when its count is 0.  All columns are integers:
 *               strain_name<TAB>metagenome<TAB>depth<TAB>informative_kmers<TAB>observed_hits
 *             depth is 0, 1, ..., D, then >D.
 * sk_covacc_set_spectrum: 0 turns the spectrum off (the state after create), 1..SK_COVACC_SPECTRUM_MAX turn it on with that D;
 * anything else is SK_E_ARG.  sk_covacc_finish_target and sk_covacc_finish_target_regions return what they return without it.
 * sk_covacc_finish_target_spectrum: sk_covacc_finish_target, and the same one sweep of the counters (they are zero afterwards)
 * yields every member's spectrum -- spec[m * (D + 1) + d - 1] = n[d] for d <= D, spec[m * (D + 1) + D] = n[>D], deep_total[m] =
 * hits[>D] -- and, when reg_unique is not NULL, the region pairs of sk_covacc_finish_target_regions.  SK_E_STATE with the spectrum off.
 * sk_distinct_spectrum: sk_distinct_count with the spectrum of the keys' multiplicities per sample, same layout. */
#define SK_COVACC_SPECTRUM_MAX 1023u
int  sk_covacc_set_spectrum(sk_covacc *a, uint32_t max_depth);
int  sk_covacc_finish_target_spectrum(sk_covacc *a, uint64_t *out_unique /* nmembers */, uint64_t *out_total /* nmembers */,
                                      uint64_t *spec /* nmembers x (max_depth + 1): n[1..D], n[>D] */, uint64_t *deep_total /* nmembers: hits[>D] */,
                                      uint64_t *reg_unique /* NULL: no regions */, uint64_t *reg_total);
int  sk_distinct_spectrum(sk_ctx *ctx, const uint64_t *keys, const uint32_t *sample, uint64_t n, uint32_t nsamples, uint32_t max_depth,
                          uint64_t *out_unique, uint64_t *out_total, uint64_t *spec /* nsamples x (max_depth + 1) */, uint64_t *deep_total);
/* RECURRENCE (new: strain_detect --coverage-recurrence [--recurrence-pairs], coverage_depth --recurrence [--recurrence-pairs]): which informative k-mers of a strain were seen in sample
 * after sample of one run.  Every other number here is per (strain, sample); two cases with the same numbers per sample differ
 * across samples: a strain present at low depth shows another random subset of its informative k-mers in every sample (the union
 * grows, few are seen everywhere, few never), a relative, a shared plasmid or a handful of conserved k-mers shows the same subset
 * in every sample (a block seen in all T samples, the rest in none).  The rule, for a strain and the T samples of a run:
 *   sample    a target's basename, as in the script; T = the samples of the main coverage table, in its order.  Samples without a
 *             hit count in T.
 *   seen      a row is seen in a sample when its depth there is >= 1 after the script's read filter (total_kmer > min_kmer_hits):
 *             exactly the row set that unique_observed_informative_kmers counts.
 *   limits    1 <= T <= SK_RECUR_SAMPLES_MAX = 4096; the pair table takes T <= SK_RECUR_PAIRS_MAX = 256.
 *   n[m]      for 1 <= m <= T: the rows seen in exactly m samples.  n[0] = I - sum over m >= 1 of n[m]; I = the strain's informative
 *             rows (the total_genome_informative_kmers trailer), as the spectrum does it.
 *   shared[i][j]  for samples i <= j: the rows seen in both; shared[i][i] is sample i's unique column.
 *             either[i][j] = shared[i][i] + shared[j][j] - shared[i][j].
 *   invariants  sum of m * n[m] = sum of shared[i][i] = the sum of the main table's unique column; sum of n[m] over m >= 0 = I;
 *             shared is symmetric and shared[i][j] <= min(shared[i][i], shared[j][j]).
 *   tables    a header line each, all columns integers:
 *               strain_name<TAB>samples<TAB>seen_in<TAB>informative_kmers
 *             seen_in ascends, one line per non-empty m, the 0 line whenever I is known;
 *               strain_name<TAB>metagenome_a<TAB>metagenome_b<TAB>shared_informative_kmers<TAB>either_informative_kmers
 *             every i <= j, zeros included, i ascending, then j.
 * The engine works on generic bit planes: nmembers (1..SK_RECUR_MEMBERS_MAX) members of nbits[m] bits, nsamples planes, all zero
 * after create, on ctx's device; errors go through ctx (sk_last_error); one caller at a time; every call is synchronous.
 *   sk_recur_create: SK_E_ARG for nsamples of 0 or above SK_RECUR_SAMPLES_MAX.
 *   sk_recur_mark_bits: OR these bits of `member` into plane `sample`; duplicates are fine.  SK_E_ARG for a bit, member or sample
 *   out of range, and then nothing of the call is marked.
 *   sk_recur_finish: hist[m * (nsamples + 1) + k] = bits of member m set in exactly k planes (entry 0: in none); pairs (NULL: not
 *   wanted; SK_E_ARG with nsamples > SK_RECUR_PAIRS_MAX): pairs[(m * nsamples + i) * nsamples + j] = bits of member m set in planes i
 *   and j, symmetric, diagonal filled.  It reads only: it may be called again, and after more marks.
 *   sk_covacc_set_recurrence: build member's rank map from ctx's table (same device, same row count, the row order of
 *   sk_covacc_region_rows): a row whose counter in type_col equals informative_value gets its rank among the member's such rows,
 *   every other row 0xFFFFFFFF.  *out_informative = the number of such rows: the member's nbits.  One u32 per row of the
 *   accumulator is kept from the first call on; a member never set has no informative row.
 *   sk_covacc_mark_target: every row with a non-zero counter sets bit rank[row] of its member in plane `sample` of r; the counters
 *   are not changed (call it before the sweep that ends the target).  A non-zero row without a rank marks nothing and is counted in
 *   *out_stray.  SK_E_ARG when r's members or a member's nbits differ from what set_recurrence returned, when the devices differ or
 *   the sample is out of range.
 *   sk_distinct_recurrence: the two tables of a hit list of (sample, key) pairs, one member: hist[nsamples + 1] with entry 0 left 0
 *   (the list does not say how many keys there are), pairs NULL or [nsamples x nsamples].  Keys must not be 0xFFFFFFFFFFFFFFFF; the
 *   engine's limits and refusals. */
#define SK_RECUR_SAMPLES_MAX 4096u
#define SK_RECUR_PAIRS_MAX    256u
#define SK_RECUR_MEMBERS_MAX 65535u
typedef struct sk_recur sk_recur;
int  sk_recur_create(sk_ctx *ctx, uint32_t nmembers, const uint32_t *nbits, uint32_t nsamples, sk_recur **out);
void sk_recur_destroy(sk_recur *r);
int  sk_recur_mark_bits(sk_recur *r, uint32_t member, uint32_t sample, const uint32_t *bits, uint64_t n);
int  sk_recur_finish(sk_recur *r, uint64_t *hist /* nmembers x (nsamples + 1) */, uint64_t *pairs /* NULL, or nmembers x nsamples x nsamples */);
int  sk_covacc_set_recurrence(sk_covacc *a, uint32_t member, sk_ctx *ctx, uint32_t type_col, uint32_t informative_value,
                              uint32_t *out_informative);
int  sk_covacc_mark_target(sk_covacc *a, sk_recur *r, uint32_t sample, uint64_t *out_stray);
int  sk_distinct_recurrence(sk_ctx *ctx, const uint64_t *keys, const uint32_t *sample, uint64_t n, uint32_t nsamples,
                            uint64_t *hist /* nsamples + 1; entry 0 is left 0 */, uint64_t *pairs /* NULL or nsamples^2 */);
/* THRESHOLDS (new: strain_detect --coverage-thresholds, coverage_depth --thresholds): step 4's two numbers at several
 * min_kmer_hits from one pass.  In the reference the read filter of step 4 is chosen after the pass -- scripts/coverage_depth.py -m N
 * counts a hit line iff total_kmer_pe1 + total_kmer_pe2 > N (:89) and is run at several N over one hit list; --coverage-only
 * writes no hit list, so the choice would cost a pass per N.  The rule, for a strain, a sample and a list t[0] < t[1] < ...:
 *   list      1 to SK_COVACC_THRESHOLDS_MAX = 16 integers, 0 <= t <= 2^31 - 2, strictly ascending (--threshold-list t1,t2,...;
 *             default 0,1,2,3,5,10,20,50).  An empty field, a duplicate, a descending value, more than 16 entries or a value out of
 *             range is refused.
 *   sample    a target's basename, as in the script; the table's samples and their order are the main coverage table's.
 *   total[t]  the number of hit lines of step 3 whose pair has h1 + h2 > t.
 *   unique[t] the number of distinct k-mers (rows) those lines name.
 *             Exactly the main table's total_observed_informative_kmers and unique_observed_informative_kmers of a run with
 *             --min-kmer-hits t.  The run's own --min-kmer-hits still governs the main table and the regions, spectrum and
 *             recurrence tables, and need not be in the list.
 *   table     a header line, then for every sample one line per threshold, ascending, zeros included, all columns integers:
 *               strain_name<TAB>metagenome<TAB>min_kmer_hits<TAB>unique_observed_informative_kmers<TAB>total_observed_informative_kmers
 *   invariants  neither number increases with t; unique[t] <= total[t]; where the run's --min-kmer-hits is in the list, that line
 *             carries the main table's two numbers for the sample.
 * The class of a hit line is the number of thresholds its pair's total exceeds; total[t[q]] is the number of lines of class > q and
 * unique[t[q]] the number of rows with a line of class > q, so the accumulator keeps the lines per class and every row's highest
 * class: one u32 per accumulator row from the first sk_covacc_set_thresholds on, whatever the list's length.
 *   sk_covacc_set_thresholds: n = 0 turns thresholds off (the state after create); otherwise the list is checked by the rule above
 *   (SK_E_ARG).  It may be called between targets; whatever was classified since the last finish is discarded.
 *   sk_covacc_add with thresholds on classifies every log entry of the run by its pair's total: the entry counts for the main
 *   counters iff the total exceeds min_kmer_hits, as ever, and for threshold q iff it exceeds t[q] -- whichever of the two is lower.
 *   sk_covacc_add_rows_hits: n host-replayed hits on these rows of `member`, NOT filtered, each with its pair's total h1 + h2, under
 *   the same rule for the main counters and the thresholds (thresholds off: the main counters only).  With thresholds on the
 *   filtered sk_covacc_add_rows returns SK_E_STATE: its rows carry no totals.
 *   sk_covacc_finish_target_thresholds: thr_unique[m * n + q], thr_total[m * n + q] for the list's n thresholds.  A pass of its own
 *   in front of whichever sweep ends the target, as sk_covacc_mark_target is: it changes no depth counter, so the three sweeps
 *   return what they return without it; the threshold state is zero afterwards (a second call returns zeros).  SK_E_STATE with
 *   thresholds off.
 *   sk_distinct_thresholds: the same two numbers per sample and threshold ([nsamples x nt]) for a hit list of (sample, key, total)
 *   triples; keys as for sk_distinct_count. */
#define SK_COVACC_THRESHOLDS_MAX 16u
int  sk_covacc_set_thresholds(sk_covacc *a, const int64_t *t, uint32_t n);
int  sk_covacc_add_rows_hits(sk_covacc *a, uint32_t member, const uint32_t *rows, const uint32_t *total_hits, uint64_t n);
int  sk_covacc_finish_target_thresholds(sk_covacc *a, uint64_t *thr_unique /* nmembers x n */, uint64_t *thr_total /* nmembers x n */);
int  sk_distinct_thresholds(sk_ctx *ctx, const uint64_t *keys, const uint32_t *sample, const uint32_t *total_hits, uint64_t n,
                            uint32_t nsamples, const int64_t *t, uint32_t nt, uint64_t *out_unique /* nsamples x nt */,
                            uint64_t *out_total /* nsamples x nt */);
/* SCRUB SWEEP, step 4 (new: strain_detect --coverage-scrub-sweep, coverage_depth --scrub-sweep): step 4's numbers at every fraction
 * of a class file (above) from the one pass made with set 0.  Step 4's read filter uses the reads' hits on ALL k-mers of the strain
 * (scripts/coverage_depth.py:84-89), which the informative set does not change, so a row's depth counter in the run at f[0] is what
 * it would be in a run at f[q] for every q whose set holds the row: the numbers at q are sums over the rows of class >= q + 1,
 * exactly those of a separate run.  A -g list breaks this (its cut is sized by the number of informative rows) and is refused.
 *   table     a header line, then per sample of the main coverage table, in its order, one line per fraction, descending, zeros
 *             included, all numbers integers; genome_num_informative_kmers is the size of set q:
 *               strain_name<TAB>metagenome<TAB>min_fraction<TAB>genome_num_informative_kmers<TAB>unique_observed_informative_kmers<TAB>total_observed_informative_kmers
 *   sk_covacc_set_classes: member's class bytes from a sparse list: rows[i] gets cls[i] (1 .. ncls), rows not named class 0.  A row
 *   or a class out of range is SK_E_ARG before anything is launched; a row named twice keeps one of its classes, which one is not
 *   defined (the programs refuse such a class file).  ncls = 0 turns the member's classes off (n must be 0).
 *   sk_covacc_finish_target_classes: out_unique[m * F + q], out_total[m * F + q], F = the largest ncls set (members with fewer, or
 *   none, have zeros beyond theirs).  A pass of its own in front of whichever sweep ends the target: it reads the depth counters and
 *   the class bytes and changes no counter; two calls return the same numbers and the sweeps return what they return without it.
 *   *out_stray = non-zero rows of class 0 or of a class above their member's ncls, members without classes not counted (the
 *   programs treat a non-zero count as an internal error).  SK_E_STATE when no member has classes.
 *   sk_distinct_classes: the same two numbers per sample and fraction ([nsamples x ncls]) for a hit list of (sample, key, class)
 *   triples with class 1 .. ncls (SK_E_ARG otherwise); the lines of a (sample, key) pair carry one class; keys as for
 *   sk_distinct_count. */
int  sk_covacc_set_classes(sk_covacc *a, uint32_t member, const uint32_t *rows, const uint8_t *cls, uint64_t n, uint32_t ncls);
int  sk_covacc_finish_target_classes(sk_covacc *a, uint64_t *out_unique /* nmembers x F */, uint64_t *out_total /* nmembers x F */,
                                     uint64_t *out_stray);
int  sk_distinct_classes(sk_ctx *ctx, const uint64_t *keys, const uint32_t *sample, const uint8_t *cls, uint64_t n, uint32_t nsamples,
                         uint32_t ncls, uint64_t *out_unique /* nsamples x ncls */, uint64_t *out_total /* nsamples x ncls */);
/* SUPPORT (new): the READ PAIRS behind step 4's numbers, per strain and across the strains of a panel.  Every other table here counts
 * k-mers; 500 counted lines can be 500 pairs of one hit or 10 pairs of 50, and a strain whose lines come from pairs that also support
 * a sibling of its panel is a relative of both or a chimera, not either strain (after a -C scrub the informative sets of two panel
 * strains are disjoint).  The reference never built this view (the commented-out --read_hits_file of scripts/coverage_depth.py).
 * The rule, for one strain m and a target whose pairs are numbered j = 0, 1, ... in file order (single reads: a pair is a read):
 *   the reference's read loop (src/strain_detect.c:443-626) refreshes the tallies h (all hits) and i (informative hits) of every
 *   read with at least k bases; a shorter read keeps the tallies and rows of the read before it.  If h1 + h2 >= 1 and i1 + i2 >= 1 it
 *   prints the PE1 read's informative rows, then, if the PE2 read is valid, that read's; every line carries h1 + h2 and the script
 *   counts a line iff h1 + h2 > min_kmer_hits.
 *   emission    one pass of pair j through that point that prints L >= 1 lines, all of them counted.  A short read re-emits the rows
 *               of the read before it: that counts as an emission, so that `lines` stays equal to step 4's total.
 *   supporting_pairs[m]  the number of emissions of m.
 *   lines[m]             the sum of L over them: total_observed_informative_kmers of the main table's line.
 *   both_mates[m]        emissions in which the PE1 part and the PE2 part each printed at least one line; 0 for single reads.
 *   group       the strains that share one launch (a union's members; a single context is a group of one).  For a, b of one group:
 *   shared_pairs[a][b]   pairs j at which both a and b have an emission (symmetric);
 *   lines_a[a][b]        the sum of a's L over those pairs (not symmetric);
 *   exclusive_pairs[a], exclusive_lines[a]   emissions of a at pairs where no other strain of the group has one, and their L: the
 *               diagonal [a][a] of the two matrices.  Strains of different groups are not compared: their cells are zero.
 *   invariants  supporting_pairs[a] >= exclusive_pairs[a]; shared_pairs[a][b] <= min(supporting_pairs[a], supporting_pairs[b]);
 *               lines_a[a][b] <= lines[a]; both_mates[a] <= supporting_pairs[a] <= lines[a].
 *   tables      strain_detect --coverage-support[=FILE] (with --coverage-depth or --coverage-only; default FILE the -o path with
 *               ".kmer_hits.gz" replaced by ".coverage_support") writes per strain a header line and one line per sample, in the
 *               order of the strain's main table (a sample is a target's basename; two targets with one basename are one sample; a
 *               sample without an emission has a line of zeros), all numbers integers:
 *                 metagenome<TAB>supporting_pairs<TAB>both_mates<TAB>lines
 *               --support-pairs=FILE (with --coverage-support and -S; one process, union tables) writes ONE file for the panel: a
 *               line "#group<TAB>g<TAB>strain names..." per group (the consecutive -S lines that share a union table: 32, or
 *               SK_SD_GROUP), a header line, then per sample (first appearance), strain a (-S order) and strain b of a's group:
 *                 metagenome<TAB>strain_a<TAB>strain_b<TAB>pairs<TAB>lines_a
 *               a != b: shared_pairs and lines_a, only where pairs > 0, both orders; a == b: exclusive_pairs and exclusive_lines,
 *               for every strain and sample, zeros included.  Strain names as in the coverage tables.  Strains of different groups
 *               are not compared and have no line.
 * In a run the device folds every read has k bases or more, so an emission of (j, m) is tot[j, m] > min_kmer_hits with
 * inf_1 + inf_2 >= 1 and L = inf_1 + inf_2 (the sparse records' third word): the fold needs nothing beyond the records.
 *   sk_covacc_set_support: on != 0 switches support on, 0 off (the state after create).  While it is off nothing of it is allocated
 *   and no fold or sweep launches a kernel it did not launch before; every other result of the accumulator is the same either way.
 *   At most SK_COVACC_SUPPORT_MEMBERS_MAX members (the matrices are nmembers x nmembers), and with support on sk_covacc_add takes
 *   launches of at most SK_UNION_MAX members (SK_E_ARG otherwise).  Rows handed in by sk_covacc_add_rows / sk_covacc_add_rows_hits
 *   carry no read identity and add nothing here: the emissions of replayed runs are the caller's to count.
 *   sk_covacc_finish_target_support: the numbers of the folds since the last call, all u64 -- out_pairs, out_lines, out_both per
 *   member; out_shared and out_lines_a as [nmembers x nmembers], row a, column b, zero outside a launch's members -- and the
 *   accumulators are zero afterwards (a second call returns zeros).  Independent of the sweeps.  SK_E_STATE while support is off. */
#define SK_COVACC_SUPPORT_MEMBERS_MAX 1024u
int  sk_covacc_set_support(sk_covacc *a, int on);
int  sk_covacc_finish_target_support(sk_covacc *a, uint64_t *out_pairs /* nmembers */, uint64_t *out_lines /* nmembers */,
                                     uint64_t *out_both /* nmembers */, uint64_t *out_shared /* nmembers x nmembers */,
                                     uint64_t *out_lines_a /* nmembers x nmembers */);
/* RAREFACTION (new): step 4's two numbers at nested subsamples of a target's read pairs, from the one pass -- how the distinct
 * informative k-mers grow with the number of pairs, which says whether a negative or borderline call was sequenced deeply enough.
 * With the reference this takes a subsample of the FASTQ and a rerun of steps 3 and 4 at every depth.  The rule:
 *   pair ordinal  i = the pair's 0-based position in the target in file order: -t PE the record index in the mate-1 file, -t PEI
 *             record index / 2, single-end the record index.  Every record counts, whatever its content: shorter than k, with N, or
 *             missing a mate.
 *   draw      x = (uint32)i ^ ((uint32)(i >> 32) * 0x9E3779B9u) ^ seed;
 *             x ^= x >> 16; x *= 0x85EBCA6Bu;  x ^= x >> 13; x *= 0xC2B2AE35u;  x ^= x >> 16;  u(i) = x   (all in 32 bits)
 *             seed is a u32, default 0 (--rarefaction-seed S).
 *   fractions 1 to SK_COVACC_RAREFACTION_MAX = 16 decimal fractions f0,f1,... with 0 < f <= 1, strictly descending
 *             (--rarefaction-list; default 1,0.5,0.25,0.125,0.0625,0.03125).  T[q] = (uint64)floor(strtod(f_q) * 4294967296.0): a
 *             double times 2^32 is exact, and int(float(s) * 4294967296.0) in Python gives the same value.  An empty field, a field
 *             that is no plain decimal number (digits, '.', an exponent), a value outside (0, 1], an order that does not descend, two
 *             fractions with equal T, more than 16 entries or a field of more than 39 characters is refused.
 *   subsample q   holds pair i iff u(i) < T[q].  The class of a pair is the number of q that hold it; the list descends, so the pair
 *             is in subsamples 0 .. class - 1, and the subsamples are nested.
 *   pairs[q]  the pairs of the target in subsample q.
 *   total[q]  the hit lines of step 3 that pass the run's --min-kmer-hits and whose pair is in subsample q.
 *   unique[q] the rows (informative k-mers) with at least one such line.
 *             A line belongs to the pair that printed it.  For a target whose records all have k bases or more and whose mates are
 *             all there, these are exactly step 4's two numbers for a run of the same program on a file that holds only the
 *             subsample's pairs, in order.  A record shorter than k, and a read without its mate, re-use the tallies (and a short
 *             PE1 read the rows) of the record before them (src/strain_detect.c:444), which in a subsample's file is another
 *             record: at such records a rerun can differ.  With f0 = 1, unique[0] and total[0] are the main table's numbers and
 *             pairs[0] is the target's pair count.
 *   table     strain_detect --coverage-rarefaction[=FILE] [--rarefaction-list ...] [--rarefaction-seed S] (with --coverage-depth or
 *             --coverage-only; default FILE the -o path with ".kmer_hits.gz" replaced by ".coverage_rarefaction"): a header line,
 *             then per target (its basename), in the run's order, one line per fraction in the list's order, zeros included, numbers
 *             integers, `fraction` the user's text; with -S every line begins with a column strain_name:
 *               metagenome<TAB>fraction<TAB>pairs<TAB>unique_kmers<TAB>total_hits
 * The accumulator keeps the counted lines per (member, class) and every row's highest class, as for the thresholds: one u32 per
 * accumulator row from the first sk_covacc_set_rarefaction on, whatever the list's length, plus [nmembers x 17] line bins, as many
 * row bins and 17 pair bins.
 *   sk_covacc_set_rarefaction: n = 0 turns rarefaction off (the state after create: nothing of it is allocated and no fold or sweep
 *   launches a kernel it did not launch before).  Otherwise T[0] > T[1] > ... and T[0] <= 2^32, at most 16 (SK_E_ARG).  It may be
 *   called between targets; whatever was classified since the last finish is discarded.
 *   sk_covacc_set_pair_base: the ordinal of pair 0 of the next sk_covacc_add's run (it stays until set again; 0 after create).
 *   sk_covacc_add with rarefaction on also classifies, in a pass of its own over each side's log, every entry whose pair's total
 *   exceeds min_kmer_hits by the class of pair first_pair + j, and counts the run's npairs pairs by class, once per run.  It writes
 *   no depth counter: the main counters, the thresholds and support are what they are without it.
 *   sk_covacc_add_rows_hits_pairs: sk_covacc_add_rows_hits, and each of the n unfiltered hits also carries its pair's ordinal and is
 *   classified by the same rule.  sk_covacc_add_pairs: pairs first .. first + n - 1 of the target counted by class (the pairs of
 *   replayed runs, which sk_covacc_add does not see).  Every pair of a target is to be counted exactly once.  Both are SK_E_STATE
 *   with rarefaction off.
 *   sk_covacc_finish_target_rarefaction: out_pairs[q], out_unique[m * n + q], out_total[m * n + q] for the list's n fractions.  A
 *   pass of its own in front of whichever sweep ends the target: it changes no depth counter; the rarefaction state is zero
 *   afterwards (a second call returns zeros).  SK_E_STATE with rarefaction off.
 * The host side (sk_host_rarefaction.c): skh_rarefaction_parse reads a list (NULL: the default) into T[] and keeps each field's
 * text; skh_rarefaction_draw and skh_rarefaction_class are the rule above; skh_rarefaction_fold is the table of one strain and
 * target from its hit lines as (pair ordinal, row < nrows, pair total) triples and the target's pairs first_pair .. first_pair +
 * npairs - 1 (SK_E_ARG for a row out of range); skh_rarefaction_write prints the header (metagenome NULL) or a sample's lines.
 * coverage_depth has no flag for this table: a hit list carries no pair ordinal. */
#define SK_COVACC_RAREFACTION_MAX 16u
#define SKH_RAREFACTION_DEFAULT "1,0.5,0.25,0.125,0.0625,0.03125"
typedef struct skh_rarefaction {
    uint32_t n, seed;
    uint64_t T[SK_COVACC_RAREFACTION_MAX];
    char     text[SK_COVACC_RAREFACTION_MAX][40];
} skh_rarefaction;
int  sk_covacc_set_rarefaction(sk_covacc *a, const uint64_t *T, uint32_t n, uint32_t seed);
int  sk_covacc_set_pair_base(sk_covacc *a, uint64_t first_pair);
int  sk_covacc_add_pairs(sk_covacc *a, uint64_t first, uint64_t n);
int  sk_covacc_add_rows_hits_pairs(sk_covacc *a, uint32_t member, const uint32_t *rows, const uint32_t *total_hits,
                                   const uint64_t *pair_ordinal, uint64_t n);
int  sk_covacc_finish_target_rarefaction(sk_covacc *a, uint64_t *out_pairs /* n */, uint64_t *out_unique /* nmembers x n */,
                                         uint64_t *out_total /* nmembers x n */);
int  skh_rarefaction_parse(const char *list_or_null, uint32_t seed, skh_rarefaction *out);
uint32_t skh_rarefaction_draw(uint64_t pair, uint32_t seed);
uint32_t skh_rarefaction_class(const skh_rarefaction *r, uint64_t pair);
int  skh_rarefaction_fold(const skh_rarefaction *r, int64_t min_kmer_hits, uint32_t nrows, const uint64_t *pair, const uint32_t *row,
                          const uint32_t *total_hits, uint64_t n, uint64_t first_pair, uint64_t npairs,
                          uint64_t *out_pairs /* r->n */, uint64_t *out_unique /* r->n */, uint64_t *out_total /* r->n */);
int  skh_rarefaction_write(FILE *f, const skh_rarefaction *r, const char *strain_or_null, const char *metagenome_or_null,
                           const uint64_t *pairs, const uint64_t *unique, const uint64_t *total);
/* The script's command line (-k/--kmer_hits_file, -m/--min_kmer_hits, -b/--background_metagenomes_file):
 * same stdout bytes and exit status.  New: --scrub-classes FILE --scrub-sweep[=FILE] also writes the scrub sweep table (above) to
 * FILE, default the hits file's path with a trailing ".kmer_hits.gz" replaced by ".coverage_scrub_sweep"; stdout is unchanged; a hit
 * list in the general mode, or one with a k-mer the class file does not name, is refused.  New: --thresholds[=FILE] [--threshold-list t1,t2,...] also writes the thresholds table (above)
 * to FILE, default the hits file's path with a trailing ".kmer_hits.gz" replaced by ".coverage_thresholds"; stdout is unchanged and a
 * hit list in the general mode is refused.  New: --spectrum[=FILE] [--spectrum-max D] also writes the depth spectrum (above) to FILE,
 * default the hits file's path with a trailing ".kmer_hits.gz" removed plus ".coverage_spectrum"; stdout is unchanged.  A hit list
 * in the general (non-ACGT text) mode is refused.  New: --recurrence[=FILE] [--recurrence-pairs[=FILE]] also writes the recurrence
 * tables (above), default paths with ".coverage_recurrence" and ".coverage_recurrence_pairs", under the same conditions. */
int skh_coverage_depth_main(int argc, char **argv, FILE *out, FILE *err);

#ifdef __cplusplus
}
#endif
#endif /* STRAINER_KMER_H */
