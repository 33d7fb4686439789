/* sk_internal.h -- entry points shared between the translation units of libstrainer_kmer.so; not part
 * of the C-ABI (include/strainer_kmer.h). */
#ifndef SK_INTERNAL_H
#define SK_INTERNAL_H
#include <stdint.h>
#include <stdio.h>
#include "../../include/strainer_kmer.h"
#ifdef __cplusplus
extern "C" {
#endif
#define SK_E_UNSUPPORTED -100
/* record a message for sk_last_error and hand back `code` */
int sk_fail_(sk_ctx *ctx, int code, const char *fmt, ...);
int sk_ctx_device_(const sk_ctx *ctx);
/* column `col` of the resident counters, in the caller's row order, into a device buffer of nrows u32;
 * complete on return */
int sk_counts_rows_to_device_(sk_ctx *ctx, uint32_t col, uint32_t *d_out);
/* sk_table_first_pos into a device buffer of nrows u32 on the context's device; complete on return */
int sk_table_first_pos_to_device_(sk_ctx *ctx, uint32_t *d_out);
/* coverage/depth accumulator of sk_host_cov.c, fed by strain_detect when steps 3 and 4 are fused */
typedef struct skc_acc skc_acc;
skc_acc *skc_create(int64_t min_hits);
void skc_destroy(skc_acc *a);
int skc_add_hit(skc_acc *a, const char *metagenome, int64_t hits_pe1, int64_t hits_pe2, uint32_t row);
int skc_add_counts(skc_acc *a, const char *metagenome, uint64_t unique, uint64_t total);
int skc_add_trailer(skc_acc *a, const char *metagenome, const char *name, int64_t value);
int skc_report(skc_acc *a, sk_ctx *ctx, const char *hits_file_name, FILE *out, FILE *err);
/* ... and per region of the strain's genome (strain_detect --coverage-regions): counts handed in per metagenome and region (next to
 * skc_add_counts), or folded from the hits by skc_report_regions, which prints the table; call it after skc_report */
int skc_add_region_counts(skc_acc *a, const char *metagenome, const uint64_t *unique, const uint64_t *total, uint32_t nbins);
int skc_report_regions(skc_acc *a, const char *hits_file_name, const skh_regions *rg, const uint32_t *row_region, uint32_t nrows,
                       const uint64_t *reg_inf, FILE *out, FILE *err);
/* ... and the depth spectrum (strain_detect --coverage-spectrum): a metagenome's bins handed in (nbins = max_depth + 1: n[1..D],
 * n[>D]; deep_total = hits[>D]; next to skc_add_counts), or folded from the hits by skc_report_spectrum, which prints the table;
 * call it after skc_report */
int skc_add_spectrum_counts(skc_acc *a, const char *metagenome, const uint64_t *spec, uint64_t deep_total, uint32_t nbins);
int skc_report_spectrum(skc_acc *a, const char *hits_file_name, uint32_t max_depth, FILE *out, FILE *err);
/* ... and recurrence over the run's samples (strain_detect --coverage-recurrence [--recurrence-pairs]): the run's tables handed in
 * once, by the caller's sample ordinals (hist[T + 1], entry 0 unused; pairs[T x T] or NULL; metagenome[i] names ordinal i, known to
 * the accumulator already), or folded from the hits by skc_report_recurrence, which prints both tables (out_pairs NULL: the first
 * alone); call it after skc_report */
int skc_add_recurrence_counts(skc_acc *a, const char *const *metagenome, uint32_t T, const uint64_t *hist, const uint64_t *pairs);
int skc_report_recurrence(skc_acc *a, const char *hits_file_name, FILE *out, FILE *out_pairs, FILE *err);
/* ... and the two numbers at several thresholds (strain_detect --coverage-thresholds): skc_set_thresholds right after skc_create
 * (-1: a bad list, or hits were added already) makes skc_add_hit also keep, in a list of its own and with its pair's total, every
 * hit above t[0], whatever the main filter does with it; a metagenome's numbers handed in per threshold (next to skc_add_counts),
 * or folded from the kept hits by skc_report_thresholds, which prints the table; call it after skc_report.
 * skc_parse_threshold_list reads "t1,t2,..." by the rule of include/strainer_kmer.h: 0, or 1 and in `why` what is wrong */
int skc_parse_threshold_list(const char *text, int64_t *t /* SK_COVACC_THRESHOLDS_MAX */, uint32_t *n, char *why, size_t why_cap);
int skc_set_thresholds(skc_acc *a, const int64_t *t, uint32_t n);
int skc_add_threshold_counts(skc_acc *a, const char *metagenome, const uint64_t *unique, const uint64_t *total, uint32_t n);
int skc_report_thresholds(skc_acc *a, const char *hits_file_name, FILE *out, FILE *err);
/* support on the host (sk_host_support.c; include/strainer_kmer.h has the rule): a run's numbers per sample and strain.
 * sks_create: `group` consecutive strains form a group (1: no strain is compared with another).  sks_sample: the sample of a target's
 * path, made at first sight; call it once per target, before anything is added for it (-1: out of memory).  It takes no lock (it
 * counts the targets and may move the samples): no sks_merge or sks_add_device may be under way on another thread while it runs --
 * strain_detect drains its lanes at the end of every target, before the next target's sks_sample.  The other calls lock.  A replayed run's
 * emissions go into one sks_list per strain ({the run's pair number, lines, parts: 1 PE1 | 2 PE2}, pairs ascending) and
 * sks_merge adds all of them; sks_add_device adds what sk_covacc_finish_target_support returned for n strains from `first` on. */
typedef struct sks_em { uint32_t pair, lines, parts; } sks_em;
typedef struct sks_list { sks_em *e; uint32_t n, cap; } sks_list;
typedef struct sks_acc sks_acc;
sks_acc *sks_create(uint32_t nstrains, uint32_t group);
void sks_destroy(sks_acc *a);
int sks_sample(sks_acc *a, const char *metagenome);
int sks_list_push(sks_list *l, uint32_t pair, uint32_t lines, uint32_t parts);
void sks_list_free(sks_list *l);
int sks_merge(sks_acc *a, uint32_t sample, const sks_list *lists /* nstrains */);
int sks_add_device(sks_acc *a, uint32_t sample, uint32_t first, uint32_t n, const uint64_t *pairs, const uint64_t *lines, const uint64_t *both,
                   const uint64_t *shared /* n x n */, const uint64_t *lines_a /* n x n */);
int sks_write_support(const sks_acc *a, uint32_t strain, FILE *f);
int sks_write_pairs(const sks_acc *a, const char *const *names /* nstrains */, FILE *f);
/* ... and the scrub sweep (strain_detect --coverage-scrub-sweep, coverage_depth --scrub-sweep; include/strainer_kmer.h has the rule and
 * the class file's lines).  skc_classes_read reads a class file (gzip or plain): 0, or 1 and in `why` what is wrong -- a missing or
 * unreadable file, a header line missing or out of place, a bad fraction list, a line that is not kmer<TAB>class with class 1..F, or
 * set sizes that the lines do not add up to.  skc_set_classes right after skc_create hands the accumulator the fractions' texts and
 * the sets' sizes; a metagenome's numbers per fraction are handed in (next to skc_add_counts), or folded from the hits by
 * skc_report_classes (row_class[row] for the strain's nrows rows; a hit on a row of class 0 or above F is an error), which prints the
 * table; call it after skc_report. */
#define SKW_TEXT_MAX 48                          /* a fraction's text, terminator included (sk_sweep.h parses the lists) */
typedef struct {
    uint32_t F; char frac[SK_SCRUB_SWEEP_MAX][SKW_TEXT_MAX]; uint64_t size[SK_SCRUB_SWEEP_MAX];   /* the header lines */
    char *arena; uint64_t *off; uint8_t *cls; uint64_t n, arena_len;                    /* the k-mer lines: text at arena + off[i], class */
} skc_classes;
int skc_classes_read(const char *path, skc_classes *c, char *why, size_t why_cap);
void skc_classes_free(skc_classes *c);
int skc_set_classes(skc_acc *a, const skc_classes *c);
int skc_add_class_counts(skc_acc *a, const char *metagenome, const uint64_t *unique, const uint64_t *total, uint32_t F);
int skc_report_classes(skc_acc *a, const char *hits_file_name, const uint8_t *row_class, uint32_t nrows, FILE *out, FILE *err);
/* kmer_scrub_count --detect: the genome files of the strains the next skh_strain_detect_resident[_many] call adopts (it has no -r;
 * --coverage-regions reads the records' names and lengths from them).  The call takes the list and forgets it. */
void skh_resident_genomes_(const char *const *paths, uint32_t n);
/* strain_detect's key set built on the device (sk_host.c): SK_OK, the ctx holds the table and *ks the keys in row order; SK_E_UNSUPPORTED: a
 * strain with letters other than A/C/G/T/N (byte-string keys) or without a key -- the caller builds it on the host */
int skh_keyset_build_on_device(skh_keyset *ks, sk_ctx *ctx, const char *path, uint32_t ncols, uint32_t col0_value);
/* ... whose host list of keys (ks->packed) is filled in on demand: the keys of these rows now */
int skh_keyset_fetch_keys(skh_keyset *ks, sk_ctx *ctx, const uint32_t *rows, uint32_t n);
/* gzip on the device (sk_inflate.hip; experimental, SK_GPU_INFLATE=1).  SK_E_UNSUPPORTED: not a file this path takes, or a check failed --
 * the caller decodes it on the host as before. */
typedef struct sk_inflater sk_inflater;
int  sk_inflater_create(int device, sk_inflater **out);
void sk_inflater_destroy(sk_inflater *f);
const char *sk_inflater_error(const sk_inflater *f);
uint64_t sk_inflate_gz_size(const uint8_t *gz, uint64_t n);
int  sk_inflate_gz(sk_inflater *f, const uint8_t *gz, uint64_t n, uint8_t *host_text, uint64_t host_cap, uint64_t *text_len, uint32_t *trailer_crc);
/* A batch's buffers, for the text parser that fills it on the device (sk_text.hip: sk_batch_fill_text).  sk_batch_hook_ makes room for
 * a stream of stream_bytes and rec_words u32 of record starts + tile index (device and page-locked staging), waits for the batch's
 * stream and says where they are; `text`/`text_free`: the parser's own state of this batch, freed by sk_batch_destroy.
 * sk_batch_contents_: what the batch holds now (nrec 0: nothing to launch on). */
typedef struct sk_batch_hook {
    sk_ctx *owner;
    void *stream, *ready;              /* hipStream_t, hipEvent_t */
    void *d_stream; uint32_t *d_rec, *h_rec;
    void **text; void (**text_free)(void *);
} sk_batch_hook;
int  sk_batch_hook_(sk_batch *b, uint64_t stream_bytes, uint64_t rec_words, sk_batch_hook *out);
void sk_batch_contents_(sk_batch *b, uint64_t nbytes, uint32_t nrec);
/* ... and for the device pack of a batch's resident bytes (sk_packdev.hip: sk_batch_pack_home).  want_room != 0: SK_E_STATE unless the
 * batch holds bytes that came up as bytes; d_pack (batch-owned, 8-byte aligned) holds sk_packed_bytes(nbytes), d_odd one u32, `home` is
 * the event of the copy home.  The batch's stream is not waited for. */
typedef struct sk_batch_pack_hook {
    sk_ctx *owner;
    void *stream, *home;               /* hipStream_t, hipEvent_t */
    const void *d_stream; uint64_t nbytes;
    void *d_pack; uint32_t *d_odd;
} sk_batch_pack_hook;
int  sk_batch_pack_hook_(sk_batch *b, int want_room, sk_batch_pack_hook *out);
/* The results a launch left on the device (sk_tally_collect_counts / sk_union_tally_collect_counts), for the coverage accumulator
 * (sk_covacc.hip): d_recs = nrecs triples {record * max(members, 1) + member, all, informative}, d_hits = nhits log entries,
 * d_rec_start = the batch's nrec record starts.  members 0: a single context's launch (a log entry's row is the row itself).
 * SK_E_STATE when nothing is held or the log ran over. */
typedef struct sk_tally_view {
    sk_ctx *owner; int device; uint32_t members;
    const uint32_t *d_recs; uint64_t nrecs;
    const sk_hit *d_hits; uint64_t nhits;
    const uint32_t *d_rec_start; uint32_t nrec;
} sk_tally_view;
int sk_tally_view_(sk_ctx *ctx, sk_union *u, sk_tally_view *out);
/* the background tables on the host (sk_host_background.c): one strain's blocks as sk_background_finish / sk_union_background_finish
 * returned them, one per target in run order (skb_add copies SK_BACKGROUND_WORDS(max_depth) u64 and keeps the target's basename), and
 * the two tables; every call returns 0, or -1 (out of memory, a write that failed, a NULL) */
typedef struct skb_table skb_table;
skb_table *skb_create(uint32_t max_depth);
void skb_destroy(skb_table *t);
int skb_add(skb_table *t, const char *metagenome, const uint64_t *block);
uint32_t skb_targets(const skb_table *t);
int skb_write(const skb_table *t, const char *strain_name, FILE *f);
int skb_write_spectrum(const skb_table *t, const char *strain_name, FILE *f);
/* A count column and the type column beside it, as they lie on the device (both in the counters' own order, so row i of one is row i
 * of the other), for the background sweep (sk_background.hip).  Pending increments are folded in and both scan lanes joined before
 * this returns; the sweep runs on `stream` and leaves the column zero. */
typedef struct sk_background_view {
    int device; void *stream;              /* hipStream_t */
    uint32_t *d_col; const uint32_t *d_type; uint32_t nrows;
} sk_background_view;
int sk_background_view_(sk_ctx *ctx, uint32_t col, uint32_t type_col, sk_background_view *out);
/* An item slot and the two columns its fold adds to, as they lie on the device (all four in the counters' own order), for
 * sk_item_fold (sk_prevalence.hip).  Both scan lanes are joined before this returns and lane 1's next scan waits for what the caller
 * puts on `stream`.  d_diff holds nrows + 1 live entries, d_sums room for the block sums of that many (sk_diff_sums_). */
typedef struct sk_item_view {
    int device; void *stream;              /* hipStream_t */
    uint32_t *d_scratch, *d_diff, *d_sums, *d_count, *d_prev; uint32_t nrows;
} sk_item_view;
int sk_item_view_(sk_ctx *ctx, uint32_t slot, uint32_t count_col, uint32_t prev_col, sk_item_view *out);
/* An item slot of a union's context and what its fold needs of the union and its members, as they lie on the device, for
 * sk_union_item_fold (sk_prevalence.hip): the slot's pair and the block sums as in sk_item_view (global rows), canon[] (every global
 * row's key slot row), the members' first global rows (base[members] = nrows) and, for the members of member_mask, their two
 * columns (the others' are NULL).  Both scan lanes of the union's context are joined before this returns and lane 1's next scan
 * waits for what the caller puts on `stream`; a masked member's pending increments are flushed on its own stream and `stream`
 * waits for them on the device -- the host waits for nothing. */
typedef struct sk_union_item_view {
    sk_ctx *uc; int device; void *stream;  /* the union's context; hipStream_t */
    uint32_t *d_scratch, *d_diff, *d_sums; const uint32_t *d_canon; uint32_t nrows, members;
    uint32_t base[SK_UNION_MAX + 1];
    uint32_t *d_count[SK_UNION_MAX], *d_prev[SK_UNION_MAX];
} sk_union_item_view;
int sk_union_item_view_(sk_union *u, uint32_t slot, uint32_t count_col, uint32_t prev_col, uint32_t member_mask, sk_union_item_view *out);
/* skh_print_counts' table from columns from[0..3] of ctx (from[0]: the reference_count column), `extra` (or NULL) written behind
 * the header line: the prevalence table of kmer_scrub_count --prevalence */
int skh_print_table_cols_(sk_ctx *ctx, const skh_keyset *ks, FILE *out, int with_drug_column, const uint32_t from[4], const char *extra);
/* the block sums (one per 4096 entries) of a difference array of n entries and their exclusive scan in place, on ctx's stream */
int sk_diff_sums_(sk_ctx *ctx, const uint32_t *d_diff, uint32_t n, uint32_t *d_sums);
/* the device time of the item folds (sk_item_fold), from an event pair around each while the clocks are on: the call hands out the
 * sum and the number of the folds since the last call (ms / folds NULL: not wanted) and sets the clocks (on != 0: running).  Off
 * unless asked for: the list walk asks under SK_TIMING. */
int sk_item_fold_timing_(sk_ctx *ctx, int on, double *ms, uint64_t *folds);
/* the accumulator's device time (events around every fold and every target sweep): on != 0 starts the clocks, ms_fold / ms_sweep
 * (NULL: not wanted) are the sums so far.  Off unless asked for: strain_detect asks under SK_SD_TIMING. */
int sk_covacc_timing_(sk_covacc *a, int on, double *ms_fold, double *ms_sweep);
/* the device time of the accumulator's marks (sk_covacc_mark_target), kept by the same clocks */
int sk_covacc_mark_timing_(sk_covacc *a, double *ms_mark);
/* ... and of its threshold finishing passes (sk_covacc_finish_target_thresholds) */
int sk_covacc_thresholds_timing_(sk_covacc *a, double *ms_thr);
/* ... and of its class passes (sk_covacc_finish_target_classes) */
int sk_covacc_classes_timing_(sk_covacc *a, double *ms_cls);
/* ... and of support: the takes inside the folds (a part of ms_fold) and the copies home (sk_covacc_finish_target_support) */
int sk_covacc_support_timing_(sk_covacc *a, double *ms_take, double *ms_finish);
/* ... and of rarefaction: the classifying passes and pair counts inside the folds (a part of ms_fold) and the finishing passes */
int sk_covacc_rarefaction_timing_(sk_covacc *a, double *ms_class, double *ms_finish);
/* The recurrence engine's planes (sk_recur.hip), for the feeders that set bits with kernels of their own (sk_covacc.hip,
 * sk_cover.hip): plane `sample` of member m begins at d_planes + sample * words + word_base[m] and holds (nbits[m] + 63) / 64
 * words; a feeder sets no bit at or above nbits[m] and synchronises before the engine's next call. */
typedef struct sk_recur_view {
    int device; uint32_t nmembers, nsamples;
    const uint32_t *nbits;                 /* [nmembers], host */
    const uint64_t *word_base;             /* [nmembers + 1], host */
    const uint64_t *d_word_base;           /* the same on the device */
    unsigned long long *d_planes; uint64_t words;
} sk_recur_view;
int sk_recur_view_(sk_recur *r, sk_recur_view *out);
/* the device time of the engine's two sweeps (events around them in sk_recur_finish): on != 0 starts the clocks */
int sk_recur_timing_(sk_recur *r, int on, double *ms_hist, double *ms_gram);
#ifdef __cplusplus
}
#endif
#endif
