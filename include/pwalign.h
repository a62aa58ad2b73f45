/*
 * pwalign.h -- C ABI of the MI355X-native pairwise-alignment engine (libpwalign.so).
 *
 * Drop-in boundary for the DP hot path of the reference program
 *   /root/reference/Local_Global_Alignment/hw2.cpp
 * The reference has no FFI; its only callable surface for this path is the two C++ functions
 *   AlignmentResult* globalAlignmentNeedlemanWunsch(const string&, const string&, int, int, int)  hw2.cpp:118
 *   AlignmentResult* localAlignmentSmithWaterman  (const string&, const string&, int, int, int)  hw2.cpp:192
 * called once per pair from the loop at hw2.cpp:328-338.  Each entry point below names the
 * reference lines it replaces.  INTEGRATION.md shows the stub a maintainer of hw2.cpp would add.
 *
 * Conventions
 *   - plain pointers and sizes only; every buffer is caller-owned HOST memory unless the
 *     parameter name starts with d_ (then it is a DEVICE pointer on the context's GPU);
 *   - sequences are RAW BYTES compared for equality (hw2.cpp:142, 208): any alphabet, case-sensitive;
 *   - scores are int32 with the reference's recurrences and tie-breaks; results are bit-identical
 *     to hw2.cpp wherever hw2.cpp itself does not overflow int -- for ANY match / mismatch / gap: the fills with a
 *     traceback band keep H*4+priority keys while max|score| * (n + m + 2) <= 2^28 and switch to a plain int32
 *     compare-and-select form beyond that (slower, never refused);
 *   - every function returns PWA_OK (0) or a negative PWA_E_* code; nothing throws, exits or
 *     prints across the ABI; pwa_last_error() gives the text of the last failure on a context;
 *   - a context is bound to ONE GPU and is not thread-safe: one context per host thread.
 *   - there is NO CPU fallback: without a usable GPU pwa_ctx_create fails with PWA_E_NODEVICE.
 *
 * Engines (chosen by the library, never by the caller; all exact, so the choice changes no result):
 *   strip engine       scores only: lane = pair, register strips (batch_scores.hip.h);
 *   stripe engine      one wave per 64 RL rows of a pair, anti-diagonal front, stripes pipelined (pair_fill.hip.h): traceback fills
 *                      of long patterns, scores with end cells, and -- by estimated cost -- the scores of pairs that would leave the
 *                      strip engine's waves under-filled (a few long pairs);
 *   mini-stripe engine 16 lanes per pair, four pairs per wave (mini_fill.hip.h): traceback fills of patterns of up to 256 rows, and --
 *                      without a band -- the scores of such pairs when a scores pass routes them off the strips or asks for end cells.
 *   pwa_align_batch / pwa_overlaps pick the band geometry pair by pair; pwa_scores / pwa_batch_create split a list between the three
 *   engines by estimated cost.
 *
 * Environment switches (tests and diagnostics only).  They are read ONCE, by pwa_ctx_create, into the context; no other entry point
 * consults the environment, so a process that wants another setting creates another context.  (pwa_fasta_read, which has no context,
 * reads PWA_FASTA_MIN_CHUNK -- bytes per parser chunk -- on every call.)
 *   PWA_DEBUG, PWA_PROBE          host-side phase times / nop-kernel probes on stderr
 *   PWA_SCORES_ROUTE=0|1          scores passes: 0 every pair on the strip engine, 1 every pair on the stripe engine (default: by cost);
 *                                 distance passes in the two-value form likewise, for the pairs the stripe engine's distance fill takes;
 *                                 affine score passes likewise, for the lists the stripe engine's affine fill takes
 *   PWA_CELL16=0|1                local strip scores: 0 never / 1 always (where the batch admits it) the packed f16 cells, two pairs per
 *                                 lane (default: by estimated cost; pwa_batch_cell_bits says which form a batch runs)
 *   PWA_PROF16=0|1                packed f16 local strip scores: 0 never / 1 always (where the batch admits it) their profile form, one
 *                                 pattern against 128 texts per wave task (default: by estimated cost; pwa_batch_profile_form says which)
 *   PWA_PROF16_INT=0|1            the profile form's row step: 0 always the f16 row, 1 (and by default) the integer-coded row wherever the
 *                                 scoring admits it (mismatch >= gap and match >= gap; pwa_batch_profile_int says which)
 *   PWA_TB_ENGINE=0|2             traceback fills and scores off the strips: 0 the stripe engine's plain forms only, 2 mini-stripe kernels
 *                                 wherever they exist (default: by the list -- patterns of <= 256 rows, and of <= 1024 rows in batches)
 *   PWA_NO_PIPELINE, PWA_PIPE_RUNS=N  one-shot score calls: runs strictly one after the other / a list that fits one arena cut into N runs
 *   PWA_ARENA_LIMIT, PWA_LANE_ROWS_LIMIT   bytes per run of the one-shot calls / per-lane text rows per batch (force the multi-run paths)
 *   PWA_RANGE_BYTES               band + op bytes per range of pwa_align_batch / pwa_overlaps (forces several ranges on a small list);
 *                                 band bytes per chunk of pwa_align_affine_batch's stripe-engine pairs; wavefront + op bytes per range of
 *                                 pwa_scores_wfa / pwa_align_wfa_batch(_cigar) / pwa_align_wfa_codes_batch(_cigar) and the pwa_*_wfa_sg calls
 *   PWA_BANDED_RL=4|8             pwa_align_banded_batch(_cigar), pwa_scores_banded, their _subst forms and the pwa_extend_banded calls (with or without a table): every pair on stripes of 256 / 512 rows (default: by the pair's band width)
 *   PWA_OCC_CHUNK_HITS=N          pwa_sa_occurrences: at most N raw hits per chunk of patterns (forces several chunks on a small list);
 *                                 pwa_sa_seed: at most N worst-case hits per range of reads (forces several ranges on a small list);
 *                                 pwa_mm_seed: the same over the index's minimizers; pwa_mm_sketch: at most N k-mers per range of sequences;
 *                                 pwa_approx_occurrences: at most N hits staged on the device per slice of whole tasks;
 *                                 pwa_approx_starts: at most N hit records on the device per slice
 *   PWA_APPROX_CHUNK=N            pwa_approx_find / pwa_approx_occurrences: a task reports at most N text columns (default 4096)
 *   PWA_AFFINE_TB_ROUTE=0|1       pwa_align_affine_batch: 0 every pair on the strips, 1 every wave task of a list the stripe engine
 *                                 takes on the stripes (default: by estimated cost, and tasks whose strip band does not fit)
 *   PWA_POISON=<byte>             decimal or 0x.., 0 .. 255: every buffer the context hands to a call -- a new or regrown device
 *                                 allocation, a kept one that is reused, a page-locked staging buffer -- is filled with that byte over its
 *                                 whole capacity first (a blocking hipMemset between two device synchronises: slow, a test mode), so a
 *                                 call that reads what it did not write reads that byte, not zeros or the last call's values; a value
 *                                 that does not parse makes pwa_ctx_create fail with PWA_E_INVALID; pwa_ctx_poison_stats counts the fills
 *   PWA_NO_PAIR_TABLE, PWA_NO_KEYED_TB, PWA_NO_GAP_SHIFT, PWA_NO_TILED_OPS, PWA_NO_PACKED_DIST, PWA_FORCE_LANES,
 *   PWA_FORCE_R, PWA_FORCE_MODE, PWA_FORCE_RL, PWA_FORCE_W, PWA_WG_PER_CU, PWA_MINI_PER_CU, PWA_NO_LDS_PAD, PWA_STAMPS,
 *   PWA_TRACE_STRIPE
 *                                 select one of several equivalent kernel forms / geometries, or record time stamps
 */
#ifndef PWALIGN_H
#define PWALIGN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PWA_MODE_NW 0 /* global, hw2.cpp:118-190 (tie-break diag >= left >= up, 145-153)      */
#define PWA_MODE_SW 1 /* local,  hw2.cpp:192-265 (tie-break zero > diag > up > left, 214-222) */
/* Semi-global ("fitting", "glocal"): the WHOLE pattern against any substring of the text; the text's unaligned prefix and suffix
 * cost nothing.  An extension of the library: hw2.cpp has no such mode.  NW's recurrence and tie-break (diag >= left >= up) with
 *   dp[0][j] = 0 for all j (traceback ' '), dp[i][0] = i * gap for i > 0 ('u');
 *   end cell (n, j*): j* the SMALLEST j in 0..m with maximal dp[n][j]; score = dp[n][j*];
 *   the walk (NW's rules) runs from (n, j*) while i > 0 -- down column 0 ('D') if it reaches j = 0 first -- and stops at (0, j0):
 *   start_cell = (0, j0), text [j0, j*) is aligned.  n = 0: score 0, end = start = (0, 0), no ops; m = 0 < n: n * gap, n 'D'.
 * Scores of this mode run on the stripe / mini-stripe engines (never the strip kernels); pwa_overlaps does not take it. */
#define PWA_MODE_SG 2

#define PWA_OK 0
#define PWA_E_INVALID (-1)     /* bad argument (null pointer, unknown mode, index out of range) */
#define PWA_E_NODEVICE (-2)    /* no usable gfx950 device / HIP runtime                         */
#define PWA_E_HIP (-3)         /* a HIP call failed (text in pwa_last_error)                     */
#define PWA_E_NOMEM (-4)       /* host or device allocation failed                              */
#define PWA_E_CAPACITY (-5)    /* caller buffer too small / problem exceeds an index width       */
#define PWA_E_IO (-6)          /* a file cannot be opened or read (pwa_fasta_read)                */

typedef struct pwa_ctx pwa_ctx;
typedef struct pwa_batch pwa_batch;

/* Library / build identification: "pwalign <ver> gfx950". */
const char *pwa_version(void);
const char *pwa_strerror(int code);
/* Test hook, no GPU involved: runs the host scheduler's sorting helpers (stable counting sort, its multi-threaded form, the length
 * sort, the radix sort) on pseudo-random lists against std::stable_sort, and the range planner of the alignment batches (classes,
 * ranges, wave tasks, band layout) on pseudo-random length lists with made-up free-memory figures against the properties every plan
 * must have; the parser of PWA_POISON's value on a list of good and bad spellings; the cutting of a list into runs under a budget
 * (chunks of patterns, slices of tasks, ranges of WFA pairs) on its edge cases and on random lists; that every form of
 * pwa_pair_form_table resolves to kernels, to a fill of its own wherever a field the fill depends on differs, and to a walk that
 * follows from engine class, rows per lane, lanes, mode and walk alone; and the context's device-memory policy (slot reuse and
 * regrowth, the free list's best fit and caps, the parked hand-off buffer, the one retry after a failed allocation, teardown) over a
 * counting fake allocator.  Returns 0, or the number of the first check that failed. */
int pwa_selftest_host(uint32_t seed);

/* Context = one GPU (HIP device ordinal) + its streams and workspaces. */
int pwa_ctx_create(int device, pwa_ctx **out);
void pwa_ctx_destroy(pwa_ctx *ctx);
const char *pwa_last_error(const pwa_ctx *ctx);
/* When on, pwa_align / pwa_align_batch also materialise the int32 SCORE band in HBM next to the
 * traceback band (4 + 1 B/cell: the reference's own footprint, hw2.cpp:119-120 / 193-194), written as
 * one coalesced 64*RL*4-byte wave store per anti-diagonal step.  The walk does not need it; it exists
 * for inspection (pwa_align_matrices returns it) and for the 5 B/cell roofline accounting. */
int pwa_ctx_set_score_band(pwa_ctx *ctx, int on);
/* What PWA_POISON has filled on this context so far, as running totals: buffers, and their bytes (whole capacities).  The buffers
 * of a pwa_sa_index and of batch objects count on the context they were created on.  Zeros with the switch unset; a pointer may be
 * NULL.  PWA_E_INVALID on a NULL context. */
int pwa_ctx_poison_stats(const pwa_ctx *ctx, uint64_t *buffers, uint64_t *bytes);

/*
 * Scores of many pairs (the scores-only pass over hw2.cpp's pair loop 328-338; for -l the
 * reference selects the best pair from `result->score` alone, 352-356).
 *
 *   seq_bytes/seq_off : n_seq sequences, sequence s = seq_bytes[seq_off[s] .. seq_off[s+1])
 *   pair_a/pair_b     : pair k aligns pattern = sequence pair_a[k] (rows, hw2 "patterns")
 *                       against reference/text = sequence pair_b[k] (columns, hw2 "references")
 *   score_out[k]      : NW: dp[n][m] (hw2.cpp:186);  SW: max cell (hw2.cpp:225-229);  SG: max of row n (PWA_MODE_SG)
 *   end_i_out/end_j_out (each may be NULL): the cell the reference's traceback starts from --
 *                       NW (n, m); SW the FIRST maximum in row-major order, (0,0) if all zero; SG (n, j*), the first
 *                       maximum of row n.
 * Pair lists of any size: a batch object addresses its sequence arena with 32-bit offsets (4 GiB of distinct sequences),
 * so this call (like pwa_distances and pwa_scores_affine) cuts the list into runs of consecutive pairs whose sequences
 * fit one arena and PIPELINES them: run k + 1 is scheduled, coded and uploaded while the kernels of run k execute.  Remaining limits: a sequence < 2^31 - 64 symbols; pattern +
 * reference of ONE pair < 4 GiB; < 2^32 - 1 pairs per call.
 */
int pwa_scores(pwa_ctx *ctx, int mode, int match, int mismatch, int gap, const uint8_t *seq_bytes,
               const uint64_t *seq_off, uint32_t n_seq, const uint32_t *pair_a, const uint32_t *pair_b,
               uint64_t n_pairs, int32_t *score_out, uint32_t *end_i_out, uint32_t *end_j_out);

/*
 * The same pass split into prepare / run / fetch so that a caller can keep inputs resident in
 * HBM, time the kernels alone, and hand the device-side score vector to a collective
 * (RCCL all-gather over xGMI) without a host round trip.
 *   pwa_batch_create  uploads the sequences, builds the wave-task list (host), allocates outputs; PWA_E_CAPACITY when the
 *                     sequences the pair list uses exceed one 4 GiB arena (split the list, or call pwa_scores);
 *   pwa_batch_run     enqueues the kernels on `stream` (a hipStream_t, NULL = the context's own
 *                     stream) -- asynchronous, no host synchronisation, graph-capturable;
 *   pwa_batch_d_scores  device pointer to int32[n_pairs] in pair order (valid until destroy),
 *                     complete once the run has finished on its stream;
 *   pwa_batch_fetch   synchronises the stream and copies scores (and end cells, if requested at
 *                     create time) to host buffers.
 */
int pwa_batch_create(pwa_ctx *ctx, int mode, int match, int mismatch, int gap, const uint8_t *seq_bytes,
                     const uint64_t *seq_off, uint32_t n_seq, const uint32_t *pair_a, const uint32_t *pair_b,
                     uint64_t n_pairs, int want_end_cells, pwa_batch **out);
int pwa_batch_run(pwa_batch *b, void *stream);
int32_t *pwa_batch_d_scores(pwa_batch *b);
/* Redirect the score vector to caller-owned DEVICE memory (int32[n_pairs], e.g. a torch tensor's
 * data_ptr) so that it can be handed to a collective without aliasing library memory. */
int pwa_batch_set_d_scores(pwa_batch *b, int32_t *d_scores);
int pwa_batch_fetch(pwa_batch *b, int32_t *score_out, uint32_t *end_i_out, uint32_t *end_j_out);
/* Facts about the prepared batch for reporting: cells = sum n*m; padded_cells = cells the kernels
 * actually evaluate (register-tile padding); kernel_name = the dominant kernel instantiation. */
int pwa_batch_info(const pwa_batch *b, uint64_t *cells, uint64_t *padded_cells, uint64_t *n_tasks,
                   const char **kernel_name);
/* Cell form of the batch's register-strip launch: 16 = two pairs per lane in packed f16 cells, 32 = int32 cells (one pair per
 * lane), 0 = no pair runs on the strips.  The packed form is taken for local scores over patterns whose symbols are four of the
 * texts' (codes 0..3), with mismatch <= 0, gap <= 0, |scores| <= 127 and longest pattern * max(match, 0) <= 2047, when the cost
 * model prefers it; PWA_CELL16=0|1 forces either form where it applies. */
int pwa_batch_cell_bits(const pwa_batch *b);
/* 1 when the batch's strips run the profile form of the packed f16 cells (one pattern against 128 texts per wave task; PWA_PROF16=0|1
 * forces either form where it applies), 0 otherwise. */
int pwa_batch_profile_form(const pwa_batch *b);
/* 1 when that profile form runs its integer-coded row step (scores stored as integers, one 32-bit add per two cells; taken when
 * mismatch - gap >= 0 and match - gap >= 0 unless PWA_PROF16_INT=0), 0 otherwise.  Scores are the same either way. */
int pwa_batch_profile_int(const pwa_batch *b);
/* Host only, no context: the column-block loop of the profile form's integer row for one wave task.  blocks: the 8-column blocks
 * of a task whose longest text has max_text_len columns; interior_blocks: how many of them, from the first, prefetch their texts
 * with plain loads (whole words inside every text of the task, the shortest having min_text_len columns) -- the rest clamp the
 * word index and merge the pad code.  Scores do not depend on it. */
int pwa_profile_plan(uint32_t min_text_len, uint32_t max_text_len, uint32_t *interior_blocks, uint32_t *blocks);
/* Host only, no context: entry `index` of the table of instantiated register-strip kernels the scheduler picks from, and the number
 * of entries in *count (written whatever the index; any output pointer may be NULL).  name: the entry's part of pwa_batch_info's
 * kernel_name; rows: the strip height R; mode: its cell form (0 SW, 1 NW, 2 gap-shifted NW, 3 / 4 hw3 affine plain / shifted,
 * 5 / 7 hw4 distance plain / packed key, 6 saturating SW, 8 / 9 / 10 gotoh NW plain / shifted / SW); score_path: 0 coded symbols
 * with a byte table, 1 raw bytes compared; variants: which further kernels the entry carries beside its multi-strip one, as
 * PWA_STRIP_* bits.  PWA_E_INVALID when index >= *count.  For tests that want to reach every instantiation by name. */
#define PWA_STRIP_SINGLE 1u        /* every task a single strip: no hand-off rows */
#define PWA_STRIP_LANES 2u         /* every lane its own text (index-paired lists) */
#define PWA_STRIP_LANES_SINGLE 4u
#define PWA_STRIP_CELL16 8u        /* two pairs per lane in packed f16 cells */
#define PWA_STRIP_CELL16_SINGLE 16u
#define PWA_STRIP_PROF16 32u       /* ... their profile form */
#define PWA_STRIP_PROF16_INT 64u   /* ... with the integer-coded row */
int pwa_strip_table(uint32_t index, const char **name, int *rows, int *mode, int *score_path, uint32_t *variants, uint32_t *count);
/* The stripe and mini-stripe ("pair") engine's launches by name.  A launch of that engine is one value -- family, mode, band, walk,
 * cell form, rows per lane, compute waves (stripe families) or lanes per pair (mini families) -- and its name spells the seven fields:
 *   family/mode/band/walk/cells/rl<n>/w<n>      stripe_fill | stripe_dist | stripe_affine | stripe_affine_tb
 *   family/mode/band/walk/cells/rl<n>/ln<n>     mini_fill | mini_gotoh | mini_subst
 * with mode NW | SW | SG, band none | tb | tb+scores, walk none | ops | overlap, cells plain | keyed | coded | gap0; for example
 * stripe_fill/NW/tb/ops/coded/rl2/w4 or mini_subst/SG/none/none/keyed/rl16/ln64.
 * pwa_pair_form_table (host only, no context): entry `index` of the list of forms the library's call sites can build, and the number
 * of entries in *count (written whatever the index; any output pointer may be NULL).  PWA_E_INVALID when index >= *count.
 * pwa_pair_forms: the names of the forms this context has prepared launches of since the last pwa_pair_forms_reset -- distinct, in
 * first-seen order, joined by '\n', NUL-terminated.  A batch object's launches are prepared by its create call and count on the
 * context that created it.  *needed receives the size required (PWA_E_CAPACITY when cap is too small; call with cap = 0 to size the
 * buffer).  Nothing but pwa_pair_forms_reset empties the record, so a test brackets exactly the call it means; it never holds more
 * names than the table has entries.  For tests that want to reach every instantiation by name. */
int pwa_pair_form_table(uint32_t index, const char **name, uint32_t *count);
int pwa_pair_forms(const pwa_ctx *ctx, char *buf, uint64_t cap, uint64_t *needed);
int pwa_pair_forms_reset(pwa_ctx *ctx);
/* Device time of the most recent pwa_batch_run in ms (HIP events on the run's stream); the call
 * synchronises the run. */
int pwa_batch_last_ms(pwa_batch *b, float *ms);
/* Device times (ms, oldest first) of up to `cap` most recent runs (at most 64 are kept): each is
 * bracketed by HIP events recorded on the stream the kernels were enqueued on. */
int pwa_batch_run_times(pwa_batch *b, float *ms_out, int cap, int *n_out);
void pwa_batch_destroy(pwa_batch *b);

/*
 * Affine-gap global alignment SCORES of many pairs -- the score pass of the sibling program
 *   /root/reference/Multiple_Sequence_Alignment/hw3.cpp
 * i.e. `affine_alignment(Si, Sj, M, Mm, Go, Ge, &score)` (hw3.cpp:23-102) as called by the all-pairs
 * loop of the center-star MSA (hw3.cpp:232-241).  The recurrence is hw3's own three-matrix form with
 * its quirks (boundary gap of length L costs Go + Ge(L-1), interior gap Go + Ge*L; F never reads E and
 * E never reads F; result = max(V, F, E)[n][m]); it is NOT interchangeable with hw2's linear-gap NW.
 * pair (a, b): string1 = sequence a (rows), string2 = sequence b (columns).
 * The returned batch object works with pwa_batch_run / _d_scores / _set_d_scores / _fetch / _info /
 * _run_times / _destroy exactly like a linear-gap batch (no end cells).
 * Engines: the strip kernels (lane = pair) take every list; a list over at most 7 symbols (coded arena)
 * with (n + m + 2) * max(|M|, |Mm|, |Go| + |Ge|) < 2^28 is split by estimated cost between them and the
 * stripe engine's affine fill (a pair over many waves: few long sequences), like a scores pass;
 * PWA_SCORES_ROUTE=0 keeps every pair on the strips, =1 moves every pair of such a list.  A split batch
 * reports "<strip kernel> + <stripe kernel>".  pwa_scores_affine inherits the routing.
 */
int pwa_affine_batch_create(pwa_ctx *ctx, int match, int mismatch, int gap_open, int gap_extend, const uint8_t *seq_bytes,
                            const uint64_t *seq_off, uint32_t n_seq, const uint32_t *pair_a, const uint32_t *pair_b,
                            uint64_t n_pairs, pwa_batch **out);
int pwa_scores_affine(pwa_ctx *ctx, int match, int mismatch, int gap_open, int gap_extend, const uint8_t *seq_bytes,
                      const uint64_t *seq_off, uint32_t n_seq, const uint32_t *pair_a, const uint32_t *pair_b,
                      uint64_t n_pairs, int32_t *score_out);

/*
 * The alignments hw3.cpp builds against the center of the star (hw3.cpp:261-283): affine_alignment(string1, string2,
 * ..., &alignedString1, &alignedString2), i.e. hw3.cpp:23-135 with its three trace matrices, its tie-breaks (V,
 * then F if strictly greater, then E if strictly greater; a gap is extended only if that is strictly better than
 * opening one) and its walk.  pair (a, b): string1 = sequence a, string2 = sequence b.
 * Engines: pairs that share string1 (the center) form wave tasks of up to 64 pairs, one lane each, on the strip kernels
 * (batch_affine_tb.hip.h); a task moves to the stripe engine (pair_affine_tb.hip.h: each pair over ceil(n / 256) waves, then one
 * wave walks it) when that is estimated to be faster -- few long pairs -- or when its strip band would not fit the HBM budget.
 * Only lists with (n + m + 2) * max(|M|, |Mm|, |Go| + |Ge|) < 2^26 qualify; every other list stays on the strips.  The stripe
 * pairs run in consecutive chunks whose bands (~n * (m + 80) bytes per pair) fit min(0.6 free HBM, 48 GiB); a single pair whose
 * band exceeds free HBM fails with PWA_E_NOMEM.  Both engines give the reference's op lists byte for byte.
 * PWA_AFFINE_TB_ROUTE=0 keeps every pair on the strips, =1 moves every task of a qualifying list.
 *   score_out[k] : max(V, F, E)[n][m] as pwa_scores_affine
 *   ops          : one byte per alignment column in TRACEBACK order (end -> start), pair k at ops[ops_off[k] ..):
 *                  'M' both symbols, 'D' string1 symbol against '-', 'I' '-' against string2 symbol; the caller
 *                  leaves room for n_k + m_k bytes per pair;   n_ops[k] : columns of pair k
 */
int pwa_align_affine_batch(pwa_ctx *ctx, int match, int mismatch, int gap_open, int gap_extend, const uint8_t *seq_bytes,
                           const uint64_t *seq_off, uint32_t n_seq, const uint32_t *pair_a, const uint32_t *pair_b,
                           uint64_t n_pairs, int32_t *score_out, uint8_t *ops, const uint64_t *ops_off, uint64_t *n_ops);
/* The last pwa_align_affine_batch on ctx: pairs it ran on the stripe engine, device ms of their fills and of their walks
 * (event-timed, summed over chunks), and the bytes of traceback band those fills wrote. */
int pwa_align_affine_last_stats(const pwa_ctx *ctx, uint64_t *stripe_pairs, float *fill_ms, float *walk_ms, uint64_t *band_bytes);

/*
 * The all-pairs step of the sibling program /root/reference/hw4/hw4.cpp (138-159): per pair a
 * Needleman-Wunsch alignment with hw4's tie-break (diag >= up >= left, hw4.cpp:36-47 -- not hw2's) and
 * the number of alignment columns that hold a gap or a mismatch (146-152).  dist_out[k] is that count
 * for pair k (pair_a = sequence1 = rows, pair_b = sequence2 = columns).  No traceback is stored: the
 * kernel carries the distance of the chosen path through the DP.  The batch object behaves like any
 * other (run / d_scores / fetch / info / destroy; no end cells).
 * Engines: the strip kernels (lane = pair) take every list; a list in the two-value form (some pair with
 * n + m > 4000, or PWA_NO_PACKED_DIST) over at most 7 symbols with (n + m + 2) * max|score| < 2^28 is split
 * by estimated cost between them and the stripe engine's distance fill (a pair over many waves: few long
 * sequences), like a scores pass; PWA_SCORES_ROUTE=0 keeps every pair on the strips, =1 moves every such
 * pair.  A split batch reports "<strip kernel> + <stripe kernel>".  pwa_distances inherits the routing.
 */
int pwa_nwdist_batch_create(pwa_ctx *ctx, int match, int mismatch, int gap, const uint8_t *seq_bytes,
                            const uint64_t *seq_off, uint32_t n_seq, const uint32_t *pair_a, const uint32_t *pair_b,
                            uint64_t n_pairs, pwa_batch **out);
int pwa_distances(pwa_ctx *ctx, int match, int mismatch, int gap, const uint8_t *seq_bytes, const uint64_t *seq_off,
                  uint32_t n_seq, const uint32_t *pair_a, const uint32_t *pair_b, uint64_t n_pairs, int32_t *dist_out);
/* Host-side UPGMA + Newick of hw4.cpp:162-228 over a dense symmetric n x n matrix of doubles (no GPU
 * work).  Writes the NUL-terminated tree "(...):0.0;" into out; *needed receives the size required
 * (PWA_E_CAPACITY when cap is too small; call with cap = 0 to size the buffer). */
int pwa_upgma_newick(const double *dist, const char *const *names, uint32_t n, char *out, uint64_t cap, uint64_t *needed);

/*
 * Full alignment of ONE pair: matrix fill with the traceback band in HBM + traceback walk on
 * the device.  Replaces one call of hw2.cpp:118 / hw2.cpp:192 up to (not including) the string
 * post-processing prepareCigarString / prepareMDZString (59-116), which stays on the host.
 *
 *   ops      : receives the walk's op bytes 'M' (diagonal), 'D' (up: pattern char vs '-'),
 *              'I' (left: '-' vs text char) in TRACEBACK order, i.e. exactly the contents of
 *              the reference's `tracebacks` vector (hw2.cpp:161, 237) before any reversal;
 *   ops_cap  : capacity of ops; n + m always suffices (PWA_E_CAPACITY otherwise);
 *   end_cell : {i, j} the walk starts from (NW: n, m; SW: first row-major maximum; SG: n, j* = first maximum of row n);
 *   start_cell: {i, j} where it stops (NW: 0,0; SG: 0, j0).   Either may be NULL.
 *   score    : NW dp[n][m]; SW the maximum cell; SG dp[n][j*].
 */
int pwa_align(pwa_ctx *ctx, int mode, int match, int mismatch, int gap, const uint8_t *pattern, uint64_t n,
              const uint8_t *text, uint64_t m, int32_t *score, uint8_t *ops, uint64_t ops_cap, uint64_t *n_ops,
              uint64_t end_cell[2], uint64_t start_cell[2]);

/*
 * The two matrices the reference keeps per pair, in the reference's own row-major form (for
 * inspection and whole-matrix parity tests; sizes are the caller's problem: 5 B per cell):
 *   dp_out : int32 (n+1) x (m+1) = `dp`        (hw2.cpp:119 / 193), or NULL
 *   tb_out : char  (n+1) x (m+1) = `traceback` (hw2.cpp:120 / 194): ' ', 'd', 'u', 'l', '0', or NULL
 *            (SG: row 0 is 0 / ' ', column 0 i * gap / 'u', the interior NW's)
 * On the device both are written as skewed bands (int32 score band + 1 B/cell traceback band, one
 * coalesced wave store per anti-diagonal step); the host un-skews them.
 */
int pwa_align_matrices(pwa_ctx *ctx, int mode, int match, int mismatch, int gap, const uint8_t *pattern, uint64_t n,
                       const uint8_t *text, uint64_t m, int32_t *dp_out, char *tb_out);

/* Device time in ms of the fill kernel(s) / traceback kernel of the last pwa_align on ctx, and
 * the bytes of traceback band it wrote to HBM (for roofline accounting). */
int pwa_align_last_stats(const pwa_ctx *ctx, float *fill_ms, float *traceback_ms, uint64_t *band_bytes);

/*
 * Full alignment of many pairs (the -g path needs every pair's alignment: hw2.cpp:344).
 * ops of pair k are written at ops[ops_off[k] .. ops_off[k] + n_ops[k]); the caller sizes
 * ops_off so that pair k has room for n_k + m_k bytes.  When the regions follow one another without a gap
 * (ops_off[k + 1] == ops_off[k] + n_k + m_k) the device op buffer mirrors the caller's and every chunk of pairs comes
 * back with one copy straight into `ops`; any other layout works through a staging copy.  No sequence-arena limit here
 * (64-bit device pointers); the traceback bands are processed in ranges of consecutive pairs that fit the free HBM, and inside a
 * range every pair runs with the band geometry its own pattern length asks for.  Bytes of a pair's region beyond n_ops[k] are
 * undefined after the call.
 */
int pwa_align_batch(pwa_ctx *ctx, int mode, int match, int mismatch, int gap, const uint8_t *seq_bytes,
                    const uint64_t *seq_off, uint32_t n_seq, const uint32_t *pair_a, const uint32_t *pair_b,
                    uint64_t n_pairs, int32_t *score_out, uint8_t *ops, const uint64_t *ops_off, uint64_t *n_ops,
                    uint64_t *end_cells /* 2*n_pairs or NULL */, uint64_t *start_cells /* 2*n_pairs or NULL */);

/*
 * The same alignments as pwa_align_batch (same arguments, same score_out / end_cells / start_cells), returned as the two
 * strings the reference derives from each walk -- prepareCigarString (hw2.cpp:59-78) and prepareMDZString (80-116) -- instead
 * of the op lists.  The strings are built on the device right after each range's walks, and only they cross to the host.
 *   pair k's CIGAR is cigar[cigar_off[k] .. cigar_off[k + 1]), its MD:Z mdz[mdz_off[k] .. mdz_off[k + 1]) (n_pairs + 1 offsets each,
 *   written by the library); the strings are packed back to back in pair order, without NUL terminators, and are exactly the
 *   bytes pwa_format_alignment gives for that pair's op list (any byte value may appear, '-' and NUL included).  A pair with
 *   one side empty: NW "nD" / "0^<pattern>0" (empty text), "mI" / "0" (empty pattern); SW: "" / "0", as for a zero score; SG: as NW
 *   for an empty text, "" / "0" for an empty pattern.  score_out / end_cells / start_cells: as pwa_align, per pair.
 *   PWA_E_CAPACITY when the strings exceed cigar_cap / mdz_cap: needed (when not NULL) receives the two totals, and the string
 *   buffers are undefined.  The sums over the pairs of pwa_cigar_bound(n_k + m_k) and pwa_mdz_bound(n_k + m_k) always suffice.
 */
int pwa_align_batch_cigar(pwa_ctx *ctx, int mode, int match, int mismatch, int gap, const uint8_t *seq_bytes,
                          const uint64_t *seq_off, uint32_t n_seq, const uint32_t *pair_a, const uint32_t *pair_b,
                          uint64_t n_pairs, int32_t *score_out,
                          char *cigar, uint64_t cigar_cap, uint64_t *cigar_off /* n_pairs + 1 */,
                          char *mdz, uint64_t mdz_cap, uint64_t *mdz_off /* n_pairs + 1 */,
                          uint64_t *end_cells /* 2*n_pairs or NULL */, uint64_t *start_cells /* 2*n_pairs or NULL */,
                          uint64_t needed[2] /* or NULL */);

/*
 * Affine-gap ("gotoh") alignments of many pairs: pwa_align_batch / pwa_align_batch_cigar with a gap open and a gap extend.  Named
 * gotoh, not affine, to keep them apart from hw3's drop-in (pwa_scores_affine, pwa_align_affine_batch), whose quirks they do not share.
 * Scoring: match, mismatch, gap_open, gap_extend (signed, the usual sign convention); a gap of length L scores gap_open + L * gap_extend.
 * gap_open <= 0 and gap_extend <= 0, else PWA_E_INVALID.  s(i,j) = match when p[i-1] == t[j-1] as raw bytes (any byte value, NUL and
 * '-' included), mismatch otherwise; oe = gap_open + gap_extend.
 *   E[i][j] = max(H[i][j-1] + oe, E[i][j-1] + gap_extend)   'I' (left);  a tie OPENS
 *   F[i][j] = max(H[i-1][j] + oe, F[i-1][j] + gap_extend)   'D' (up);    a tie OPENS
 *   H[i][j] = max(H[i-1][j-1] + s(i,j), E[i][j], F[i][j])    SW: and 0
 *   H tie-break  NW, SG: diag >= E >= F  (hw2's NW: diag >= left >= up);  SW: zero > diag > F > E  (hw2's SW: zero > diag > up > left)
 *   E[i][0] = F[0][j] = -inf
 *   NW: H[0][0] = 0, H[0][j] = gap_open + j * gap_extend, H[i][0] = gap_open + i * gap_extend
 *   SW: H[0][j] = H[i][0] = 0
 *   SG: H[0][j] = 0, H[i][0] = gap_open + i * gap_extend
 * End cells and scores follow the linear modes: NW ends at (n, m); SW at the first row-major maximum of H, or at (0, 0) with no ops
 * when every H is 0; SG at (n, j*), j* the smallest j with maximal H[n][j].
 * The walk starts in state H at the end cell.  In H the cell's source decides: diag emits 'M' and goes to (i-1, j-1); E or F switch to
 * that state on the same cell; SW stops on a zero cell.  In E: 'I', then (i, j-1) in H when E[i][j] opened, in E when it extended; F
 * likewise with 'D' and (i-1, j).  Boundaries as in the linear modes: NW and SG emit the 'D' run down column 0, NW the 'I' run along
 * row 0; SG stops at row 0 with start_cell = (0, j0); SW stops in state H at i = 0, at j = 0 or on a zero cell.  Ops are written in
 * traceback order ('M' / 'D' / 'I'), as pwa_align_batch writes them; a pair with an empty side follows pwa_align_batch_cigar's
 * conventions per mode (its one gap scores gap_open + L * gap_extend, an empty pair 0).
 * With gap_open = 0, the H matrix, every code choice and every op list equal the linear mode's with gap = gap_extend.
 * Range: every result is exact while (n + m + 2) * max(|match|, |mismatch|, |gap_open| + |gap_extend|) < 2^28; a pair beyond that is
 * PWA_E_CAPACITY.  Shape: patterns of at most 1024 symbols (0..256 rows: 16 lanes per pair, 257..1024: one pair per wave), else
 * PWA_E_CAPACITY; texts of any length the linear calls take.
 * Arguments, op-region layout, range splitting (PWA_RANGE_BYTES) and string buffers (pwa_cigar_bound / pwa_mdz_bound) are exactly
 * pwa_align_batch's and pwa_align_batch_cigar's.  An empty pair list is PWA_OK.
 */
int pwa_align_gotoh_batch(pwa_ctx *ctx, int mode /* NW, SW, SG */, int match, int mismatch, int gap_open, int gap_extend,
                          const uint8_t *seq_bytes, const uint64_t *seq_off, uint32_t n_seq, const uint32_t *pair_a,
                          const uint32_t *pair_b, uint64_t n_pairs, int32_t *score_out, uint8_t *ops, const uint64_t *ops_off,
                          uint64_t *n_ops, uint64_t *end_cells /* 2*n_pairs or NULL */, uint64_t *start_cells /* 2*n_pairs or NULL */);
int pwa_align_gotoh_batch_cigar(pwa_ctx *ctx, int mode, int match, int mismatch, int gap_open, int gap_extend,
                                const uint8_t *seq_bytes, const uint64_t *seq_off, uint32_t n_seq, const uint32_t *pair_a,
                                const uint32_t *pair_b, uint64_t n_pairs, int32_t *score_out,
                                char *cigar, uint64_t cigar_cap, uint64_t *cigar_off /* n_pairs + 1 */,
                                char *mdz, uint64_t mdz_cap, uint64_t *mdz_off /* n_pairs + 1 */,
                                uint64_t *end_cells /* 2*n_pairs or NULL */, uint64_t *start_cells /* 2*n_pairs or NULL */,
                                uint64_t needed[2] /* or NULL */);
/* Device ms of the fills and walks of the last pwa_align_gotoh_batch(_cigar) on ctx, and the band bytes they wrote. */
int pwa_align_gotoh_last_stats(const pwa_ctx *ctx, float *fill_ms, float *walk_ms, uint64_t *band_bytes);

/*
 * BANDED affine-gap alignments of long pairs: pwa_align_gotoh_batch(_cigar) restricted to a diagonal band per pair.
 *   pwa_align_banded_batch        pwa_align_gotoh_batch's arguments, then band_lo, band_hi (one value each per list pair);
 *   pwa_align_banded_batch_cigar  pwa_align_gotoh_batch_cigar's arguments, then the same two arrays;
 *   pwa_align_banded_last_stats   device ms of the fills and walks of the last such call on ctx, and the band bytes they wrote.
 * Everything not said here is the gotoh block's rule above: E / F / H, "a tie opens", the H tie-break per mode, raw-byte equality, the
 * sign rule for gap_open / gap_extend, op order, empty-side conventions, op-region layout, string buffers, PWA_RANGE_BYTES, the empty
 * list, and the range rule (n + m + 2) * max(|match|, |mismatch|, |gap_open| + |gap_extend|) < 2^28 (an all-zero scoring counts as 1).
 * The band.  Cell (i, j), 0 <= i <= n, 0 <= j <= m, is in the band of pair k iff band_lo[k] <= j - i <= band_hi[k].  Every cell
 * outside the band is -inf in H, E and F.  The result is the exact optimum over the paths that stay inside the band, with the walk and
 * the tie-breaks applied to the banded matrices.
 * Boundaries.  A boundary cell keeps its mode's boundary value only when the boundary path that value stands for lies in the band,
 * else it is -inf:
 *   NW row 0,  H[0][j] = gap_open + j * gap_extend:  needs band_lo <= 0 and j <= band_hi;
 *   NW / SG column 0,  H[i][0] = gap_open + i * gap_extend:  needs band_hi >= 0 and -i >= band_lo;
 *   the free boundaries (SG / SW row 0, SW column 0, value 0):  need the cell itself in the band.
 * Ends.  NW ends at (n, m); SG at the smallest in-band j with maximal H[n][j]; SW at the first row-major maximum over in-band cells,
 * or at (0, 0) with no ops when no in-band H is positive.
 * Validity, checked before any device work, in pair order (the first offending pair decides the error):  PWA_E_INVALID for
 * band_lo > band_hi; for NW unless band_lo <= 0 <= band_hi and band_lo <= m - n <= band_hi; for SG unless band_hi >= 0 and
 * n + band_lo <= m (together: an in-band path from row 0 to row n exists).  SW takes any band.  A pair with an empty side follows the
 * gotoh conventions, provided its band is valid.
 * Shape.  Patterns and texts of any length the linear calls take.  Band width band_hi - band_lo + 1 of at most 4096 (the hand-off row
 * of a pair lives in LDS), else PWA_E_CAPACITY.
 * Identity.  If the walk of the unbanded gotoh alignment stays inside the band, the banded call returns the same score, cells and op
 * list byte for byte: banded values are <= the unbanded ones everywhere and equal on that path, so every priority choice and every
 * open / extend bit on the path is the same (the bits of cells whose E or F is -inf are never read by a walk).
 */
int pwa_align_banded_batch(pwa_ctx *ctx, int mode /* NW, SW, SG */, int match, int mismatch, int gap_open, int gap_extend,
                           const uint8_t *seq_bytes, const uint64_t *seq_off, uint32_t n_seq, const uint32_t *pair_a,
                           const uint32_t *pair_b, uint64_t n_pairs, int32_t *score_out, uint8_t *ops, const uint64_t *ops_off,
                           uint64_t *n_ops, uint64_t *end_cells /* 2*n_pairs or NULL */, uint64_t *start_cells /* 2*n_pairs or NULL */,
                           const int32_t *band_lo /* n_pairs */, const int32_t *band_hi /* n_pairs */);
int pwa_align_banded_batch_cigar(pwa_ctx *ctx, int mode, int match, int mismatch, int gap_open, int gap_extend,
                                 const uint8_t *seq_bytes, const uint64_t *seq_off, uint32_t n_seq, const uint32_t *pair_a,
                                 const uint32_t *pair_b, uint64_t n_pairs, int32_t *score_out,
                                 char *cigar, uint64_t cigar_cap, uint64_t *cigar_off /* n_pairs + 1 */,
                                 char *mdz, uint64_t mdz_cap, uint64_t *mdz_off /* n_pairs + 1 */,
                                 uint64_t *end_cells /* 2*n_pairs or NULL */, uint64_t *start_cells /* 2*n_pairs or NULL */,
                                 uint64_t needed[2] /* or NULL */, const int32_t *band_lo /* n_pairs */, const int32_t *band_hi /* n_pairs */);
int pwa_align_banded_last_stats(const pwa_ctx *ctx, float *fill_ms, float *walk_ms, uint64_t *band_bytes);

/*
 * BANDED affine-gap SCORES of long pairs: the banded block above without alignments -- no traceback band, no walk.
 * For every list that pwa_align_banded_batch accepts, score_out[k], end_i_out[k] and end_j_out[k] equal that call's score and end cell for pair k.
 * That covers the boundary rule, the end rule per mode, the empty-side conventions, the empty list (PWA_OK), and validity: the same checks
 * with the same codes, before any device work and in pair order; a null score_out, band_lo or band_hi with n_pairs > 0 is PWA_E_INVALID.
 * end_i_out / end_j_out may each be NULL.  No band bytes exist, so PWA_RANGE_BYTES does not cut the list.
 *   pwa_scores_banded_last_stats  device ms of the score passes of the last such call on ctx, and its in-band cells: the cells (i, j),
 *                                 1 <= i <= n, 1 <= j <= m, band_lo <= j - i <= band_hi, summed over the list (what the recurrence
 *                                 computes; a pair with an empty side counts 0).  A call that fails validation leaves them unchanged.
 * Not offered: a batch object (no pwa_banded_batch_create / pwa_batch_run, no sharding).
 */
int pwa_scores_banded(pwa_ctx *ctx, int mode /* NW, SW, SG */, int match, int mismatch, int gap_open, int gap_extend,
                      const uint8_t *seq_bytes, const uint64_t *seq_off, uint32_t n_seq, const uint32_t *pair_a,
                      const uint32_t *pair_b, uint64_t n_pairs, int32_t *score_out, uint32_t *end_i_out /* or NULL */,
                      uint32_t *end_j_out /* or NULL */, const int32_t *band_lo /* n_pairs */, const int32_t *band_hi /* n_pairs */);
int pwa_scores_banded_last_stats(const pwa_ctx *ctx, float *fill_ms, uint64_t *in_band_cells);

/*
 * BANDED X-DROP EXTENSION of long pairs ("EXT"): the alignment is anchored at cell (0, 0) -- a seed's end --, its end is free in both
 * sequences, and the sweep over the rows is given up once the score has fallen xdrop below the best seen (BLAST's X-drop; the zdrop of
 * ksw2_extz without its diagonal term).
 *   pwa_extend_banded_batch        pwa_align_banded_batch's arguments without `mode` and `start_cells`, xdrop after gap_extend, and rows_out;
 *   pwa_extend_banded_batch_cigar  pwa_align_banded_batch_cigar's, changed the same way;
 *   pwa_scores_extend_banded       pwa_scores_banded's, changed the same way: no traceback band, no walk;
 *   pwa_extend_banded_last_stats   device ms of the fills and walks of the last of these three calls on ctx, and the sum of its rows_out.
 * Everything not said here is the banded block's rule (pwa_align_banded_batch): the gotoh recurrences, "a tie opens", raw-byte
 * equality, gap_open <= 0 and gap_extend <= 0, the band band_lo <= j - i <= band_hi with -inf outside, a width of at most 4096
 * (else PWA_E_CAPACITY), op order and op-region layout, string buffers, PWA_RANGE_BYTES, and the empty list.
 * Matrix.  The banded NW matrix: H[0][0] = 0, row 0 and column 0 hold gap_open + L * gap_extend under the banded boundary rule, the H
 * tie-break is NW's (diag >= E >= F), and there is no zero floor.
 * Validity.  band_lo <= 0 <= band_hi: the anchor is in the band; otherwise PWA_E_INVALID.  Nothing is required of m - n.
 * band_lo > band_hi is checked first, then this rule, then the width; in pair order, and the first offending pair decides.
 * Best cell.  The record starts as (score 0, cell (0, 0)).  Rows i = 1, 2, ... are taken in order; rmax(i) is the maximum of H[i][j]
 * over the in-band cells with 1 <= j <= m (-inf when the row has none), and the smallest such j stands for the row.  A row replaces
 * the record only on a strictly larger value: the end cell is the first row-major maximum, and a best score of 0 ends at (0, 0) with
 * no ops.
 * X-drop.  With xdrop >= 0, row i stops the sweep iff rmax(i) < best(i - 1) - xdrop, best(i - 1) being the record's score after row
 * i - 1.  The first such row r* and every row below it are not considered, and rows_out[k] = r* - 1, or n when no row stops.  A row
 * whose band has left the matrix (i + band_lo > m) has rmax = -inf and stops the sweep whenever xdrop >= 0.  With xdrop < 0 no row ever
 * stops, and rows_out[k] is the last row that has an in-band cell (min(n, m - band_lo) for a clamped band).  xdrop > 2^27 is
 * PWA_E_INVALID.
 * Walk.  From the end cell in state H, NW's walk on the banded matrices, down to (0, 0).  The start cell is always (0, 0), so the calls
 * do not return it.
 * Empty sides.  A pair with an empty side scores 0, ends at (0, 0), has no ops and rows_out = 0; its band must still be valid.
 * Range.  (n + m + 2) * max(|match|, |mismatch|, |gap_open| + |gap_extend|, 1) < 2^27, else PWA_E_CAPACITY: one bit tighter than the
 * banded rule, because the row maxima are kept as H * 16 + 4 column bits and H may be negative here.
 * Memory.  A pair's traceback band is planned for all n rows: the host cannot know the stop row.
 * Identities.  (1) With xdrop < 0 the score is the maximum over all in-band cells of the banded NW matrix, together with 0.  (2) If
 * the stop row lies below the end row that xdrop < 0 gives, both calls return the same score, end cell and ops.  (3) The scores call
 * equals the alignment call on (score, end, rows).
 * end_cells, rows_out, end_i_out and end_j_out may each be NULL.  A null score_out, band_lo or band_hi with n_pairs > 0 is
 * PWA_E_INVALID.  A call that fails validation leaves the stats unchanged; walk_ms is 0 after the scores call.
 * Not offered: ksw2's diagonal-aware Z-drop term, the pattern-end result (the best score of row n: the substitution-matrix forms below
 * return it), a batch object.
 */
int pwa_extend_banded_batch(pwa_ctx *ctx, int match, int mismatch, int gap_open, int gap_extend, int xdrop,
                            const uint8_t *seq_bytes, const uint64_t *seq_off, uint32_t n_seq, const uint32_t *pair_a,
                            const uint32_t *pair_b, uint64_t n_pairs, int32_t *score_out, uint8_t *ops, const uint64_t *ops_off,
                            uint64_t *n_ops, uint64_t *end_cells /* 2*n_pairs or NULL */, uint32_t *rows_out /* n_pairs or NULL */,
                            const int32_t *band_lo /* n_pairs */, const int32_t *band_hi /* n_pairs */);
int pwa_extend_banded_batch_cigar(pwa_ctx *ctx, int match, int mismatch, int gap_open, int gap_extend, int xdrop,
                                  const uint8_t *seq_bytes, const uint64_t *seq_off, uint32_t n_seq, const uint32_t *pair_a,
                                  const uint32_t *pair_b, uint64_t n_pairs, int32_t *score_out,
                                  char *cigar, uint64_t cigar_cap, uint64_t *cigar_off /* n_pairs + 1 */,
                                  char *mdz, uint64_t mdz_cap, uint64_t *mdz_off /* n_pairs + 1 */,
                                  uint64_t *end_cells /* 2*n_pairs or NULL */, uint32_t *rows_out /* n_pairs or NULL */,
                                  uint64_t needed[2] /* or NULL */, const int32_t *band_lo /* n_pairs */, const int32_t *band_hi /* n_pairs */);
int pwa_scores_extend_banded(pwa_ctx *ctx, int match, int mismatch, int gap_open, int gap_extend, int xdrop,
                             const uint8_t *seq_bytes, const uint64_t *seq_off, uint32_t n_seq, const uint32_t *pair_a,
                             const uint32_t *pair_b, uint64_t n_pairs, int32_t *score_out, uint32_t *end_i_out /* or NULL */,
                             uint32_t *end_j_out /* or NULL */, uint32_t *rows_out /* or NULL */,
                             const int32_t *band_lo /* n_pairs */, const int32_t *band_hi /* n_pairs */);
int pwa_extend_banded_last_stats(const pwa_ctx *ctx, float *fill_ms, float *walk_ms, uint64_t *rows_considered);

/*
 * BANDED X-DROP EXTENSION UNDER A SUBSTITUTION MATRIX, with a PATTERN-END result: the EXT calls above with the caller's score table,
 * for a protein seed extended under BLOSUM-style scores, a long read with a neutral N, transitions scored apart from transversions.
 *   pwa_extend_banded_subst_batch        pwa_extend_banded_batch's arguments with (code, n_sym, submat) in place of (match, mismatch),
 *                                        and pend_score_out, pend_j_out after rows_out;
 *   pwa_extend_banded_subst_batch_cigar  pwa_extend_banded_batch_cigar's, changed the same way;
 *   pwa_scores_extend_banded_subst       pwa_scores_extend_banded's, changed the same way: no traceback band, no walk.
 * Semantics: exactly those of the EXT block -- the banded NW matrix with no zero floor, validity band_lo <= 0 <= band_hi, the record
 * and rmax(i) over 1 <= j <= m, the stop rule, rows_out, NW's walk, the empty-side conventions, the band width of at most 4096,
 * PWA_RANGE_BYTES (the table is uploaded once per call and serves every range), the empty list (PWA_OK) -- with
 *   s(i,j) = submat[ code[p[i-1]] * n_sym + code[t[j-1]] ]
 * and code, n_sym, submat as in the substitution-matrix block: n_sym is 1 .. 32, every one of the 256 code entries is < n_sym, the
 * table may be asymmetric and may hold any signs, and both are copied during the call.  CIGAR and MD:Z come from the ops and the RAW
 * bytes: MD:Z reports byte identity, not the sign of the score.
 * Pattern end (ksw2_extz's mqe / mqe_t): did the extension reach the end of the pattern, and what does the to-end alignment score?
 * If n >= 1 and rows_out[k] == n: pend_score_out[k] = rmax(n), pend_j_out[k] = the smallest column attaining it (rows_out == n
 * implies that row n has an in-band cell with j >= 1, so the value is real; it may lie below score_out[k], whose end row is then
 * above n).  Otherwise -- a row up to and including n stopped the sweep, the band left the matrix before row n, or m = 0 with n > 0 --
 * pend_score_out[k] = PWA_EXT_NO_PEND and pend_j_out[k] = 0.  For n = 0 the anchor is the pattern's end: score 0 and j 0.  The
 * result depends on nothing but the fill, so the three calls agree on it.  Where pend_j >= 1, pend_score is the score that
 * pwa_scores_banded_subst(PWA_MODE_NW) gives for the pattern against the text's first pend_j symbols under the same band.
 * pend_score_out and pend_j_out may each be NULL.
 * Range.  (n + m + 2) * max(max |submat|, |gap_open| + |gap_extend|, 1) < 2^27, else PWA_E_CAPACITY: the EXT block's one-bit-tighter
 * rule with the table's magnitude, because the row maxima are kept as H * 16 + 4 column bits and H may be negative.  With A that
 * maximum, every H, E or F that stands for a path inside the band is a sum of at most n + m + 1 steps of magnitude <= A each, so
 * |V| < 2^27 - A: the alignment fill's sentinel key -2^31 + 8 A + 1 is below every key V * 8 + 0..7, the score pass's plain sentinel
 * -2^30 below every V and V + gap_open + gap_extend, and a sentinel meets at most one gap extension (>= -A) before the sum is compared
 * and dropped; only |s| enters the bound.  The row key H * 16 + 0..15 of a real H lies strictly inside int32 and above the key
 * INT32_MIN of a row without an in-band cell, whose H reads as -2^27, below every real H; best - xdrop cannot wrap.
 * Checks, all before any device work: first the table's own, as pwa_align_banded_subst_batch makes them (PWA_E_INVALID for a null
 * code or submat, n_sym outside 1 .. 32, a code[] entry >= n_sym, gap_open > 0 or gap_extend > 0, a null band_lo or band_hi with
 * n_pairs > 0); then xdrop > 2^27 (PWA_E_INVALID); then per pair, in pair order, band_lo > band_hi, the anchor rule, the width and
 * the range rule (the first offending pair decides the error).
 * Stats: pwa_extend_banded_last_stats, the same record as the byte-compare EXT calls; pwa_align_subst_last_stats and the
 * pwa_align_banded / pwa_scores_banded stats are not touched.  A call that fails validation leaves all stats unchanged.
 * Not offered: ksw2's diagonal-aware Z-drop term, a batch object, named matrices.
 */
#define PWA_EXT_NO_PEND INT32_MIN /* pend_score_out: row n was not reached or not kept */
int pwa_extend_banded_subst_batch(pwa_ctx *ctx, const uint8_t code[256], int n_sym, const int32_t *submat, int gap_open,
                                  int gap_extend, int xdrop, const uint8_t *seq_bytes, const uint64_t *seq_off, uint32_t n_seq,
                                  const uint32_t *pair_a, const uint32_t *pair_b, uint64_t n_pairs, int32_t *score_out, uint8_t *ops,
                                  const uint64_t *ops_off, uint64_t *n_ops, uint64_t *end_cells /* 2*n_pairs or NULL */,
                                  uint32_t *rows_out /* n_pairs or NULL */, int32_t *pend_score_out /* n_pairs or NULL */,
                                  uint32_t *pend_j_out /* n_pairs or NULL */, const int32_t *band_lo /* n_pairs */,
                                  const int32_t *band_hi /* n_pairs */);
int pwa_extend_banded_subst_batch_cigar(pwa_ctx *ctx, const uint8_t code[256], int n_sym, const int32_t *submat, int gap_open,
                                        int gap_extend, int xdrop, const uint8_t *seq_bytes, const uint64_t *seq_off, uint32_t n_seq,
                                        const uint32_t *pair_a, const uint32_t *pair_b, uint64_t n_pairs, int32_t *score_out,
                                        char *cigar, uint64_t cigar_cap, uint64_t *cigar_off /* n_pairs + 1 */,
                                        char *mdz, uint64_t mdz_cap, uint64_t *mdz_off /* n_pairs + 1 */,
                                        uint64_t *end_cells /* 2*n_pairs or NULL */, uint32_t *rows_out /* n_pairs or NULL */,
                                        int32_t *pend_score_out /* n_pairs or NULL */, uint32_t *pend_j_out /* n_pairs or NULL */,
                                        uint64_t needed[2] /* or NULL */, const int32_t *band_lo /* n_pairs */,
                                        const int32_t *band_hi /* n_pairs */);
int pwa_scores_extend_banded_subst(pwa_ctx *ctx, const uint8_t code[256], int n_sym, const int32_t *submat, int gap_open,
                                   int gap_extend, int xdrop, const uint8_t *seq_bytes, const uint64_t *seq_off, uint32_t n_seq,
                                   const uint32_t *pair_a, const uint32_t *pair_b, uint64_t n_pairs, int32_t *score_out,
                                   uint32_t *end_i_out /* or NULL */, uint32_t *end_j_out /* or NULL */, uint32_t *rows_out /* or NULL */,
                                   int32_t *pend_score_out /* or NULL */, uint32_t *pend_j_out /* or NULL */,
                                   const int32_t *band_lo /* n_pairs */, const int32_t *band_hi /* n_pairs */);

/*
 * Affine-gap ("gotoh") SCORES of many pairs: what pwa_scores / pwa_batch_create are to pwa_align_batch.  Recurrence, boundaries, raw-byte
 * equality, sign rule (gap_open <= 0 and gap_extend <= 0, else PWA_E_INVALID), score and end cell per mode, pairs with an empty side,
 * the range rule (a pair beyond it is PWA_E_CAPACITY) and the empty list (PWA_OK) are exactly those of the comment block of
 * pwa_align_gotoh_batch above: score_out[k] (and the end cell) equal what that call returns for pair k wherever both accept the pair.
 *   pwa_gotoh_batch_create  a batch object like every other: pwa_batch_run (asynchronous, on the caller's stream) / _d_scores /
 *                     _set_d_scores / _fetch / _info / _last_ms / _run_times / _destroy; end cells when want_end_cells was set;
 *                     pwa_batch_cell_bits is 32 or 0, pwa_batch_profile_form 0;
 *   pwa_scores_gotoh  the one-call form over lists of any size (cut into arena-sized pipelined runs, as pwa_scores); end cells when
 *                     end_i_out or end_j_out is given.
 * Engines, chosen by rule: PWA_MODE_NW, and PWA_MODE_SW with mismatch <= 0, without end cells run on register-strip kernels of their own
 * (lane = pair, patterns of ANY length) as long as some byte value occurs in no text (the strips pad short patterns with it).  Every
 * other list -- PWA_MODE_SG, end cells wanted, SW with mismatch > 0, texts that use all 256 byte values -- runs on the band-less form of
 * pwa_align_gotoh_batch's fills, whose shape rule then holds for the whole list: patterns of at most 1024 symbols, else PWA_E_CAPACITY.
 */
int pwa_gotoh_batch_create(pwa_ctx *ctx, int mode /* NW, SW, SG */, int match, int mismatch, int gap_open, int gap_extend,
                           const uint8_t *seq_bytes, const uint64_t *seq_off, uint32_t n_seq, const uint32_t *pair_a,
                           const uint32_t *pair_b, uint64_t n_pairs, int want_end_cells, pwa_batch **out);
int pwa_scores_gotoh(pwa_ctx *ctx, int mode, int match, int mismatch, int gap_open, int gap_extend, const uint8_t *seq_bytes,
                     const uint64_t *seq_off, uint32_t n_seq, const uint32_t *pair_a, const uint32_t *pair_b, uint64_t n_pairs,
                     int32_t *score_out, uint32_t *end_i_out, uint32_t *end_j_out);

/*
 * Substitution-matrix scoring for the affine-gap ("gotoh") calls: alignments (op lists, or CIGAR + MD:Z), batch objects and one-call
 * scores.  The semantics are exactly those of the comment block of pwa_align_gotoh_batch above -- recurrences for E / F / H, a tie
 * opens, the H tie-breaks per mode, boundaries, end cells, the three-state walk and its op bytes, the conventions for pairs with an
 * empty side, gap_open <= 0 and gap_extend <= 0 (else PWA_E_INVALID; gap_open = 0 gives linear gaps) -- with one substitution:
 *   s(i,j) = submat[ code[p[i-1]] * n_sym + code[t[j-1]] ]
 *   code    uint8_t[256], byte value -> symbol code.  Every one of the 256 entries must be < n_sym, else PWA_E_INVALID: the caller
 *           decides where unknown bytes, lower case, NUL and '-' go (a wildcard code with a row and a column of its own, say).
 *   n_sym   1 .. 32, else PWA_E_INVALID.
 *   submat  int32_t[n_sym * n_sym], row = pattern code, column = text code.  It may be asymmetric and may hold any signs, positive
 *           off-diagonal entries in PWA_MODE_SW included.
 * code and submat are copied during the call (a batch object keeps its own copy): the caller may free them afterwards.  A null code or
 * submat is PWA_E_INVALID.  No named matrix (BLOSUM, PAM) ships with the library: the caller supplies the numbers.
 * CIGAR and MD:Z are built from the ops and the RAW bytes, as in every other call: MD:Z reports BYTE IDENTITY, not the sign of the
 * score.  'a' against 'A', mapped to one code and scored as a match, is an 'M' column that MD:Z lists as a mismatch.
 * Range: every result is exact while (n + m + 2) * max(max |submat|, |gap_open| + |gap_extend|) < 2^28; a pair beyond that is
 * PWA_E_CAPACITY.  Shape: patterns of at most 1024 symbols, else PWA_E_CAPACITY -- for the alignments AND for the scores (there is no
 * strip form).  An empty pair list is PWA_OK.
 *   pwa_align_subst_batch        pwa_align_gotoh_batch's arguments and outputs, (code, n_sym, submat) in place of (match, mismatch);
 *   pwa_align_subst_batch_cigar  likewise pwa_align_gotoh_batch_cigar's (too small a buffer: PWA_E_CAPACITY with the exact needed[]);
 *   pwa_subst_batch_create       a batch object like pwa_gotoh_batch_create's (pwa_batch_run / _d_scores / _set_d_scores / _fetch /
 *                                _info / _last_ms / _run_times / _destroy); pwa_batch_cell_bits and pwa_batch_profile_form are 0;
 *   pwa_scores_subst             the one-call form over lists of any size, as pwa_scores_gotoh; end cells when end_i_out or end_j_out
 *                                is given;
 *   pwa_align_subst_last_stats   device ms of the fills and walks of the last pwa_align_subst_batch(_cigar) on ctx, and their band
 *                                bytes (the gotoh and linear figures are kept apart).
 */
int pwa_align_subst_batch(pwa_ctx *ctx, int mode /* NW, SW, SG */, const uint8_t code[256], int n_sym, const int32_t *submat,
                          int gap_open, int gap_extend, const uint8_t *seq_bytes, const uint64_t *seq_off, uint32_t n_seq,
                          const uint32_t *pair_a, const uint32_t *pair_b, uint64_t n_pairs, int32_t *score_out, uint8_t *ops,
                          const uint64_t *ops_off, uint64_t *n_ops, uint64_t *end_cells /* 2*n_pairs or NULL */,
                          uint64_t *start_cells /* 2*n_pairs or NULL */);
int pwa_align_subst_batch_cigar(pwa_ctx *ctx, int mode, const uint8_t code[256], int n_sym, const int32_t *submat, int gap_open,
                                int gap_extend, const uint8_t *seq_bytes, const uint64_t *seq_off, uint32_t n_seq,
                                const uint32_t *pair_a, const uint32_t *pair_b, uint64_t n_pairs, int32_t *score_out,
                                char *cigar, uint64_t cigar_cap, uint64_t *cigar_off /* n_pairs + 1 */,
                                char *mdz, uint64_t mdz_cap, uint64_t *mdz_off /* n_pairs + 1 */,
                                uint64_t *end_cells /* 2*n_pairs or NULL */, uint64_t *start_cells /* 2*n_pairs or NULL */,
                                uint64_t needed[2] /* or NULL */);
int pwa_subst_batch_create(pwa_ctx *ctx, int mode, const uint8_t code[256], int n_sym, const int32_t *submat, int gap_open,
                           int gap_extend, const uint8_t *seq_bytes, const uint64_t *seq_off, uint32_t n_seq, const uint32_t *pair_a,
                           const uint32_t *pair_b, uint64_t n_pairs, int want_end_cells, pwa_batch **out);
int pwa_scores_subst(pwa_ctx *ctx, int mode, const uint8_t code[256], int n_sym, const int32_t *submat, int gap_open, int gap_extend,
                     const uint8_t *seq_bytes, const uint64_t *seq_off, uint32_t n_seq, const uint32_t *pair_a, const uint32_t *pair_b,
                     uint64_t n_pairs, int32_t *score_out, uint32_t *end_i_out, uint32_t *end_j_out);
int pwa_align_subst_last_stats(const pwa_ctx *ctx, float *fill_ms, float *walk_ms, uint64_t *band_bytes);

/*
 * BANDED affine-gap alignments and scores of long pairs UNDER A SUBSTITUTION MATRIX: the banded calls with the table of the block
 * above, for what neither family takes alone -- a protein of more than 1024 residues under BLOSUM-style scores, a long read or contig
 * with a neutral N, transitions scored apart from transversions, or folded lower case.
 *   pwa_align_banded_subst_batch        pwa_align_subst_batch's arguments, then band_lo, band_hi (one value each per list pair);
 *   pwa_align_banded_subst_batch_cigar  pwa_align_subst_batch_cigar's arguments, then the same two arrays;
 *   pwa_scores_banded_subst             pwa_scores_banded's arguments with (code, n_sym, submat) in place of (match, mismatch).
 * Semantics: exactly those of the banded block (pwa_align_banded_batch, pwa_scores_banded) -- the band, the boundary rule, the ends per
 * mode, validity, pairs with an empty side, the empty list (PWA_OK), PWA_RANGE_BYTES (the table is uploaded once per call and serves
 * every range; the scores form is not cut), the op regions and the string buffers -- with
 *   s(i,j) = submat[ code[p[i-1]] * n_sym + code[t[j-1]] ]
 * and code, n_sym, submat as in the substitution-matrix block: the table may be asymmetric and may hold any signs; both are copied
 * during the call.  CIGAR and MD:Z come from the ops and the RAW bytes: MD:Z reports byte identity, not the sign of the score.
 * Range: every result is exact while (n + m + 2) * max(max |submat|, |gap_open| + |gap_extend|, 1) < 2^28; a pair beyond that is
 * PWA_E_CAPACITY.  Shape: patterns and texts of any length the linear calls take; band width of at most 4096, else PWA_E_CAPACITY.
 * Checks, all before any device work: first the call's own, as pwa_align_subst_batch makes them (PWA_E_INVALID for a null code or
 * submat, n_sym outside 1 .. 32, a code[] entry >= n_sym, gap_open > 0 or gap_extend > 0, a null band_lo or band_hi with n_pairs > 0);
 * then per pair, in pair order, the band's validity, its width and the range rule (the first offending pair decides the error).
 * Why the sentinel of the banded kernels still lies below every real value: with A = max(max |submat|, |gap_open| + |gap_extend|, 1)
 * every H, E or F that stands for a path inside the band is a sum of at most n + m + 1 steps of magnitude <= A each, so |V| < 2^28 - A
 * under the range rule; the alignment fill's sentinel key -2^31 + 8 A + 1 is below every key V * 8 + 0..7, the score pass's plain
 * sentinel -2^30 below every V and V + gap_open + gap_extend, and a sentinel meets at most one gap extension (>= -A) before the sum is
 * compared and dropped.  Only |s| enters the bound: asymmetry and positive off-diagonal entries change nothing.
 * Stats: the alignment calls report into pwa_align_banded_last_stats, the score call into pwa_scores_banded_last_stats (its in-band
 * cell count means what it means there); pwa_align_subst_last_stats is not touched.  A call that fails validation leaves them unchanged.
 * Not offered: a batch object, named matrices.
 */
int pwa_align_banded_subst_batch(pwa_ctx *ctx, int mode /* NW, SW, SG */, const uint8_t code[256], int n_sym, const int32_t *submat,
                                 int gap_open, int gap_extend, const uint8_t *seq_bytes, const uint64_t *seq_off, uint32_t n_seq,
                                 const uint32_t *pair_a, const uint32_t *pair_b, uint64_t n_pairs, int32_t *score_out, uint8_t *ops,
                                 const uint64_t *ops_off, uint64_t *n_ops, uint64_t *end_cells /* 2*n_pairs or NULL */,
                                 uint64_t *start_cells /* 2*n_pairs or NULL */, const int32_t *band_lo /* n_pairs */,
                                 const int32_t *band_hi /* n_pairs */);
int pwa_align_banded_subst_batch_cigar(pwa_ctx *ctx, int mode, const uint8_t code[256], int n_sym, const int32_t *submat, int gap_open,
                                       int gap_extend, const uint8_t *seq_bytes, const uint64_t *seq_off, uint32_t n_seq,
                                       const uint32_t *pair_a, const uint32_t *pair_b, uint64_t n_pairs, int32_t *score_out,
                                       char *cigar, uint64_t cigar_cap, uint64_t *cigar_off /* n_pairs + 1 */,
                                       char *mdz, uint64_t mdz_cap, uint64_t *mdz_off /* n_pairs + 1 */,
                                       uint64_t *end_cells /* 2*n_pairs or NULL */, uint64_t *start_cells /* 2*n_pairs or NULL */,
                                       uint64_t needed[2] /* or NULL */, const int32_t *band_lo /* n_pairs */,
                                       const int32_t *band_hi /* n_pairs */);
int pwa_scores_banded_subst(pwa_ctx *ctx, int mode /* NW, SW, SG */, const uint8_t code[256], int n_sym, const int32_t *submat,
                            int gap_open, int gap_extend, const uint8_t *seq_bytes, const uint64_t *seq_off, uint32_t n_seq,
                            const uint32_t *pair_a, const uint32_t *pair_b, uint64_t n_pairs, int32_t *score_out,
                            uint32_t *end_i_out /* or NULL */, uint32_t *end_j_out /* or NULL */, const int32_t *band_lo /* n_pairs */,
                            const int32_t *band_hi /* n_pairs */);

/*
 * The -g selection without the op lists: hw2.cpp:342-350 keeps, of every pair's global alignment, only
 * overlapLongestExactMatch(alignedPattern, alignedReference) (hw2.cpp:267-278) and the score.  Same fill and
 * traceback band as pwa_align_batch; the device walk looks at the symbols under each run of diagonal moves
 * and returns the longest run of equal, gap-free columns -- no op list is written or copied back.  The
 * caller then asks pwa_align for the ONE winning pair (first strictly larger overlap, hw2.cpp:346).
 *   score_out[k]   : as pwa_align_batch;   overlap_out[k] : as pwa_alignment_overlap on that pair's walk
 * Modes NW and SW only (PWA_MODE_SG: PWA_E_INVALID).
 */
int pwa_overlaps(pwa_ctx *ctx, int mode, int match, int mismatch, int gap, const uint8_t *seq_bytes,
                 const uint64_t *seq_off, uint32_t n_seq, const uint32_t *pair_a, const uint32_t *pair_b, uint64_t n_pairs,
                 int32_t *score_out, int32_t *overlap_out);

/*
 * FASTA ingest (no GPU work): readFasta (hw2.cpp:25-57) on one or more files, straight into the layout the
 * entries above consume -- ONE byte blob and n_seq + 1 offsets -- parsed by n_threads threads (<= 0: one per
 * host core, at most 16) over the mmap'ed file.  Semantics are the reference's, byte for byte: header text is
 * dropped, lines are joined after stripping trailing '\r' / whitespace, blank lines are skipped, records with an
 * empty body are dropped, bytes ahead of the first header form a record.  Sequences of paths[i] are
 * first_seq[i] .. first_seq[i + 1] - 1.  PWA_E_IO when a file cannot be opened (the reference prints
 * "Error: Cannot open file <name>" and exits 1, hw2.cpp:28-31): *failed_path is its index.
 */
typedef struct pwa_fasta pwa_fasta;
int pwa_fasta_read(const char *const *paths, int n_paths, int n_threads, pwa_fasta **out, int *failed_path /* or NULL */);
uint32_t pwa_fasta_n_seq(const pwa_fasta *f);
const uint8_t *pwa_fasta_bytes(const pwa_fasta *f);
const uint64_t *pwa_fasta_offsets(const pwa_fasta *f);   /* n_seq + 1 */
const uint32_t *pwa_fasta_first_seq(const pwa_fasta *f); /* n_paths + 1 */
void pwa_fasta_free(pwa_fasta *f);

/*
 * Suffix-array index of one text (hw1, multiple_pattern_matching.cpp): the sorted suffixes that the reference's Ukkonen
 * tree (50-281) encodes, built on the device by prefix doubling over a device radix sort, then searched by many patterns
 * at once.  Suffixes are ordered by bytes as SIGNED char (the reference's std::map<char, ...>, 40), a suffix before every
 * longer one it is a prefix of.
 *   pwa_sa_create       uploads text[0 .. n) and builds its suffix array on the context's GPU; n < 2^31 (positions are
 *                       int32 in the reference), PWA_E_CAPACITY otherwise;
 *   pwa_sa_fetch        sa_out[n]: the suffix array (start positions in sorted order);
 *   pwa_sa_find         counts_out[n_pat]: exact occurrences of each pattern anywhere in the text (pattern k is
 *                       pat_bytes[pat_off[k] .. pat_off[k + 1])); an empty pattern occurs at every position;
 *   pwa_sa_occurrences  the occurrences the reference reports (search 168-200 + the grouping at 390-431): reference r is
 *                       text[ref_start[r] .. ref_start[r + 1]) whose LAST byte is its terminator (ref_start[0] = 0,
 *                       ref_start[n_ref] = n, strictly increasing); hits on a terminator are dropped, every other hit p of
 *                       reference r is the key header_rank[r] << 32 | (p - ref_start[r]).  Pattern k's keys are
 *                       occ[occ_off[k] .. occ_off[k + 1]) in ascending order (occ_off: n_pat + 1 entries).  Patterns are
 *                       processed in chunks whose raw hits fit a device budget.  PWA_E_CAPACITY with *needed set when
 *                       cap < the number of keys (the sum of pwa_sa_find's counts always suffices);
 *   pwa_sa_last_stats   rounds of the build (the first sort included), device ms of the build (events), host ms of the
 *                       last find / occurrences call.
 * The text's positions are searched on the device only: there is no CPU path.
 */
typedef struct pwa_sa_index pwa_sa_index;
int pwa_sa_create(pwa_ctx *ctx, const uint8_t *text, uint64_t n, pwa_sa_index **out);
int pwa_sa_fetch(pwa_sa_index *ix, uint32_t *sa_out);
int pwa_sa_find(pwa_sa_index *ix, const uint8_t *pat_bytes, const uint64_t *pat_off, uint32_t n_pat, uint32_t *counts_out);
int pwa_sa_occurrences(pwa_sa_index *ix, const uint8_t *pat_bytes, const uint64_t *pat_off, uint32_t n_pat, const uint32_t *ref_start,
                       uint32_t n_ref, const uint32_t *header_rank, uint64_t *occ_off, uint64_t *occ, uint64_t cap, uint64_t *needed);
int pwa_sa_last_stats(const pwa_sa_index *ix, uint32_t *rounds, float *build_ms, float *search_ms);
void pwa_sa_destroy(pwa_sa_index *ix);

/* ---- Seeding a list of reads against a kept index: the exact k-mer anchors that pwa_chain_anchors takes
 *
 * The index is a pwa_sa_index of the text as given -- no terminator is appended -- created once and used for any number of calls.
 * Reads.  Read r is read_bytes[read_off[r] .. read_off[r + 1]).  Its slots are q = 0, step, 2 step, ... while q + k <= len: that is
 * (len - k) / step + 1 slots, or 0 when len < k.
 * Hits.  A slot's hits are every t with t + k <= n and text[t .. t + k) == read[q .. q + k) as raw bytes; any byte value is legal, NUL
 * and >= 0x80 included.  The search treats a suffix shorter than k as smaller, so no hit runs past n.  A slot with more than max_occ hits
 * contributes none.
 * Anchors.  Read r's anchors are its slots' hits in ascending (t, q).  Every anchor has len = k, so this is the (t + len, q + len)
 * order of the chaining call.  Read r's anchors are entries anc_off_out[r] .. anc_off_out[r + 1]) of anc_t and anc_q.
 * On the device: the k-mers are cut out of the read blob by the search kernel, each k-mer is searched once, the hits are gathered and
 * sorted there; nothing per k-mer is built on the host.
 * Validation runs before any device work.  First a null required pointer, or k, step or max_occ equal to 0, PWA_E_INVALID; then in
 * read order, the first offending read decides: read_off decreasing PWA_E_INVALID; a read of 2^31 bytes or more PWA_E_CAPACITY (the
 * chaining call needs q + k < 2^31); a read whose worst-case hits, slots x min(max_occ, max(n - k + 1, 0)), reach 2^32
 * PWA_E_CAPACITY; then a total of 2^32 slots or more PWA_E_CAPACITY.  n_reads = 0, n < k and a list without a slot are valid calls:
 * they do no device work, and anc_off_out is all zeros.
 * Ranges.  Consecutive reads run together as long as the sum of their worst-case hits stays within PWA_OCC_CHUNK_HITS, else the
 * library's budget (2^27); one read alone may exceed it.  A range without a slot launches nothing and is not counted.  The device
 * buffers of a range's hits are sized from the hits it has, not from the worst case.
 *   pwa_seed_plan           host only, no context, no GPU: the validation code of the same inputs for a text of text_n bytes,
 *                           *bad_read = the first offending read (0xFFFFFFFF: none, or a pointer, a parameter or the total was at
 *                           fault), *n_slots = the list's slots, *n_ranges = the ranges the call would run under budget_hits (0: the
 *                           library's budget); both are 0 with an error.  bad_read, n_slots and n_ranges may be NULL.
 *   pwa_sa_seed             runs the seeding, writes anc_off_out[n_reads + 1], and keeps the call's anchors with the index until the
 *                           next pwa_sa_seed on it or pwa_sa_destroy (sizing with cap = 0 and calling again would search twice).
 *   pwa_sa_seed_fetch       copies the kept anchors out; PWA_E_CAPACITY when cap < anc_off_out[n_reads], PWA_E_INVALID when no
 *                           seeding has run on the index (or the last one failed on the device).
 *   pwa_sa_seed_last_stats  of the last pwa_sa_seed on ix: device ms of the search kernel and of gather + sort + split (events,
 *                           summed over the ranges), the list's slots, the hits kept, the ranges run.  Any pointer may be NULL; a
 *                           call that fails validation leaves them, and the kept anchors, unchanged. */
int pwa_seed_plan(uint64_t text_n, const uint64_t *read_off /* n_reads + 1 */, uint32_t n_reads, uint32_t k, uint32_t step,
                  uint32_t max_occ, uint64_t budget_hits, uint32_t *bad_read /* or NULL */, uint64_t *n_slots /* or NULL */,
                  uint64_t *n_ranges /* or NULL */);
int pwa_sa_seed(pwa_sa_index *ix, const uint8_t *read_bytes, const uint64_t *read_off /* n_reads + 1 */, uint32_t n_reads, uint32_t k,
                uint32_t step, uint32_t max_occ, uint64_t *anc_off_out /* n_reads + 1 */);
int pwa_sa_seed_fetch(const pwa_sa_index *ix, uint32_t *anc_t, uint32_t *anc_q, uint64_t cap);
int pwa_sa_seed_last_stats(const pwa_sa_index *ix, float *search_ms, float *sort_ms, uint64_t *slots, uint64_t *hits, uint64_t *ranges);

/* ---- Minimizer sketches, a minimizer index, seeding against it
 *
 * Codes.  Byte 'A' is 0, 'C' 1, 'G' 2, 'T' 3, uppercase only.  Every other byte value -- lowercase, 'N', NUL, >= 0x80 -- makes each
 * k-mer that covers it invalid.  An anchor therefore always means text[t .. t + k) == read[q .. q + k) as raw bytes, as in pwa_sa_seed.
 * k-mer value and hash.  1 <= k <= 31.  v(p) = sum of code(s[p + i]) * 4^(k - 1 - i), the first symbol most significant;
 * h(p) = mix(v(p), 2^(2k) - 1), where mix(key, mask) is, in this order,
 *   key = (~key + (key << 21)) & mask;  key ^= key >> 24;  key = (key + (key << 3) + (key << 8)) & mask;  key ^= key >> 14;
 *   key = (key + (key << 2) + (key << 4)) & mask;  key ^= key >> 28;  key = (key + (key << 31)) & mask.
 * It is a bijection on 2k bits: equal hashes mean equal k-mers, so a lookup by hash is exact.  An invalid k-mer compares as
 * +infinity, above every valid hash (those are below 2^62).
 * Windows.  1 <= w <= 128.  A sequence of L bytes has K = L - k + 1 k-mers (0 when L < k) at starts 0 .. K - 1.  If K >= w the
 * windows are [s, s + w) for s = 0 .. K - w; if 1 <= K < w there is one window, [0, K).  A window selects its valid k-mer of smallest
 * hash, the leftmost one among equals; a window with no valid k-mer selects nothing.  The sketch is the set of distinct selected
 * starts in ascending order, each with its hash.  With w = 1 the sketch is every valid k-mer.  Equivalently, start p is selected iff
 * it is valid and some window W that holds p has h(j) > h(p) for all j < p in W and h(j) >= h(p) for all j > p in W.
 * Index.  The sketch of the text as given, n < 2^31 bytes, stored as pairs (hash, t) in ascending (hash, t); n_min is its size.
 * n < k gives a valid, empty index.  Its size and build cost scale with the sketch: nothing per text position is kept.
 * Seeding.  Each sketch entry (q, h) of read r hits every index entry with hash h; an entry with more than max_occ hits contributes
 * none (occurrences are counted among the text's minimizers, not among all text positions).  Read r's anchors are (t, q) with
 * len = k in ascending (t, q), the order pwa_chain_anchors requires, entries anc_off_out[r] .. anc_off_out[r + 1]) of anc_t and anc_q.
 * On the device: one lane per k-mer start hashes it from the blob, a workgroup stages a tile's hashes with a halo of w - 1 in LDS,
 * each lane decides by the local form among the neighbours of its own sequence, and the selected starts are compacted in position
 * order; the read minimizers are looked up by binary search over the sorted hashes; the hits are gathered and sorted there.
 * Validation runs before any device work; the first offending item decides the code.  pwa_mm_create and pwa_mm_sketch: a null
 * required pointer PWA_E_INVALID; k outside 1 .. 31 or w outside 1 .. 128 PWA_E_INVALID; then in sequence order, offsets decreasing
 * PWA_E_INVALID, a text or sequence of 2^31 bytes or more PWA_E_CAPACITY.  pwa_mm_seed and pwa_mm_plan follow pwa_seed_plan's rule
 * with step = 1 and the text's k-mer count replaced by n_min: a null pointer or max_occ = 0 (for the plan also k outside 1 .. 31)
 * PWA_E_INVALID; then in read order read_off decreasing PWA_E_INVALID, a read of 2^31 bytes or more PWA_E_CAPACITY, worst-case hits
 * (len - k + 1) x min(max_occ, n_min) of 2^32 or more PWA_E_CAPACITY; then a total of 2^32 k-mers or more PWA_E_CAPACITY.
 * n_reads = 0, an empty index and reads shorter than k are valid calls with all-zero offsets.
 * Ranges.  The same greedy cut over worst-case hits as pwa_sa_seed, under PWA_OCC_CHUNK_HITS or else 2^27; one read alone may exceed
 * it.  A range without a k-mer is not run or counted.  pwa_mm_sketch cuts its list the same way by k-mers under the same budget.
 *   pwa_mm_create           uploads text[0 .. n), sketches it and sorts the pairs on the context's GPU; the text is not kept.
 *   pwa_mm_fetch            copies the sorted entries out: hash_out[n_min], pos_out[n_min]; PWA_E_CAPACITY when cap < n_min.
 *   pwa_mm_last_stats       n_min, and the device ms of sketch + sort (events).  Either pointer may be NULL.
 *   pwa_mm_sketch           the sketches of a sequence list: sequence r's entries are min_off_out[r] .. min_off_out[r + 1]) of
 *                           pos_out and hash_out, in ascending position.  PWA_E_CAPACITY with *needed set (needed may be NULL) and
 *                           min_off_out complete when cap is too small; the total k-mer count always suffices as cap.
 *   pwa_mm_plan             host only, no context, no GPU: pwa_seed_plan for an index of n_min entries -- the validation code,
 *                           *bad_read (0xFFFFFFFF: none, or a pointer, a parameter or the total was at fault), *n_slots = the
 *                           list's k-mers, *n_ranges under budget_hits (0: the library's budget); the last three may be NULL.
 *   pwa_mm_seed             runs the seeding, writes anc_off_out[n_reads + 1], and keeps the call's anchors with the index until the
 *                           next pwa_mm_seed on it or pwa_mm_destroy.
 *   pwa_mm_seed_fetch       copies the kept anchors out; PWA_E_CAPACITY when cap < anc_off_out[n_reads], PWA_E_INVALID when no
 *                           seeding has run on the index (or the last one failed on the device).
 *   pwa_mm_seed_last_stats  of the last pwa_mm_seed on ix: device ms of the sketch passes, of the lookup kernel and of gather + sort
 *                           + split (events, summed over the ranges); slots = the k-mers examined, minimizers = the read minimizers
 *                           looked up, the hits kept, the ranges run.  Any pointer may be NULL; a call that fails validation leaves
 *                           them, and the kept anchors, unchanged.
 * A kernel that finds one of its bounds violated sets the call's fault word; the call then returns PWA_E_HIP. */
typedef struct pwa_mm_index pwa_mm_index;
int pwa_mm_create(pwa_ctx *ctx, const uint8_t *text, uint64_t n, uint32_t k, uint32_t w, pwa_mm_index **out);
void pwa_mm_destroy(pwa_mm_index *ix);
int pwa_mm_fetch(pwa_mm_index *ix, uint64_t *hash_out, uint32_t *pos_out, uint64_t cap);
int pwa_mm_last_stats(const pwa_mm_index *ix, uint64_t *n_min, float *build_ms);
int pwa_mm_sketch(pwa_ctx *ctx, const uint8_t *seq_bytes, const uint64_t *seq_off /* n_seqs + 1 */, uint32_t n_seqs, uint32_t k, uint32_t w,
                  uint64_t *min_off_out /* n_seqs + 1 */, uint32_t *pos_out, uint64_t *hash_out, uint64_t cap, uint64_t *needed /* or NULL */);
int pwa_mm_plan(uint64_t n_min, const uint64_t *read_off /* n_reads + 1 */, uint32_t n_reads, uint32_t k, uint32_t max_occ,
                uint64_t budget_hits, uint32_t *bad_read /* or NULL */, uint64_t *n_slots /* or NULL */, uint64_t *n_ranges /* or NULL */);
int pwa_mm_seed(pwa_mm_index *ix, const uint8_t *read_bytes, const uint64_t *read_off /* n_reads + 1 */, uint32_t n_reads, uint32_t max_occ,
                uint64_t *anc_off_out /* n_reads + 1 */);
int pwa_mm_seed_fetch(const pwa_mm_index *ix, uint32_t *anc_t, uint32_t *anc_q, uint64_t cap);
int pwa_mm_seed_last_stats(const pwa_mm_index *ix, float *sketch_ms, float *search_ms, float *sort_ms, uint64_t *slots, uint64_t *minimizers,
                           uint64_t *hits, uint64_t *ranges);

/* ---- Canonical minimizers: one sketch, both strands
 *
 * Codes, mix, the windows, the leftmost tie, the invalid bytes and the limits on k and w are those of the minimizer block above.
 * Canonical value and strand.  A k-mer at start p with codes c_0 .. c_(k-1) has the forward value f(p) = sum of c_i * 4^(k - 1 - i)
 * and the reverse-complement value r(p) = sum of (3 - c_i) * 4^i, the value of the k-mer read off the other strand.  If f < r the
 * strand bit s(p) = 0 and h(p) = mix(f); if r < f then s(p) = 1 and h(p) = mix(r); if f = r (a reverse palindrome, possible only for
 * even k) the k-mer is invalid: +infinity, never selected, like a k-mer over 'N'.  A k-mer and its reverse complement so have the
 * same hash and opposite strand bits.  Window selection runs over h exactly as above.
 * Sketch.  The selected starts in ascending order, each with its hash and its strand bit.
 * Index.  The text's canonical sketch as (hash, t, strand) in ascending (hash, t).
 * Seeding.  Read r of L bytes is sketched once, as given.  A sketch entry (q, h, s_q) hits every index entry (h, t, s_t); an entry
 * with more than max_occ hits contributes none, the count being over both strands together.  A hit with s_q = s_t goes to list 2r
 * as the forward anchor (t, q): text[t .. t + k) == read[q .. q + k).  A hit with s_q != s_t goes to list 2r + 1 as the reverse
 * anchor (t, L - k - q): text[t .. t + k) == revcomp(read)[q' .. q' + k) with q' = L - k - q.  Each list is in ascending (t, q), the
 * order pwa_chain_anchors requires, in the coordinates of the sequence that list would be aligned as.  Lists 2r and 2r + 1 are
 * consecutive in the kept anchors: list i is entries anc_off_out[i] .. anc_off_out[i + 1]), i = 0 .. 2 n_reads - 1.
 * Not promised: the sketch of revcomp(x) is not always the mirror of the sketch of x (the leftmost tie is not symmetric), so the
 * two lists of a read are not always what two plain seedings of the read and of its reverse complement would give.
 * The type stays pwa_mm_index; an index is plain (pwa_mm_create) or canonical (pwa_mm_create_canonical) for its lifetime, and each
 * wrong pairing of a call and an index kind is PWA_E_INVALID with a message that names the other call.  Validation order and codes
 * are those of the siblings above.
 *   pwa_mm_create_canonical  pwa_mm_create with canonical hashes; the strand bits are kept with the positions.
 *   pwa_mm_fetch_canonical   pwa_mm_fetch plus strand_out[n_min] (0 or 1).  On a plain index PWA_E_INVALID.  pwa_mm_fetch on a
 *                            canonical index gives hash and t alone.
 *   pwa_mm_sketch_canonical  pwa_mm_sketch plus strand_out, one byte (0 or 1) beside every pos_out entry.
 *   pwa_mm_seed_strands      the seeding above: writes anc_off_out[2 n_reads + 1] and keeps the anchors as pwa_mm_seed does;
 *                            pwa_mm_seed_fetch and pwa_mm_seed_last_stats serve it unchanged, minimizers counting each read
 *                            minimizer once.  On a plain index PWA_E_INVALID, as pwa_mm_seed is on a canonical one.  n_reads is at
 *                            most 2^31 - 1 so that list numbers fit 32 bits; above that PWA_E_CAPACITY.
 *   pwa_mm_plan              is the plan of pwa_mm_seed_strands as it stands: a read minimizer still has at most
 *                            min(max_occ, n_min) hits, now summed over the two lists of its read, so the worst case per read, the
 *                            ranges and the codes are the same.
 * On the device the strand bit travels as bit 31 of the position word (positions are below 2^31); nothing per text position is kept. */
int pwa_mm_create_canonical(pwa_ctx *ctx, const uint8_t *text, uint64_t n, uint32_t k, uint32_t w, pwa_mm_index **out);
int pwa_mm_fetch_canonical(pwa_mm_index *ix, uint64_t *hash_out, uint32_t *pos_out, uint8_t *strand_out, uint64_t cap);
int pwa_mm_sketch_canonical(pwa_ctx *ctx, const uint8_t *seq_bytes, const uint64_t *seq_off /* n_seqs + 1 */, uint32_t n_seqs, uint32_t k,
                            uint32_t w, uint64_t *min_off_out /* n_seqs + 1 */, uint32_t *pos_out, uint64_t *hash_out, uint8_t *strand_out,
                            uint64_t cap, uint64_t *needed /* or NULL */);
int pwa_mm_seed_strands(pwa_mm_index *ix, const uint8_t *read_bytes, const uint64_t *read_off /* n_reads + 1 */, uint32_t n_reads,
                        uint32_t max_occ, uint64_t *anc_off_out /* 2 n_reads + 1 */);

/* ---- k-edit approximate pattern search (Sellers' DP on bit-parallel columns, Myers 1999)
 *
 * For a pattern p of m >= 1 bytes and a text t of n bytes:  D[0][j] = 0, D[i][0] = i,
 *   D[i][j] = min(D[i-1][j-1] + (p[i-1] != t[j-1]), D[i-1][j] + 1, D[i][j-1] + 1),
 * bytes compared as bytes.  A hit of pattern q is every end e in 1 .. n with D[m][e] <= max_dist[q]; its distance is D[m][e].  e = 0 is
 * never a hit; max_dist >= m is legal (every end is then a hit, with its exact distance).  Pattern q is
 * pat_bytes[pat_off[q] .. pat_off[q + 1]).
 *   pwa_approx_find         counts_out[n_pat]: hits per pattern.  best_dist_out / best_end_out (each may be NULL): the smallest distance
 *                           and, among the hits of that distance, the smallest end; -1 and 0 for a pattern without a hit.  One pass over
 *                           the text (the count pass).
 *   pwa_approx_occurrences  pattern q's hits are occ[occ_off[q] .. occ_off[q + 1]), in ascending end, occ[x] = (uint64_t)e << 32 | dist.
 *                           The count pass, then the fill pass, whose hits are staged on the device in slices of whole tasks.
 *                           PWA_E_CAPACITY with *needed set (needed may be NULL) when cap < the number of hits; occ_off is complete
 *                           then, occ is untouched.  The sum of pwa_approx_find's counts always suffices.
 *   pwa_approx_last_stats   of the last of the two calls on ctx: device ms of the count and of the fill pass (events; fill_ms is 0 after
 *                           pwa_approx_find), the number of tasks, and the text columns they scanned, warm-up included.
 *   pwa_approx_plan         host only, no context, no GPU: the task list the two calls run.  A task is (pattern, report columns [lo, hi),
 *                           first scanned column scan_lo): the scan starts from the fresh column D[i] = i at scan_lo and reports ends
 *                           lo + 1 .. hi.  Per pattern the [lo, hi) tile [0, n) in ascending order with hi - lo <= chunk, tasks come in
 *                           (pattern, lo) order, and scan_lo = max(0, lo - w) rounded down to a multiple of 16, w = m + min(max_dist, m):
 *                           an alignment of cost <= max_dist spans at most that many columns, so a hit is recomputed exactly, and a
 *                           fresh start only raises values, so nothing else becomes one.  *n_tasks receives the number of tasks;
 *                           PWA_E_CAPACITY when cap is smaller (call with cap = 0 to size the arrays, which may then be NULL).
 *                           PWA_E_INVALID for chunk = 0, a pattern length of 0, or a null pat_len / max_dist / n_tasks.
 * Limits, checked before any device work: null ctx or a null required pointer PWA_E_INVALID; n >= 2^31 PWA_E_CAPACITY; then in
 * pattern order m = 0 PWA_E_INVALID and m > 512 PWA_E_CAPACITY; more than 32 distinct byte values over all patterns of the call
 * PWA_E_CAPACITY (text bytes that no pattern contains are legal and match nothing).  n = 0 or n_pat = 0: a valid call without hits. */
int pwa_approx_find(pwa_ctx *ctx, const uint8_t *text, uint64_t n, const uint8_t *pat_bytes, const uint64_t *pat_off,
                    uint32_t n_pat, const uint32_t *max_dist, uint32_t *counts_out,
                    int32_t *best_dist_out /* or NULL */, uint32_t *best_end_out /* or NULL */);
int pwa_approx_occurrences(pwa_ctx *ctx, const uint8_t *text, uint64_t n, const uint8_t *pat_bytes, const uint64_t *pat_off,
                           uint32_t n_pat, const uint32_t *max_dist, uint64_t *occ_off /* n_pat + 1 */, uint64_t *occ,
                           uint64_t cap, uint64_t *needed);
int pwa_approx_last_stats(const pwa_ctx *ctx, float *count_ms, float *fill_ms, uint64_t *tasks, uint64_t *columns);
int pwa_approx_plan(uint64_t n, const uint32_t *pat_len, const uint32_t *max_dist, uint32_t n_pat, uint32_t chunk,
                    uint32_t *task_pat, uint64_t *task_scan_lo, uint64_t *task_lo, uint64_t *task_hi, uint64_t cap,
                    uint64_t *n_tasks);

/* ---- from a hit to a placement: start positions and locally minimal ends of k-edit hits
 *
 * With ed(a, b) the unit-cost edit distance (the recurrence above with D[0][j] = j), the start of a hit (q, e, d) is the LARGEST
 * s <= e with ed(p_q, text[s .. e)) <= d: the shortest occurrence that ends at e.  For a true hit d = D[m][e] is the minimum over all
 * starts, so equality is reached and m - d <= e - s <= min(e, m + d); s = e (the empty substring) is the answer when d = m.
 *   pwa_approx_starts       start_out[x] = the start of hit occ[x], for x in occ_off[0] .. occ_off[n_pat) -- start_out is parallel to
 *                           occ, whose base is occ_off[0].  occ / occ_off are what pwa_approx_occurrences writes (pattern q's hits are
 *                           occ[occ_off[q] .. occ_off[q + 1]), occ[x] = (uint64_t)e << 32 | dist); any subset, any order within a
 *                           pattern and duplicates are legal.  One lane per hit runs the anchored column of the reversed pattern
 *                           backwards from e over at most min(e, m + dist) text symbols; the hits go to the device in slices of at
 *                           most PWA_OCC_CHUNK_HITS records.  A dist below the true D[m][e] is not an error: the scan stops at that
 *                           bound and writes PWA_APPROX_NO_START.  A dist above it gives the first column at which row m reaches it
 *                           (row m moves by +-1 per column from m down, so "<= dist" and "= dist" coincide).
 *                           Limits: those of pwa_approx_find, checked in the same order, before any device work; then, in list
 *                           order, PWA_E_INVALID for occ_off not ascending, a hit with e = 0, with e > n, or with dist > m; more than
 *                           2^32 - 1 hits PWA_E_CAPACITY.  No hits or n_pat = 0: a valid call.
 *   pwa_approx_starts_last_stats  of the last pwa_approx_starts on ctx: device ms of the pass (events: coding the text, the masks,
 *                           the scans of every slice), the hits run, the text columns they scanned.
 *   pwa_approx_minima       host only, no context, no GPU: thins the COMPLETE ascending hit list of pwa_approx_occurrences for the
 *                           same n, lengths and bounds down to its locally minimal ends, in place (occ compacted, occ_off rewritten
 *                           from occ_off[0] on).  With k' = min(max_dist, m), c(e) = dist of the hit at e, c(e) = k' + 1 for an end
 *                           1 <= e <= n without a hit and c(0) = m, a hit at e is kept iff c(e - 1) > c(e) and, with f the last
 *                           column of the run c(e) = c(e + 1) = ... = c(f), f = n or c(f + 1) > c(e): the leftmost end of every
 *                           plateau entered by a descent and left by a rise, the text end counting as a rise.  Exact without the DP
 *                           row: an end missing from the list has D[m][e] > k', above every hit, and clipping it to k' + 1 changes
 *                           no comparison that involves a hit.  PWA_E_INVALID (nothing is changed then) for a null pointer, a
 *                           pattern length of 0, offsets not ascending, ends not strictly ascending within a pattern, an end outside
 *                           1 .. n, or dist > k'. */
#define PWA_APPROX_NO_START 0xffffffffu
int pwa_approx_starts(pwa_ctx *ctx, const uint8_t *text, uint64_t n, const uint8_t *pat_bytes, const uint64_t *pat_off,
                      uint32_t n_pat, const uint64_t *occ_off /* n_pat + 1 */, const uint64_t *occ /* e << 32 | dist */,
                      uint32_t *start_out /* parallel to occ */);
int pwa_approx_starts_last_stats(const pwa_ctx *ctx, float *ms, uint64_t *hits, uint64_t *columns);
int pwa_approx_minima(uint64_t n, const uint32_t *pat_len, const uint32_t *max_dist, uint32_t n_pat,
                      uint64_t *occ_off /* in: n_pat + 1; out: of the kept hits */, uint64_t *occ /* compacted in place */);

/* ---- Wavefront alignments: exact affine-gap GLOBAL alignments of long pairs without a band (WFA, Marco-Sola et al. 2021)
 *
 * The gotoh block's scoring and conventions (match, mismatch, gap_open, gap_extend; a gap of length L scores gap_open + L * gap_extend;
 * equality on raw bytes, NUL and '-' included), mode NW only: from (0, 0) to (n, m), pattern = pair_a (rows, i), text = pair_b (j).
 * The sweep is by PENALTY, not by cell, so work and memory grow with how much a pair differs, not with its size: no limit on the
 * pattern length, no band to guess.  Penalties:
 *   x0 = 2 (match - mismatch)   o0 = -2 gap_open   e0 = match - 2 gap_extend
 *   g = gcd(x0, o0, e0) (gcd with 0 is the other value)   x, o, e = x0 / g, o0 / g, e0 / g
 * PWA_E_INVALID unless gap_open <= 0, gap_extend <= 0, match > mismatch and match - 2 gap_extend > 0.  An alignment with penalty P
 * scores (match (n + m) - g P) / 2; the division is exact.  Range rule as for gotoh: (n + m + 2) * max(|match|, |mismatch|,
 * |gap_open| + |gap_extend|) < 2^28, else PWA_E_CAPACITY.
 * Wavefronts: the offset is the text index j, the diagonal k = j - i, NULL is -inf; an offset is kept only when 0 <= j <= m and
 * 0 <= j - k <= n, otherwise it is NULL, and that holds for every term below before a max is taken.
 *   I[s][k] = max(M[s-o-e][k-1], I[s-e][k-1]) + 1          ('I': text symbol against a gap)
 *   D[s][k] = max(M[s-o-e][k+1], D[s-e][k+1])              ('D': pattern symbol against a gap)
 *   M[s][k] = extend(max(M[s-x][k] + 1, I[s][k], D[s][k]))  extend: j++ while i < n, j < m, p[i] == t[j]
 *   M[0][0] = extend(0); the sweep ends at the first s with M[s][m-n] == m; that s is the pair's penalty P
 * Wavefront s spans the diagonals [max(-n, -khi(s)), min(m, khi(s))], khi(s) = 0 for s < o + e, else (s - o) div e; width(s) is the
 * number of those diagonals.  A score whose wavefronts s - x, s - o - e and s - e are all empty (or below 0) is empty.
 * Backtrace: from state M at (P, m - n, m); ops in traceback order, as every other call writes them.  In M at s > 0: v = the max of the
 * three sources (the value before the extend); emit j - v 'M'; on ties mismatch >= I >= D (mirrors diag >= E >= F); a mismatch emits
 * one more 'M' and goes to (s - x, k, v - 1); I or D switch state on the same (s, k) with j = v.  In I: emit 'I', go to (k - 1, j - 1);
 * a tie OPENS: M[s-o-e][k-1] >= I[s-e][k-1] goes to M at s - o - e, otherwise stay in I at s - e.  D likewise with 'D', k + 1 and j
 * unchanged.  At s = 0: emit j 'M' and stop.  The op list is an optimal alignment; between ties it is chosen by these rules, not by
 * the DP walk's, so it need not equal pwa_align_gotoh_batch's byte for byte.
 * Bound: min_score[k] (the pointer may be NULL: no bound) is the lowest score worth finding for pair k.  With P_worst the penalty of
 * "n 'D' then m 'I'", (o + n e if n > 0) + (o + m e if m > 0),  P_max = min(P_worst, floor((match (n + m) - 2 min_score) / g)), and
 * the sweep never goes beyond P_max.  A pair whose optimum scores below min_score[k] is NOT FOUND: P_max < 0, or P_max < o + |n - m| e
 * for n != m (both decided on the host, no device work for the pair), or the sweep reaches P_max without ending.  Then
 * score_out[k] = PWA_WFA_NONE, penalty_out[k] = 0xffffffff, n_ops[k] = 0, and CIGAR and MD:Z are both of length 0.  A found pair with
 * an empty side follows the gotoh NW conventions ("nD" / "0^<pattern>0", "mI" / "0", "" / "0").
 * cells(k) = the sum of width(s) over s = 0 .. P_max is the planning unit: the alignment calls keep every wavefront, 12 bytes of
 * device workspace per planned cell; the score call keeps a ring of max(x, o + e) + 1 wavefronts per pair.  The workspace is processed
 * in ranges of consecutive pairs under the PWA_RANGE_BYTES budget (default min(0.6 free, 48 GiB)); a range holds at least one pair, and
 * PWA_E_NOMEM when that pair cannot be allocated.  Give a bound for long pairs: without one the plan reaches P_worst.
 *   pwa_wfa_plan             host only, no context: validation, the conversion (pen = x, o, e, g) and per pair P_max and cells (either
 *                            may be NULL); a pair not found on the host gets cells = 0 and p_max = UINT64_MAX.
 *   pwa_scores_wfa           score_out[k], and penalty_out[k] = P (penalty_out may be NULL).
 *   pwa_align_wfa_batch      score_out, and the op lists with pwa_align_gotoh_batch's op-region layout (ops_off, n_ops).
 *   pwa_align_wfa_batch_cigar  the same alignments as CIGAR and MD:Z strings with pwa_align_gotoh_batch_cigar's string buffers and
 *                            PWA_E_CAPACITY / needed protocol; the strings equal pwa_format_alignment of the op list byte for byte
 *                            (formatted on the host from the op lists).  No end or start cells: always (n, m) and (0, 0).
 *   pwa_align_wfa_codes_batch, pwa_align_wfa_codes_batch_cigar   the same two calls in the low-memory form below: parameters, validation,
 *                            bound, results, op lists, strings and the capacity protocol are pwa_align_wfa_batch(_cigar)'s, and the op
 *                            list equals pwa_align_wfa_batch's byte for byte; only the device workspace differs.
 *   pwa_wfa_last_stats       of the last of these calls on ctx: device ms of the sweeps and the walks (events), cells = the sum over
 *                            the pairs of width(s) for s = 0 .. P (P_max for a pair the sweep did not find, nothing for one decided on
 *                            the host), and the bytes of the largest range's wavefront workspace.  A call that fails validation
 *                            leaves them unchanged.
 * Validation runs before any device work, in pair order: a null context, a null required pointer, an index >= n_seq PWA_E_INVALID;
 * the scoring first.  An empty pair list is PWA_OK.
 * The codes form.  The backtrace above asks three things of a cell, and the sweep knows all three when it computes the cell, so the
 * codes calls keep one byte per planned cell instead of three offsets and run the sweep on the score call's ring:
 *   bits 0-1  where M[s][k] came from: 0 mismatch, 1 I, 2 D (the first of M[s-x][k] + 1, I[s][k], D[s][k], in this order, that equals
 *             their max), 3 none (the cell is NULL, or s = 0)
 *   bit 2     I[s][k] opened: M[s-o-e][k-1] >= I[s-e][k-1]          bit 3     D[s][k] opened: M[s-o-e][k+1] >= D[s-e][k+1]
 * The length of a match run is not stored: extend() depends on the offset before it alone, so the run is found again from the
 * sequences.  The walk has two passes.  Pass A follows the state machine of the backtrace over the codes alone, from (P, m - n, M) to
 * s = 0 (where k must be 0), and notes one record per edit -- 'M' for a mismatch, 'I', 'D' -- in traceback order, each with a flag:
 * the walk is in state M after it (a mismatch, or a gap's open).  That gives the op count: the records plus n minus the pattern
 * symbols they consume.  Pass B replays the records from (0, 0), last record first: where the flag is set it extends greedily and
 * writes the run, then it writes the edit; after the last record it extends once more and must stand on (n, m) with every op slot
 * written.  It fills the op list from its end downwards, so the list is in traceback order; the records lie at the front of the
 * pair's own op region and are each read before an op can take their place.
 * Workspace of a device pair: a ring of min(max(x, o + e) + 1, P_max + 1) wavefronts of 3 width(P_max) int32 (what pwa_scores_wfa
 * keeps), then cells(k) code bytes, wavefront s at byte offset width(0) + .. + width(s - 1), padded to the next multiple of 4:
 * ring + cells <= bytes <= ring + cells + 3, against 12 cells.  A range's weight is ring + codes + op bytes. */
#define PWA_WFA_NONE INT32_MIN
int pwa_wfa_plan(int match, int mismatch, int gap_open, int gap_extend, const uint64_t *n, const uint64_t *m,
                 const int32_t *min_score /* or NULL */, uint64_t n_pairs, int32_t pen[4] /* x, o, e, g */,
                 uint64_t *p_max /* or NULL */, uint64_t *cells /* or NULL */);
int pwa_scores_wfa(pwa_ctx *ctx, int match, int mismatch, int gap_open, int gap_extend, const uint8_t *seq_bytes,
                   const uint64_t *seq_off, uint32_t n_seq, const uint32_t *pair_a, const uint32_t *pair_b, uint64_t n_pairs,
                   const int32_t *min_score /* or NULL */, int32_t *score_out, uint32_t *penalty_out /* or NULL */);
int pwa_align_wfa_batch(pwa_ctx *ctx, int match, int mismatch, int gap_open, int gap_extend, const uint8_t *seq_bytes,
                        const uint64_t *seq_off, uint32_t n_seq, const uint32_t *pair_a, const uint32_t *pair_b, uint64_t n_pairs,
                        int32_t *score_out, uint8_t *ops, const uint64_t *ops_off, uint64_t *n_ops,
                        const int32_t *min_score /* or NULL */);
int pwa_align_wfa_batch_cigar(pwa_ctx *ctx, int match, int mismatch, int gap_open, int gap_extend, const uint8_t *seq_bytes,
                              const uint64_t *seq_off, uint32_t n_seq, const uint32_t *pair_a, const uint32_t *pair_b,
                              uint64_t n_pairs, int32_t *score_out,
                              char *cigar, uint64_t cigar_cap, uint64_t *cigar_off /* n_pairs + 1 */,
                              char *mdz, uint64_t mdz_cap, uint64_t *mdz_off /* n_pairs + 1 */,
                              uint64_t needed[2] /* or NULL */, const int32_t *min_score /* or NULL */);
int pwa_align_wfa_codes_batch(pwa_ctx *ctx, int match, int mismatch, int gap_open, int gap_extend, const uint8_t *seq_bytes,
                              const uint64_t *seq_off, uint32_t n_seq, const uint32_t *pair_a, const uint32_t *pair_b,
                              uint64_t n_pairs, int32_t *score_out, uint8_t *ops, const uint64_t *ops_off, uint64_t *n_ops,
                              const int32_t *min_score /* or NULL */);
int pwa_align_wfa_codes_batch_cigar(pwa_ctx *ctx, int match, int mismatch, int gap_open, int gap_extend,
                                    const uint8_t *seq_bytes, const uint64_t *seq_off, uint32_t n_seq, const uint32_t *pair_a,
                                    const uint32_t *pair_b, uint64_t n_pairs, int32_t *score_out,
                                    char *cigar, uint64_t cigar_cap, uint64_t *cigar_off /* n_pairs + 1 */,
                                    char *mdz, uint64_t mdz_cap, uint64_t *mdz_off /* n_pairs + 1 */,
                                    uint64_t needed[2] /* or NULL */, const int32_t *min_score /* or NULL */);
int pwa_wfa_last_stats(const pwa_ctx *ctx, float *sweep_ms, float *walk_ms, uint64_t *cells, uint64_t *workspace_bytes);

/* ---- Semi-global wavefront alignments: the WHOLE pattern against any substring of the text, both text ends free, exact, for patterns
 * of any length and without a band.  What PWA_MODE_SG of the gotoh block computes (score, end cell = the first
 * maximum of row n), by the sweep of the block above; scoring, sequences, pairs, bytes and the range rule are that block's.
 * The global conversion does not carry over: its 2x scale rests on n + m being fixed, and here the consumed text length varies.
 * Penalties are counted per PATTERN symbol instead -- every one is consumed, so n = matches + mismatches + 'D':
 *   x0 = match - mismatch   o0 = -gap_open   eI0 = -gap_extend   eD0 = match - gap_extend
 *   g = gcd(x0, o0, eI0, eD0) (gcd with 0 is the other value)   x, o, eI, eD = the four divided by g     score = match n - g P
 * P is the sum of the reduced penalties of the alignment's mismatches and gaps: a run of L 'I' (text symbol against a gap) costs
 * o + L eI, a run of L 'D' (pattern symbol against a gap) o + L eD, a skipped text prefix or suffix nothing; minimal P is maximal
 * semi-global score.  PWA_E_INVALID unless gap_open <= 0, gap_extend < 0, match > mismatch and match - gap_extend > 0 (gap_extend = 0
 * would give eI = 0, a dependency between diagonals of one wavefront).
 * Wavefronts, on the definitions above (offset = text index j, k = j - i, the trim on every term):
 *   I[s][k] = max(M[s-o-eI][k-1], I[s-eI][k-1]) + 1
 *   D[s][k] = max(M[s-o-eD][k+1], D[s-eD][k+1])
 *   M[s][k] = extend(max(M[s-x][k] + 1, I[s][k], D[s][k]))
 *   M[0][k] = extend(k) for every k = 0 .. m: a start at cell (0, k); I[0] and D[0] are NULL
 * A score is empty when its five source wavefronts (s - x, s - o - eI, s - eI, s - o - eD, s - eD) are all empty or below 0.
 * Wavefront s spans the diagonals [max(-n, -khD(s)), m], khD(s) = 0 for s < o + eD, else (s - o) div eD; width(s) = m + 1 +
 * min(n, khD(s)), and cells(k) = the sum of width(s) over s = 0 .. P_max as above.
 * End: the sweep ends at the first s at which some diagonal holds an offset with j - k = n; that s is P, and the end cell is
 * (n, n + k_end) with k_end the LOWEST such diagonal -- the first maximum of row n, so end cells equal the DP calls' exactly.  Op
 * lists need not: between ties the path is chosen by the wavefront rules.
 * Backtrace: from state M at (P, k_end, n + k_end) with the rules above (ties mismatch >= I >= D, a tie opens); I reads s - o - eI and
 * s - eI at k - 1, D reads s - o - eD and s - eD at k + 1.  At s = 0 it stands on a diagonal 0 <= k <= m, emits j - k 'M' and stops:
 * the start cell is (0, k).
 * Bound: P_worst = o + n eD for n > 0 (all 'D'), else 0; for m >= n the smaller of that and n x (all mismatches).
 * P_max = min(P_worst, floor((match n - min_score) / g)).  NOT FOUND on the host: P_max < 0, or n > m and P_max < o + (n - m) eD; on
 * the device: the sweep reaches P_max without ending.  A pair not found gets PWA_WFA_NONE, penalty 0xffffffff, n_ops = 0, empty
 * strings, and end and start cells (0, 0).  Empty sides as PWA_MODE_SG: n = 0 scores 0 with end = start = (0, 0) and no ops; m = 0
 * gives n 'D'.
 *   pwa_wfa_sg_plan          pwa_wfa_plan for this form: pen = x, o, eI, eD, g.
 *   pwa_scores_wfa_sg        score_out[k], penalty_out[k] = P and end_j_out[k] = the end cell's text index (0 for a pair not found);
 *                            the last two may be NULL.  Workspace: a ring of min(max(x, o + eI, o + eD) + 1, P_max + 1) wavefronts of
 *                            3 width(P_max) int32 per pair.
 *   pwa_align_wfa_sg_batch   op lists with pwa_align_wfa_codes_batch's op regions (n + m bytes of room per pair), and per pair the end
 *                            cell (i, j) in end_cells[2k], [2k + 1] and the start cell in start_cells (either may be NULL).
 *   pwa_align_wfa_sg_batch_cigar  the same alignments as CIGAR and MD:Z with pwa_align_wfa_codes_batch_cigar's buffers and
 *                            PWA_E_CAPACITY / needed protocol; the strings equal pwa_format_alignment of the op list with the returned
 *                            end cell byte for byte.
 * The alignment calls exist in the codes form only: the ring above, then cells(k) code bytes with the same bit layout, written by
 * the same sweep; pass A starts at (P, k_end), accepts any 0 <= k <= m at s = 0 and notes it as the start; pass B replays from
 * (0, k_start) and must end on (n, n + k_end) with every op slot written.  Validation, its order, the ranges under PWA_RANGE_BYTES
 * (weight = ring + codes + op bytes) are those of pwa_align_wfa_codes_batch(_cigar); pwa_wfa_last_stats reports these calls too. */
int pwa_wfa_sg_plan(int match, int mismatch, int gap_open, int gap_extend, const uint64_t *n, const uint64_t *m,
                    const int32_t *min_score /* or NULL */, uint64_t n_pairs, int32_t pen[5] /* x, o, eI, eD, g */,
                    uint64_t *p_max /* or NULL */, uint64_t *cells /* or NULL */);
int pwa_scores_wfa_sg(pwa_ctx *ctx, int match, int mismatch, int gap_open, int gap_extend, const uint8_t *seq_bytes,
                      const uint64_t *seq_off, uint32_t n_seq, const uint32_t *pair_a, const uint32_t *pair_b, uint64_t n_pairs,
                      const int32_t *min_score /* or NULL */, int32_t *score_out, uint32_t *penalty_out /* or NULL */,
                      uint64_t *end_j_out /* or NULL */);
int pwa_align_wfa_sg_batch(pwa_ctx *ctx, int match, int mismatch, int gap_open, int gap_extend, const uint8_t *seq_bytes,
                           const uint64_t *seq_off, uint32_t n_seq, const uint32_t *pair_a, const uint32_t *pair_b,
                           uint64_t n_pairs, int32_t *score_out, uint8_t *ops, const uint64_t *ops_off, uint64_t *n_ops,
                           uint64_t *end_cells /* 2 * n_pairs or NULL */, uint64_t *start_cells /* 2 * n_pairs or NULL */,
                           const int32_t *min_score /* or NULL */);
int pwa_align_wfa_sg_batch_cigar(pwa_ctx *ctx, int match, int mismatch, int gap_open, int gap_extend, const uint8_t *seq_bytes,
                                 const uint64_t *seq_off, uint32_t n_seq, const uint32_t *pair_a, const uint32_t *pair_b,
                                 uint64_t n_pairs, int32_t *score_out,
                                 char *cigar, uint64_t cigar_cap, uint64_t *cigar_off /* n_pairs + 1 */,
                                 char *mdz, uint64_t mdz_cap, uint64_t *mdz_off /* n_pairs + 1 */,
                                 uint64_t *end_cells /* 2 * n_pairs or NULL */, uint64_t *start_cells /* 2 * n_pairs or NULL */,
                                 uint64_t needed[2] /* or NULL */, const int32_t *min_score /* or NULL */);

/* ---- Collinear chaining of anchors: the DP between seeding and extension of a read mapper
 *
 * Anchors.  An anchor of read r is (t, q, len) with len >= 1 and claims read[q .. q + len) == text[t .. t + len); the call never looks
 * at sequences, an anchor may come from anywhere.  Read r's anchors are entries anc_off[r] .. anc_off[r + 1]) of the three parallel
 * arrays anc_t, anc_q, anc_len.  x = t + len and y = q + len are the exclusive ends.  Within a read the anchors are in non-decreasing
 * lexicographic order of (x, y); equal anchors are legal.  Indices below are local to the read.
 * Parameters: lookback H 1 .. 512, max_dist 1 .. 2^30, bandwidth 0 .. 2^20, gap_scale 0 .. 1024.
 * Recurrence.  For anchor i, over the predecessors j in [max(0, i - H), i) -- every one of them, no skip heuristic:
 *   dx = x_i - x_j, dy = y_i - y_j, dd = |dx - dy|
 *   j is admissible iff 0 < dx <= max_dist, 0 < dy <= max_dist and dd <= bandwidth
 *   cand(j) = f(j) + min(len_i, dx, dy) - beta(dd)
 *   beta(0) = 0; for dd >= 1, beta(dd) = ((gap_scale * dd) >> 8) + (floor(log2 dd) >> 1)
 *   f(i) = max(len_i, max_j cand(j))
 *   pred(i) = -1 unless some admissible cand(j) > len_i strictly; otherwise the largest j among the admissible j of maximal cand.
 * All arithmetic is int32; the limits below keep every intermediate inside it.
 * Result per read.  The chain's last anchor e is the smallest index with maximal f; the chain is e, pred(e), ... down to b with
 * pred(b) = -1.  score_out[r] = f(e), count_out[r] = the number of chain anchors, last_out[r] = e, span_out[4 r ..] = (q_b, y_e, t_b,
 * x_e), diag_out[2 r ..] = (min, max) of t - q over the chain's anchors: the j - i diagonals that band_lo / band_hi of the banded
 * calls use.  A read without anchors gives score 0, count 0, last 0xFFFFFFFF and zeros elsewhere, and never reaches the device.
 * f_out and pred_out (one int32 per anchor, local indices, each may be NULL) return the whole DP: a caller derives secondary chains
 * from them.
 * Validation runs before any device work.  First a null ctx or null required pointer and a parameter outside its range, PWA_E_INVALID;
 * then in read order, the first offending read decides, and within a read: anc_off not non-decreasing PWA_E_INVALID; more than 2^24
 * anchors PWA_E_CAPACITY; then anchor by anchor a len of 0 PWA_E_INVALID, t + len or q + len >= 2^31 PWA_E_CAPACITY, the order
 * violated PWA_E_INVALID; then a sum of len >= 2^30 PWA_E_CAPACITY.  n_reads = 0 is PWA_OK.
 * Ranges.  Consecutive reads run together as long as their device bytes -- 20 bytes per anchor (t, q, len, f, pred) plus a 40-byte
 * result record per read -- fit PWA_RANGE_BYTES, else the library's budget; one read alone may exceed it.  A range whose reads are
 * all empty launches nothing and is not counted.
 *   pwa_chain_plan        host only, no context, no GPU: the validation code of the same inputs, *bad_read = the first offending read
 *                         (0xFFFFFFFF: none, or a pointer or parameter was at fault), *n_ranges = the ranges the call would run
 *                         under budget_bytes (0: no limit).  bad_read and n_ranges may be NULL.
 *   pwa_chain_last_stats  of the last pwa_chain_anchors on ctx: device ms of the chain kernel (events, summed over the ranges), the
 *                         anchors it chained, the ranges it ran.  Any pointer may be NULL; a call that fails validation leaves them. */
int pwa_chain_plan(const uint32_t *anc_t, const uint32_t *anc_q, const uint32_t *anc_len, const uint64_t *anc_off /* n_reads + 1 */,
                   uint32_t n_reads, uint32_t lookback, uint32_t max_dist, uint32_t bandwidth, uint32_t gap_scale,
                   uint64_t budget_bytes, uint32_t *bad_read /* or NULL */, uint64_t *n_ranges /* or NULL */);
int pwa_chain_anchors(pwa_ctx *ctx, const uint32_t *anc_t, const uint32_t *anc_q, const uint32_t *anc_len,
                      const uint64_t *anc_off /* n_reads + 1 */, uint32_t n_reads, uint32_t lookback, uint32_t max_dist,
                      uint32_t bandwidth, uint32_t gap_scale, int32_t *score_out, uint32_t *count_out, uint32_t *last_out,
                      uint32_t *span_out /* 4 * n_reads */, int32_t *diag_out /* 2 * n_reads */, int32_t *f_out /* or NULL */,
                      int32_t *pred_out /* or NULL */);
int pwa_chain_last_stats(const pwa_ctx *ctx, float *chain_ms, uint64_t *anchors, uint64_t *ranges);

/* ---- Top-N chains of a read, mapping quality: the alternative placements behind the best chain
 *
 * Anchors, their order, lookback / max_dist / bandwidth / gap_scale, f and pred are those of pwa_chain_anchors above, unchanged.
 * New parameters: max_chains N 1 .. 16, min_score 1 .. 2^30, min_count 1 .. 2^24, flags 0 or PWA_CHAIN_ROOTED.
 * Selection.  Per read, every anchor carries a mark, initially "free".  Candidates are the anchors in order of descending f, the
 * smaller index first among equal f.  For each candidate e, in that order:
 *   1. stop the read when N chains are kept, or when f(e) < min_score (no later walk can score min_score);
 *   2. skip e if it is marked;
 *   3. otherwise this is a round: walk cur = e, pred(cur), ...; every anchor visited is part of the walk.  The walk ends at the
 *      anchor b whose pred is -1 (base = 0, branch = -1), or at the anchor b whose pred p is already marked (base = f(p), branch = p);
 *   4. score = f(e) - base, count = the number of anchors of the walk;
 *   5. the walk is kept iff score >= min_score and count >= min_count and (PWA_CHAIN_ROOTED is not set or branch = -1);
 *   6. its anchors are marked in either case: with the kept chain's index c = 0, 1, ... when kept, with "dropped" otherwise.
 *      A dropped walk still claims its anchors: a later walk that runs into one of them stops there.
 * A kept chain's record: score, count, last = e, (q_b, y_e, t_b, x_e), (min, max) of t - q over the walk's anchors, branch.  With
 * min_score = 1 and min_count = 1, chain 0 is pwa_chain_anchors' result field by field, with branch = -1.
 * Outputs.  n_chains_out[r] = the chains kept for read r; read r's chain c is slot r * max_chains + c of score_out, count_out,
 * last_out, branch_out, and, laid out as in pwa_chain_anchors by slot, of span_out (4 per slot) and diag_out (2 per slot).  Unused
 * slots hold score 0, count 0, last 0xFFFFFFFF, branch -1 and zeros elsewhere.  mapq_out (one per read), f_out, pred_out and
 * chain_id_out (one per anchor: c for an anchor of kept chain c, else -1) may each be NULL.  A read without anchors is answered on
 * the host; n_reads = 0 is PWA_OK.
 * Mapping quality, integers only: pwa_mapq(s1, s2, c1) = min(60, (60 * (s1 - s2) * min(c1, 10)) div (10 * s1)) in 64-bit arithmetic,
 * 0 when s1 <= 0, s2 clamped to [0, s1].  mapq_out[r] = pwa_mapq(score of chain 0, the best score among the chains 1 .. with
 * branch = -1 or 0 if there is none, count of chain 0), and 0 for a read without a kept chain.
 * Validation is pwa_chain_plan's, in its order; the four new parameters are checked in its "parameter outside its range" step.
 * Ranges.  As above, with this call's device bytes: 48 per anchor (t, q, len, f, pred, the mark, two sort keys of 8 and two sort
 * values of 4) plus 40 * max_chains + 16 per read (its chain slots and a head of 4 words).
 * The DP runs on the device with pwa_chain_anchors' kernel and stays there; the candidates are ordered by one stable radix sort per
 * range and selected by one wave per read; nothing per anchor is copied back unless f_out, pred_out or chain_id_out asks for it.
 *   pwa_chain_top_plan        host only: the validation code, *bad_read and *n_ranges as pwa_chain_plan gives them.
 *   pwa_chain_top_last_stats  of the last pwa_chain_top on ctx: device ms of the chain kernel and of the selection (keys, sort and
 *                             walks), the anchors, the rounds (step 3) summed over the reads, the ranges.  Any pointer may be NULL.
 *                             pwa_chain_last_stats keeps reporting pwa_chain_anchors only.
 *   pwa_mapq                  host only; returns the value. */
#define PWA_CHAIN_ROOTED 1u /* flags: keep only walks that end at an anchor without a predecessor */
int pwa_chain_top_plan(const uint32_t *anc_t, const uint32_t *anc_q, const uint32_t *anc_len, const uint64_t *anc_off /* n_reads + 1 */,
                       uint32_t n_reads, uint32_t lookback, uint32_t max_dist, uint32_t bandwidth, uint32_t gap_scale,
                       uint32_t max_chains, uint32_t min_score, uint32_t min_count, uint32_t flags, uint64_t budget_bytes,
                       uint32_t *bad_read /* or NULL */, uint64_t *n_ranges /* or NULL */);
int pwa_chain_top(pwa_ctx *ctx, const uint32_t *anc_t, const uint32_t *anc_q, const uint32_t *anc_len,
                  const uint64_t *anc_off /* n_reads + 1 */, uint32_t n_reads, uint32_t lookback, uint32_t max_dist, uint32_t bandwidth,
                  uint32_t gap_scale, uint32_t max_chains, uint32_t min_score, uint32_t min_count, uint32_t flags,
                  uint32_t *n_chains_out /* n_reads */, int32_t *score_out /* n_reads * max_chains, as count, last, branch */,
                  uint32_t *count_out, uint32_t *last_out, uint32_t *span_out /* 4 * n_reads * max_chains */,
                  int32_t *diag_out /* 2 * n_reads * max_chains */, int32_t *branch_out, uint32_t *mapq_out /* n_reads or NULL */,
                  int32_t *f_out /* or NULL */, int32_t *pred_out /* or NULL */, int32_t *chain_id_out /* or NULL */);
int pwa_chain_top_last_stats(const pwa_ctx *ctx, float *chain_ms, float *top_ms, uint64_t *anchors, uint64_t *rounds, uint64_t *ranges);
int pwa_mapq(int32_t s1, int32_t s2, uint32_t c1);

/*
 * Host-side post-processing of one alignment (no GPU work): everything hw2.cpp derives from
 * the walk -- the gapped strings (hw2.cpp:164-184 / 240-259), prepareCigarString (59-78),
 * prepareMDZString (80-116) and overlapLongestExactMatch (267-278) -- so that the five fields
 * of the reference's AlignmentResult (hw2.cpp:17-23) can be rebuilt from pwa_align's output.
 *   ops / n_ops / end_cell : as returned by pwa_align (ops in traceback order)
 *   aligned_pattern, aligned_reference : n_ops + 1 bytes each (NUL-terminated)
 *   cigar : pwa_cigar_bound(n_ops) bytes;  mdz : pwa_mdz_bound(n_ops) bytes
 * Note the reference's conventions are kept verbatim: 'D' = pattern char against '-',
 * 'I' = '-' against text char, MD:Z mismatches print the REFERENCE character and deletions
 * print the PATTERN characters.
 */
/* overlapLongestExactMatch (hw2.cpp:267-278) straight from the op list, without building the strings:
 * what the -g selection loop (hw2.cpp:342-350) needs for every pair. */
int pwa_alignment_overlap(const uint8_t *pattern, uint64_t n, const uint8_t *text, uint64_t m, const uint8_t *ops,
                          uint64_t n_ops, const uint64_t end_cell[2], int32_t *overlap);
uint64_t pwa_cigar_bound(uint64_t n_ops);
uint64_t pwa_mdz_bound(uint64_t n_ops);
int pwa_format_alignment(const uint8_t *pattern, uint64_t n, const uint8_t *text, uint64_t m, const uint8_t *ops,
                         uint64_t n_ops, const uint64_t end_cell[2], char *aligned_pattern, char *aligned_reference,
                         char *cigar, char *mdz, int32_t *overlap);

#ifdef __cplusplus
}
#endif
#endif /* PWALIGN_H */
