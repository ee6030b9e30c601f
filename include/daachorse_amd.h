/*
 * daachorse_amd.h — C ABI of the MI355X-native daachorse scan path.
 *
 * This is the drop-in boundary for ONE path of the daachorse crate (v4.0.0): the bytewise
 * double-array Aho-Corasick scan (find_overlapping_iter / find_iter / leftmost_find_iter and
 * friends over DoubleArrayAhoCorasick<u32>).  The reference has no FFI of its own; every entry
 * point below names the Rust item (file:line under the reference tree) whose work it takes
 * over, and INTEGRATION.md shows the `extern "C"` block a crate maintainer would add.
 *
 * Conventions
 *   - plain C, no exceptions cross the boundary, no torch/HIP types in signatures
 *     (`stream` is a hipStream_t passed as void*; NULL = the default stream);
 *   - every call returns a daac_status; daac_last_error() gives a thread-local message;
 *   - automata are immutable after creation: any number of host threads may scan the same
 *     handle concurrently (each call brings its own stream);
 *   - V = u32 only (pattern values are 32-bit), positions are 64-bit.
 *   - there is NO CPU scan backend in this library: a scan without a usable gfx950 device
 *     returns DAAC_ERR_DEVICE.
 */
#ifndef DAACHORSE_AMD_H
#define DAACHORSE_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Version of this header's ABI: struct layouts and the meaning of enum values.  daac_abi_version() returns the version the
 * loaded library was built with; a binding checks it once (the ctypes and C++ mirrors here do).
 *   3 (round 3): daac_info starts with struct_size and carries the per-request engine plan; DAAC_ENGINE_PFX; daac_match16 /
 *                daac_scan_device16.
 *   4 (round 4): daac_iter_next_batch; the lazy iterator runs its windows ahead of the consumer on a worker thread; DAAC_ENGINE_JUMP /
 *                DAAC_KERNEL_JUMP are gone (the experiment is in the history: commit c51e1c3 and before, tools/experiments/jump).
 *   5 (round 5): daac_scan_count_multi (one haystack sharded across the devices of a node); daac_pma_set_option (options per handle);
 *                daac_pma_trim; options gram4_arith, gram_tail.
 *   6 (round 6): daac_stream_feed_compact; daac_scan_count_multi runs its shards on one persistent worker thread + stream per device;
 *                daac_pma_set_option answers 6 for an option that is read at upload once the handle has tables on a device;
 *                gram_version 3 is an alias of 4; the options emit_stagger, emit_v3_lds and the four names of engines that left the
 *                library (restart_tier, emit_tiles, emit_rec_cap, emit_version) are gone.
 *   (6, additions that change no layout and no enum value: daac_scan_count_batch / daac_scan_batch_device16 — many documents in one call,
 *      per-document results — and the options batch_piece, batch_lane_max.  A binding that needs them looks the two symbols up.)
 *   (6, likewise: daac_pma_outputs / daac_scan_histogram — per-pattern match counts of an overlapping scan — and the option
 *      hist_lds_bins.)
 *   (6, likewise: daac_slot_count / daac_scan_histogram_batch — per-document pattern counts of a batch, as a CSR matrix — and the
 *      options batch_hist_wave_max, batch_hist_sort_max.)
 *   (6, likewise: daac_replace_all / daac_replace_all_batch — the text with every match of find_iter / leftmost_find_iter replaced,
 *      spliced on the device.)
 *   (6, likewise: daac_tokenize / daac_tokenize_batch and the enum daac_gap — the matches' values and the gaps between them as one token
 *      id list, on the device.)
 *   (6, likewise: daac_tokenize_unigram / daac_tokenize_unigram_batch — the segmentation whose pieces' scores sum highest, a Viterbi pass
 *      over the tuple list of an overlapping scan, on the device.)
 *   (6, likewise: daac_tokenize_bpe / daac_tokenize_bpe_batch — the token ids of byte-pair merging in rank order over the same tuple
 *      list, on the device — and the option bpe_doc_max.)
 *   (6, likewise: daac_splitter_create / daac_split_batch / daac_split, daac_offsets_compose and daac_spans_rebase — the pre-tokenizer
 *      split of a batch into words, on the device.)
 *   (6, likewise: daac_tokenize_wordpiece / daac_tokenize_wordpiece_batch — BERT's WordPiece over the same tuple list, on the device —
 *      with the split rule DAAC_SPLIT_BERT and daac_split_words_space in front of it.)
 *   (6, likewise: daac_normalizer_create / daac_normalize_batch / daac_normalize and daac_spans_to_source — a per-code-point rewrite of
 *      a batch, BERT's normalizer among them, on the device.)
 *   (6, likewise: daac_cut_batch / daac_tokens_splice — a batch cut into segments around the special tokens written into its text,
 *      and a tokenizer's result over the segments put back together per document, on the device.)
 *   (6, likewise: daac_tokens_pack and daac_pack_params — a token result wrapped in a template, truncated and padded into the planes a
 *      model reads, on the device.)
 *   (6, likewise: daac_decoder_create / daac_decoder_free / daac_tokens_decode — token ids back to text, from a CSR token result or a
 *      dense plane of ids, on the device.) */
#define DAAC_ABI_VERSION 6
uint32_t daac_abi_version(void);

/* src/errors.rs:10-22 (first four), plus the panics / extras of this boundary */
typedef enum {
    DAAC_OK = 0,
    DAAC_ERR_INVALID_ARGUMENT = 1,  /* DaachorseError::InvalidArgument   */
    DAAC_ERR_AUTOMATON_SCALE = 2,   /* DaachorseError::AutomatonScale    */
    DAAC_ERR_INVALID_CONVERSION = 3,/* DaachorseError::InvalidConversion */
    DAAC_ERR_INVALID_AUTOMATON = 4, /* DaachorseError::InvalidAutomaton  */
    DAAC_ERR_MATCH_KIND = 5,        /* the reference PANICS here: bytewise.rs:194-197, 299-302, 551-554 */
    DAAC_ERR_UNSUPPORTED = 6,       /* an engine that cannot serve the request; or the one input on which the reference itself never terminates (leftmost kind, "" in the set, haystack ends inside a longer pattern: SURVEY §8a note D) */
    DAAC_ERR_DEVICE = 7             /* HIP error / no gfx950 device */
} daac_status;

/* src/lib.rs:324-346 (repr(u8)) */
typedef enum { DAAC_STANDARD = 0, DAAC_LEFTMOST_LONGEST = 1, DAAC_LEFTMOST_FIRST = 2 } daac_match_kind;

/* Which iterator of src/bytewise/iter.rs a scan reproduces */
typedef enum {
    DAAC_FIND_OVERLAPPING = 0,           /* FindOverlappingIterator          iter.rs:117-177 */
    DAAC_FIND = 1,                       /* FindIterator                     iter.rs:44-114  */
    DAAC_LEFTMOST_FIND = 2,              /* LeftmostFindIterator             iter.rs:247-341 */
    DAAC_FIND_OVERLAPPING_NO_SUFFIX = 3  /* FindOverlappingNoSuffixIterator  iter.rs:180-244 */
} daac_scan_mode;

/* Which device engine to use.  AUTO picks GRAM for daac_scan_count[_range](FIND_OVERLAPPING) and TIERED
 * for everything else when the automaton qualifies, DARRAY otherwise. */
typedef enum {
    DAAC_ENGINE_AUTO = 0,
    DAAC_ENGINE_TIERED = 1, /* re-packed bitmap-rank trie, top levels dense in LDS */
    DAAC_ENGINE_DARRAY = 2, /* the reference's own double array, hot/cold split   */
    DAAC_ENGINE_GRAM = 3,   /* k-gram context tables in LDS, no state chain: count / checksum, and tuples of FIND_OVERLAPPING */
    DAAC_ENGINE_PFX = 4     /* hashed prefix filter in LDS + goto-only walks from the start of an occurrence: `.count()`, count + checksum
                             * and (round 4, dictionaries without duplicate patterns) the tuples of FIND_OVERLAPPING for dictionaries over
                             * any byte alphabet (what AUTO takes where GRAM's byte classes run out) */
} daac_engine;

/* Match<u32> (src/lib.rs:286-320): start() = end - length, end(), value() */
typedef struct {
    uint64_t start;
    uint64_t end;
    uint32_t value;
    uint32_t _pad;
} daac_match;

/* The same match as the crate keeps it (Match<u32>, src/lib.rs:287-291: length, end, value; start() = end - length): 16 bytes, what
 * daac_scan_device16 leaves in device memory — one 16-byte store per tuple and a third less write traffic than daac_match. */
typedef struct {
    uint64_t end;
    uint32_t length;
    uint32_t value;
} daac_match16;

/* What a request is served by (daac_info.plan_*): the engine AUTO resolves to, the kernel family behind it, and — where that is not
 * the fastest family — why.  The families differ by an order of magnitude: this is the performance contract of a handle,
 * visible before the first scan. */
typedef enum {
    DAAC_REQ_OVERLAPPING_COUNT = 0,     /* find_overlapping_iter(h).count()        daac_scan_count_only_range           */
    DAAC_REQ_OVERLAPPING_CHECKSUM = 1,  /* count + checksum of that stream         daac_scan_count / _range             */
    DAAC_REQ_OVERLAPPING_TUPLES = 2,    /* the tuples                              daac_scan / daac_scan_device[16] / daac_iter_* */
    DAAC_REQ_FIND = 3,                  /* find_iter, any form                                                            */
    DAAC_REQ_LEFTMOST_FIND = 4,         /* leftmost_find_iter, any form                                                   */
    DAAC_REQ_NO_SUFFIX = 5,             /* find_overlapping_no_suffix_iter, any form                                      */
    DAAC_REQ_N = 6
} daac_request;
typedef enum {
    DAAC_KERNEL_NONE = 0,        /* the request does not apply to this automaton's MatchKind (the crate panics) */
    DAAC_KERNEL_GRAM_COUNT = 1,  /* gram4_kernels.hip: one LDS lookup per byte, lane-local hit masks           (cfg3: 1.4 TB/s) */
    DAAC_KERNEL_GRAM_EXACT = 2,  /* gram_kernels.hip / gram2_kernels.hip with the checksum, or gram2_kernels.hip counting alone where gram4
                                  * does not serve (gram_version = 2, no gram4 launch shape fits)              (cfg3: 1.0 TB/s) */
    DAAC_KERNEL_GRAM_WIDE = 3,   /* gram2w_kernels.hip: 31 .. 62 byte classes                                   (1.0 / 0.9 TB/s) */
    DAAC_KERNEL_GRAM_EMIT = 4,   /* emit3_kernels.hip (gram2_emit_kernels.hip behind it): tuples in reference order (cfg3: 0.22 TB/s of haystack) */
    DAAC_KERNEL_PFX = 5,         /* pfx_kernels.hip: any byte alphabet; `.count()` 0.6 - 1.3 TB/s on sparse dictionaries, 0.05 - 0.1 on the
                                  * wide look-alikes; tuples through pfx_emit_kernel + EXPAND: 0.02 - 0.36 TB/s of haystack */
    DAAC_KERNEL_SEGMENT = 6,     /* scan_kernels.hip: one lane per segment, TIERED or DARRAY tables             (0.03 - 0.4 TB/s) */
    DAAC_KERNEL_MICRO = 7,       /* chain_scan.hpp overlap_count_body: micro-step walker over the double array  (0.08 - 0.4 TB/s) */
    DAAC_KERNEL_CHAIN = 8,       /* chain_scan.hpp: speculate / reconcile / emit for the restart iterators      (0.1 - 0.3 TB/s) */
    DAAC_KERNEL_SELECT = 9       /* find3_kernels.hip / left3_kernels.hip: the restart iterators' count (+ checksum) as a selection over the tuple
                                    emitter's detection, no state chain (cfg3, random text: 0.36 / 0.31 TB/s); text made of dictionary words goes
                                    back to DAAC_KERNEL_CHAIN and the plan then says so */
} daac_kernel_family;
typedef enum {
    DAAC_WHY_FASTEST = 0,        /* nothing faster exists for this request */
    DAAC_WHY_NOT_UPLOADED = 1,   /* daac_pma_upload has not run: the plan is not known yet */
    DAAC_WHY_ALPHABET = 2,       /* more distinct pattern bytes than the byte-class tables take (30 / 62) */
    DAAC_WHY_LDS = 3,            /* the tables do not fit the 160 KB of LDS */
    DAAC_WHY_EMPTY_PATTERN = 4,  /* "" is a pattern: every position matches */
    DAAC_WHY_DUPLICATES = 5,     /* duplicate patterns beyond what the tables encode (more than 3 ending after one context; for tuples: among patterns of at most K bytes, or more than 16 copies of one pattern) */
    DAAC_WHY_CHAIN = 6,          /* the iterator is a chain through its own matches: no position-parallel form */
    DAAC_WHY_CHARWISE = 7,       /* a charwise automaton: scanned over its own double array */
    DAAC_WHY_TRIE_SHAPE = 8      /* not a tree-shaped trie / other table limits */
} daac_plan_reason;

typedef struct {
    uint32_t struct_size;     /* IN: sizeof(daac_info) as the caller was compiled (0 = the round-2 layout is NOT assumed: the call fails);
                               * the library fills at most this many bytes */
    uint8_t match_kind;       /* DoubleArrayAhoCorasick::match_kind()  bytewise.rs:735-737 */
    uint32_t num_states;      /* ::num_states()                        bytewise.rs:785-787 */
    uint64_t states_len;      /* double-array elements (multiple of 256) */
    uint64_t outputs_len;
    uint64_t heap_bytes;      /* ::heap_bytes()                        bytewise.rs:764-770 */
    uint32_t max_pattern_len; /* max Output::length — the halo is this minus one */
    /* device-side re-pack (valid after upload) */
    uint32_t num_classes;     /* byte classes incl. class 0 = "byte occurs in no pattern" */
    uint32_t tier_dense_states;  /* states with a dense, fail-resolved LDS row */
    uint32_t tier_lds_states;    /* + states whose child bitmap lives in LDS */
    uint32_t tier_lds_bytes;     /* LDS bytes of the automaton tables per workgroup: at most the lds_budget they were laid out under */
    uint8_t tiered_available;    /* 0 if only the DARRAY engine can run this automaton */
    uint8_t gram_available;      /* the GRAM count engine can run this automaton */
    uint32_t gram_k;             /* context length K of the GRAM tables */
    uint32_t gram_lds_bytes;
    uint8_t charwise;            /* 1: a CharwiseDoubleArrayAhoCorasick (src/charwise.rs), 0: bytewise */
    uint32_t alphabet_size;      /* charwise: number of distinct code points in the patterns (mapper.rs:10-13) */
    uint8_t gram2_available;     /* the GRAM engine's second table set (one LDS lookup per position) serves this automaton */
    uint8_t gram2_exact;         /* ... also with the checksum (CID/H fit next to M) */
    uint32_t gram2_k;
    uint32_t gram2_lds_count;    /* LDS bytes per workgroup, count only / with checksum */
    uint32_t gram2_lds_exact;
    uint8_t gram_wide;           /* 31 .. 62 byte classes: the GRAM engine runs on 64-bit words with K = 2 (gram2w.hpp) */
    uint8_t pfx_available;       /* the PFX tables were built (any byte alphabet: `.count()`, count + checksum, tuples) */
    uint32_t pfx_key_bytes;      /* G: bytes of a PFX filter key */
    uint32_t pfx_lds_bytes;
    /* the engine plan, indexed by daac_request; valid after upload, for engine AUTO */
    uint8_t plan_engine[8];      /* daac_engine reported by daac_last_engine() after such a request */
    uint8_t plan_kernel[8];      /* daac_kernel_family */
    uint8_t plan_reason[8];      /* daac_plan_reason: why not the fastest family */
} daac_info;

typedef struct daac_pma daac_pma;         /* an automaton (host copy + per-device re-pack) */
typedef struct daac_matches daac_matches; /* result of an eager scan */
typedef struct daac_iter daac_iter;       /* lazy iterator façade */

const char *daac_last_error(void);
void daac_free(void *p);
/* daac_engine that served this thread's most recent scan (AUTO resolves to GRAM / TIERED / DARRAY per request:
 * e.g. GRAM declines ranges of 32 GiB and more and automata whose tables do not fit LDS). */
int daac_last_engine(void);
/* The kernel family — and, for the `.count()` kernel, the launch shape the options in force gave it ("gram4 ppl=32 dir=0 waves=16 arith=1 filter=1
 * mph=1 regions=23552 claims=11264 tail=auto": regions of the launch, and how many of them its waves claim from the call's counter) — that served the calling thread's last daac_scan_count* call (daac_scan_count_multi: shard 0's, as run by its device's worker).
 * The count + checksum GRAM kernels name the compiled instance that ran and the launch's regions: "gram K=3 short=1 waves=16 dense=0 rank=lds ppl=16
 * region=2048 regions=7 slab=1216" (rank: the rank directory in the LDS or read from the L2), "gram2 K=3 dir=1 dense=0 waves=16 region=.. regions=.."
 * (dir=2: 32-bit directory entries), "gram2w exact=1 region=.. regions=.." (exact=0: `.count()` alone); a call that launches nothing
 * (an empty range) says the family alone.  A materialising overlapping scan that the tuple emitter served says "emit3 raw=0 attempts=1"
 * (raw=1: the PFX form over the raw text; attempts=2: the record list proved too short and the detection was rerun with the exact size).
 * ABI 6; a diagnostic: the text is not a contract. */
const char *daac_last_kernel(void);

/* ---- construction / (de)serialisation ------------------------------------------------------ */

/* DoubleArrayAhoCorasick::deserialize (bytewise.rs:868-964): parses the crate's serialize()
 * blob for V = u32 with the same validation, rebuilds root_table (bytewise.rs:1040-1056).
 * The caller keeps `blob`. */
daac_status daac_bytewise_from_serialized(const uint8_t *blob, size_t len, daac_pma **out, size_t *consumed);

/* Takes the automaton's arrays directly (what a Rust shim has in hand without serialising):
 * `states` = n_states x {base, fail, opos_ch} (State<u32>, bytewise.rs:1131-1137) or, for leftmost
 * kinds, `lstates` = n x {base, opos_ch} + `fails` (bytewise.rs:61-63); `outputs` = n_outputs x
 * {value, length, parent} (lib.rs:213-218).  Same validation as deserialize.  `fails` must hold n_lstates entries;
 * a NULL array with a non-zero count is DAAC_ERR_INVALID_ARGUMENT. */
daac_status daac_bytewise_from_parts(const uint32_t *states, size_t n_states,
                                     const uint32_t *lstates, const uint32_t *fails, size_t n_lstates,
                                     const uint32_t *outputs, size_t n_outputs,
                                     uint8_t match_kind, uint32_t num_states, daac_pma **out);

/* DoubleArrayAhoCorasickBuilder::build / build_with_values (bytewise/builder.rs:152-244) on the
 * host CPU.  Patterns are one blob + n+1 offsets; values == NULL means value = index. */
daac_status daac_bytewise_build(const uint8_t *blob, const uint64_t *offsets, const uint32_t *values,
                                size_t n, uint8_t match_kind, uint32_t num_free_blocks, daac_pma **out);

/* ---- charwise automata (src/charwise.rs) --------------------------------------
 * A charwise handle is a daac_pma like any other: daac_pma_*, daac_scan*, daac_iter_* serve it with
 * the iterators of src/charwise/iter.rs (FindIterator :101-157, FindOverlappingIterator :160-221,
 * FindOverlappingNoSuffixIterator :224-303, LeftmostFindIterator :306-400).  Haystacks are UTF-8
 * (the reference takes AsRef<str>); start/end stay BYTE offsets, as in the reference.  Engines:
 * AUTO or DARRAY (the charwise double array runs as is). */

/* CharwiseDoubleArrayAhoCorasick::deserialize (charwise.rs:896-952), blob format of serialize()
 * (charwise.rs:831-848: states x {base, check, fail, output_pos}, mapper table + alphabet_size,
 * outputs, match_kind, num_states), same validation. */
daac_status daac_charwise_from_serialized(const uint8_t *blob, size_t len, daac_pma **out, size_t *consumed);

/* CharwiseDoubleArrayAhoCorasickBuilder::build / build_with_values (charwise/builder.rs:178-239) on the
 * host CPU; patterns are UTF-8 (one blob + n+1 byte offsets).  Byte-identical arrays. */
daac_status daac_charwise_build(const uint8_t *blob, const uint64_t *offsets, const uint32_t *values,
                                size_t n, uint8_t match_kind, uint32_t num_free_blocks, daac_pma **out);

/* ::serialize (bytewise.rs:801-820 / charwise.rs:831-848); free the buffer with daac_free. */
daac_status daac_pma_serialize(const daac_pma *pma, uint8_t **buf, size_t *len);
/* `info->struct_size` must be set by the caller (see daac_info). */
daac_status daac_pma_info(const daac_pma *pma, daac_info *info);
/* One line of text per request of the plan ("find_overlapping_iter().count(): engine gram, kernel gram4 ..."); returns the
 * number of bytes the full text needs (incl. the terminating 0); writes at most `cap`. */
size_t daac_pma_explain(const daac_pma *pma, char *buf, size_t cap);
void daac_pma_free(daac_pma *pma);

/* Re-packs the automaton for the GPU and copies it to `device` (idempotent).  Scans upload
 * lazily to the current device if this was not called. */
daac_status daac_pma_upload(daac_pma *pma, int device);
/* Releases the scratch a handle keeps between calls beside its tables (the tuple emitter's and the selection kernels' workspace, up to
 * option workspace_keep bytes per device): for processes that hold many handles.  Tables stay; the next scan allocates again. */
daac_status daac_pma_trim(daac_pma *pma);

/* ---- scans ----------------------------------------------------------------------------------- */

/* Eager scan of one haystack; replaces driving the iterator to exhaustion
 * (`pma.find_overlapping_iter(h).collect()` etc.).  `hay` is a host pointer, or a device pointer
 * if hay_is_device != 0.  Matches come back in the reference's order. */
daac_status daac_scan(daac_pma *pma, int mode, int engine, const uint8_t *hay, size_t len,
                      int hay_is_device, void *stream, daac_matches **out);
/* The same with the match list left in DEVICE memory (for consumers that run on the GPU): `*dev_out` receives a device
 * buffer of `*count` daac_match tuples in the reference's order (NULL when there are none), owned by the caller and
 * released with daac_device_free.  For DAAC_FIND_OVERLAPPING on a bytewise Standard automaton whose tables fit (engine
 * AUTO or GRAM) the tuples come from the GRAM emitter: per-tile counts, one exclusive scan, then every tuple is written
 * once, straight to its final place; all other requests run the segment scanners (count, scan, write).  The call returns
 * after the stream has finished.  daac_device_to_host copies (part of) such a list to host memory. */
daac_status daac_scan_device(daac_pma *pma, int mode, int engine, const uint8_t *hay, size_t len,
                             int hay_is_device, void *stream, daac_match **dev_out, uint64_t *count);
/* The same list as 16-byte tuples {end, length, value} (daac_match16).  The GRAM emitter writes them directly; lists from the other
 * engines are repacked on the device. */
daac_status daac_scan_device16(daac_pma *pma, int mode, int engine, const uint8_t *hay, size_t len,
                               int hay_is_device, void *stream, daac_match16 **dev_out, uint64_t *count);
void daac_device_free(void *p);
daac_status daac_device_to_host(void *dst, const void *dev_src, size_t bytes);
size_t daac_matches_count(const daac_matches *m);
const daac_match *daac_matches_data(const daac_matches *m); /* host memory, owned by `m` */
void daac_matches_free(daac_matches *m);

/* Count + order-independent checksum of the match stream without materialising it
 * (`.count()` on the iterator).  checksum = (S1 << 32) | S2 with, over all matches,
 *   h = low32(mix64(value << 32 | length)),  S1 = sum h,  S2 = sum h * low32(end)   (mod 2^32).
 * Asynchronous on `stream` when `result_dev` != NULL: the 3 x u64 {count, S1, S2} are left in
 * device memory there and count/checksum may be NULL; otherwise the call synchronises.
 * Device haystacks are read in whole aligned 16-byte granules: up to 15 bytes before `hay` and after `hay + len`
 * (inside the same 16-byte granules as the first / last byte) are loaded and masked out, never interpreted.  Any
 * hipMalloc'ed buffer satisfies this (allocations are 256-byte granular); a sub-range of a larger allocation always does. */
daac_status daac_scan_count(daac_pma *pma, int mode, int engine, const uint8_t *hay, size_t len,
                            int hay_is_device, void *stream, uint64_t *count, uint64_t *checksum,
                            uint64_t *result_dev);

/* `.count()` alone: the number of matches with end in (begin, len], no checksum.  With `result_dev` the count is left in
 * result_dev[0] (3 x u64 as above; [1] and [2] are not meaningful) and the call is asynchronous.  The GRAM engine serves
 * this with one LDS lookup per haystack byte; every other engine runs its count + checksum scan and drops the checksum. */
daac_status daac_scan_count_only_range(daac_pma *pma, int mode, int engine, const uint8_t *hay, size_t len, size_t begin,
                                       int hay_is_device, void *stream, uint64_t *count, uint64_t *result_dev);

/* One haystack sharded across the GPUs of a node (BASELINE configs[3]: 8 shards, one per MI355X).  Shard k is `len` bytes that begin at
 * haystack position `base`; `hay` points at the `halo` bytes in front of it followed by the shard itself, in the memory of `device`
 * (or in host memory when hay_is_device = 0).  Every shard but the one at position 0 needs halo >= max_pattern_len - 1 (charwise:
 * max_pattern_len, at least 3): a match is counted by the shard its END falls in, wherever it starts; halo <= base.  One
 * persistent worker thread per DEVICE the shards name (ABI 6: created at the handle's first such call, with a stream of its own — a
 * blocking stream: it sees what the caller left on the device's default stream — and the handle's options in scope) queues
 * daac_scan_count[_only]_range for its device's shards back to back (tables are uploaded there on first use) and waits once; the host adds the counts and — when
 * `checksum` is not NULL — the checksum sums with every shard's ends re-based to haystack positions, so the result equals
 * daac_scan_count of the whole haystack.  The find_overlapping modes only (status 6 otherwise: the other two iterators are chains).
 * Several shards may name the same device.  daac_last_engine() / daac_last_kernel() report shard 0's. */
typedef struct {
    int device;           /* HIP device ordinal */
    const uint8_t *hay;   /* `halo` bytes of the haystack in front of the shard, then the shard */
    size_t halo;          /* bytes in front that are there (the shard at position 0: 0) */
    size_t len;           /* bytes of the shard */
    uint64_t base;        /* haystack position of the shard's first byte */
} daac_shard;
daac_status daac_scan_count_multi(daac_pma *pma, int mode, int engine, const daac_shard *shards, size_t n, int hay_is_device,
                                  uint64_t *count, uint64_t *checksum);

/* ---- batches: many independent documents in one call --------------------------------------------------------------------------
 * A batch is one buffer `hay` and n + 1 non-decreasing `offsets`; document i is hay[offsets[i], offsets[i+1]) and the buffer is offsets[n]
 * bytes long.  Every document gets exactly what the single-haystack call returns on that document alone: a match never crosses a document
 * boundary, ends (and the checksum's ends) are relative to the document's first byte, ROOT's "" match is reported at each document's 0,
 * charwise documents are UTF-8 each on their own, and find_iter / leftmost_find_iter start a fresh chain at each document's position 0.
 * Engines AUTO, TIERED and DARRAY (GRAM and PFX: status 6).  Offsets that decrease are status 1 (device offsets: found by a small
 * validation kernel, one read-back before the scans); n = 0 is OK.  A leftmost automaton with "" on a document that ends inside a longer
 * pattern (note D) makes the whole call answer 6, and daac_last_error() names the first such document.  The find_overlapping modes cut
 * the documents into pieces of option batch_piece bytes, one lane a piece; find_iter / leftmost_find_iter give a document of at most
 * batch_lane_max bytes one lane and send longer ones through the single-haystack path (about one call's overhead per such document).
 * Host haystacks are staged in windows of whole documents.  daac_last_kernel() says how the batch was served ("batch pieces=.. lane_docs=..
 * long_docs=..").
 *
 * counts[i] (and checksums[i] when not NULL) for document i = hay[offsets[i], offsets[i+1]).  offsets (n + 1 entries) live where the
 * haystack lives (hay_is_device); counts / checksums are host arrays, or device arrays when out_is_device != 0, in which case the call is
 * asynchronous on `stream` after the offsets' validation (find_iter / leftmost_find_iter with long documents synchronise per such document). */
daac_status daac_scan_count_batch(daac_pma *pma, int mode, int engine, const uint8_t *hay, const uint64_t *offsets, size_t n, int hay_is_device,
                                  void *stream, uint64_t *counts, uint64_t *checksums, int out_is_device);
/* All documents' tuples as one CSR list in device memory: *dev_out holds *total daac_match16 {end, length, value} (end relative to the
 * document; NULL when there are none), *dev_doc_offsets holds n + 1 u64, and document i's matches are [doc_offsets[i], doc_offsets[i+1]),
 * in the reference's order.  Both buffers are released with daac_device_free.  The call returns after the stream has finished. */
daac_status daac_scan_batch_device16(daac_pma *pma, int mode, int engine, const uint8_t *hay, const uint64_t *offsets, size_t n, int hay_is_device,
                                     void *stream, daac_match16 **dev_out, uint64_t **dev_doc_offsets, uint64_t *total);

/* ---- histograms: which patterns occurred, and how often -------------------------------------------------------------------------
 * Every pattern has exactly one output record {value, length, parent} (src/lib.rs:213-218; parent is 1-based, 0 = none): record i, in
 * the automaton's order, is "slot i".  daac_pma_outputs copies the n = daac_info.outputs_len records (3 u32 each) to `out`, at most `cap`
 * of them, and returns n.  Host only, no device. */
size_t daac_pma_outputs(const daac_pma *pma, uint32_t *out, size_t cap);
/* counts[i] = number of matches of slot i's pattern among the matches daac_scan_count_range(mode, begin) counts: end in (begin, len],
 * ROOT's list at end 0 when begin == 0.  The sum over i equals that call's count, so the histograms of the shards of one haystack
 * simply add.  counts has outputs_len u64 and is overwritten; it is a host array, or a device array when counts_is_device != 0 (then
 * the call is asynchronous on `stream` for a device haystack).  Patterns that share a value are summed by the caller (the records
 * carry the value).
 * Modes: DAAC_FIND_OVERLAPPING (every hit counts its whole output list) and DAAC_FIND_OVERLAPPING_NO_SUFFIX (the head of the list
 * only); DAAC_FIND / DAAC_LEFTMOST_FIND answer 6.  Engines AUTO, TIERED and DARRAY by the rules of the other scans (GRAM and PFX: 6;
 * charwise handles: their double array).  A MatchKind mismatch is 5, NULL counts with outputs_len > 0 and begin > len are 1, all before
 * any device work.  An empty haystack or automaton is OK (ROOT's list at 0 is still counted when begin == 0).
 * The scan adds 1 at the head slot of every hit (32-bit counters, the first hist_lds_bins slots per workgroup in LDS; ranges of 2^32
 * bytes and more take several launches), and one small kernel then adds every head's total to the ancestors on its parent chain.
 * daac_last_kernel() says "hist eng=tier|darray|char lds_bins=N". */
daac_status daac_scan_histogram(daac_pma *pma, int mode, int engine, const uint8_t *hay, size_t len, size_t begin, int hay_is_device,
                                void *stream, uint64_t *counts, int counts_is_device);

/* ---- per-document pattern counts of a batch: which patterns occurred in which document, and how often ----------------------------
 * The matrix documents x slots in CSR form, in device memory: *dev_rows holds *total rows {slot, count} (NULL when there are none),
 * *dev_doc_offsets holds n + 1 u64, and document i's rows are [doc_offsets[i], doc_offsets[i+1]): one row per slot (index into
 * daac_pma_outputs) with a non-zero count in that document, in ascending slot order.  count = the matches of that slot's pattern among
 * the matches the single-haystack iterator of `mode` reports on the document alone (the contract of daac_scan_count_batch: nothing
 * crosses a document boundary, ROOT's "" match is reported at each document's 0), so a document's counts add up to its
 * daac_scan_count_batch count.  The output is a function of the input alone and compares bit for bit between calls.  Both buffers are
 * released with daac_device_free; the call returns after the stream has finished.  n = 0: *dev_rows = NULL, *dev_doc_offsets = one 0.
 * The batch arguments are those of daac_scan_batch_device16.  Modes: all four (DAAC_FIND_OVERLAPPING counts the whole output list of
 * every hit).  Engines and their refusals are the batches': AUTO, TIERED, DARRAY; GRAM / PFX, charwise + TIERED, find_iter /
 * leftmost_find_iter + TIERED: 6; a MatchKind mismatch: 5.  NULL out-pointers, NULL offsets with n > 0 and offsets that decrease: 1.
 * A document of 2^32 - 1 bytes or more: 6, naming the document (a slot takes at most one match per position plus ROOT's at 0, so a
 * 32-bit count cannot wrap below that length).  DAAC_FIND / DAAC_LEFTMOST_FIND with a document longer than option batch_lane_max: 6,
 * naming the first such document and the option — the single-haystack route the tuple batches give such documents yields
 * (value, length), not slots; a caller raises batch_lane_max (up to its clamp, 2^30 - 1) and pays one lane's walk over the document.
 * With host offsets all of these are decided before a device is touched.  Note D (see above): 6, naming the document.  Status 4 when
 * 8 bytes times the number of matches exceeds max_result_bytes, before the records are allocated (the tuple lists answer 2 there).
 * Method: one 8-byte record (the slot) per match at the place an exclusive scan of the per-piece / per-document counts gives it, then
 * a reduction of each document's records by their number R — R <= batch_hist_wave_max: one wave sorts the slots in LDS and run-length
 * encodes them; R <= batch_hist_sort_max: one workgroup does; above: a row of outputs_len u32 counters in HBM, compacted in slot order
 * — an exclusive scan of the row counts and a copy.  daac_last_kernel() says "batch_hist pieces=.. records=.. wave_docs=..
 * group_docs=.. dense_docs=..". */
typedef struct daac_slot_count {
    uint32_t slot;        /* index into daac_pma_outputs */
    uint32_t count;
} daac_slot_count;
daac_status daac_scan_histogram_batch(daac_pma *pma, int mode, int engine, const uint8_t *hay, const uint64_t *offsets, size_t n, int hay_is_device,
                                      void *stream, daac_slot_count **dev_rows, uint64_t **dev_doc_offsets, uint64_t *total);

/* ---- replace_all: the text with every match replaced ------------------------------------------------------------------------------
 * With m_0 .. m_{k-1} the matches the iterator of `mode` reports on hay, in its order, and r(m) the replacement of match m, the result is
 *     hay[0 : start_0] + r(m_0) + hay[end_0 : start_1] + r(m_1) + ... + r(m_{k-1}) + hay[end_{k-1} : len]
 * (replace_all of the aho-corasick crate over find_iter / leftmost_find_iter).  Modes: DAAC_FIND on Standard automata, DAAC_LEFTMOST_FIND
 * on the leftmost kinds (a mismatch: 5), bytewise and charwise; positions are bytes.  DAAC_FIND_OVERLAPPING and
 * DAAC_FIND_OVERLAPPING_NO_SUFFIX: 6 — overlapping matches have no splice.  An empty match ("" among the patterns) is an insertion.
 * Replacements: n_repl byte strings, replacement i = repl[repl_offsets[i], repl_offsets[i+1]) (host arrays, n_repl + 1 non-decreasing
 * offsets below 4 GiB; copied to the device on the stream per call).  n_repl == 1: every match takes replacement 0.  Otherwise a match
 * takes replacement number `value` — automata built without values number them by pattern index, so this is "replacement i for pattern
 * i"; with values, one replacement per category — and a match whose value is >= n_repl makes the call answer 1 (daac_last_error() names
 * the value and the match's start; nothing has been allocated for the caller then).  Replacements may be empty (deletion).
 * The result stays in device memory: *dev_out holds *out_len bytes (NULL when *out_len == 0), released with daac_device_free and copied
 * with daac_device_to_host; *n_replaced = k.  The call returns after the stream has finished.
 * Statuses decided before a device is touched: NULL out-pointers, n_repl == 0, repl_offsets NULL or decreasing, repl NULL with a
 * non-empty blob: 1; the overlapping modes: 6; a MatchKind mismatch: 5.  The tuple list is daac_scan_device16's (the batch:
 * daac_scan_batch_device16's): its engines and their refusals, note D (6) and the max_result_bytes rule of the list are this call's; a
 * result longer than max_result_bytes answers 2 before it is allocated.
 * A host haystack is staged to the device ONCE and whole — the splice reads the text there — not in windows: it has to fit next to the
 * tuple list and the result.
 * Method: one lane per match sizes it (replacement length, match length), two exclusive sums give O_i = start_i - sum of the lengths
 * before + sum of the replacement lengths before, the output position of match i's replacement; after one read-back of the totals the
 * result is allocated and written output-parallel, 16 bytes a lane: output byte q belongs to the largest i with O_i <= q (replacement
 * byte q - O_i, or the text behind end_i), which is what makes matches that share an output position right.  Integer work only: the
 * result is a function of the input alone.  daac_last_kernel() says "replace matches=.. out=.." in front of what the tuple call reported. */
daac_status daac_replace_all(daac_pma *pma, int mode, int engine, const uint8_t *hay, size_t len, int hay_is_device, void *stream,
                             const uint8_t *repl, const uint64_t *repl_offsets, size_t n_repl,
                             uint8_t **dev_out, uint64_t *out_len, uint64_t *n_replaced);
/* The same for a batch (the batch arguments and their rules are daac_scan_batch_device16's): every document is replaced as a haystack
 * of its own — nothing crosses a boundary, a chain starts fresh at each document's 0.  Document i's result is
 * dev_out[out_offsets[i], out_offsets[i+1]); *dev_out_offsets holds n + 1 u64 in device memory (daac_device_free).  n = 0: *dev_out =
 * NULL and one offset, 0.  Note D names the document. */
daac_status daac_replace_all_batch(daac_pma *pma, int mode, int engine, const uint8_t *hay, const uint64_t *offsets, size_t n, int hay_is_device,
                                   void *stream, const uint8_t *repl, const uint64_t *repl_offsets, size_t n_repl,
                                   uint8_t **dev_out, uint64_t **dev_out_offsets, uint64_t *out_len, uint64_t *n_replaced);

/* ---- tokenize: match values and gap tokens as an id list ---------------------------------------------------------------------------
 * With m_0 .. m_{k-1} the matches the iterator of `mode` reports on hay (ordered, disjoint, positions in bytes), the gaps are
 * g_0 = [0, start_0), g_i = [end_{i-1}, start_i), g_k = [end_{k-1}, len) (no match: the one gap [0, len)), and the token sequence is
 * tok(g_0), m_0, tok(g_1), m_1, .., m_{k-1}, tok(g_k).  A match token is {id = value, start, end}; an empty match ("" among the patterns)
 * is a token with start == end and separates two gaps like any other.  What a gap [a, b) contributes is `gap`'s choice: */
typedef enum {
    DAAC_GAP_SKIP = 0,  /* nothing */
    DAAC_GAP_UNK = 1,   /* nothing if a == b, else one token {gap_id, a, b} */
    DAAC_GAP_BYTES = 2, /* one token per byte p: {gap_id + hay[p], p, p + 1} (byte fallback) */
    DAAC_GAP_CHARS = 3  /* the gap cut at a, at every p in (a, b) with (hay[p] & 0xC0) != 0x80, and at b: one {gap_id, c_j, c_j+1} per piece —
                         * one unknown token per UTF-8 code point; the rule looks at single bytes only, so it is defined for any bytes, and
                         * a gap that begins with continuation bytes still starts a token at a */
} daac_gap;
/* Modes: DAAC_FIND on Standard automata, DAAC_LEFTMOST_FIND on the leftmost kinds, bytewise and charwise handles.  *dev_ids holds
 * *n_tokens u32 in device memory (NULL when there are none); dev_spans may be NULL (not wanted), otherwise *dev_spans holds 2 * n_tokens
 * u64, {start, end} per token; *n_matches = k.  Both buffers are released with daac_device_free and copied with daac_device_to_host.
 * The call returns after the stream has finished.
 * Decided before a device is touched — a NULL dev_ids, n_tokens or n_matches, a gap outside 0..3, DAAC_GAP_BYTES with gap_id >
 * 0xFFFFFFFF - 255: 1; the overlapping modes: 6; a MatchKind mismatch: 5.  The tuple list is daac_scan_device16's (the batch:
 * daac_scan_batch_device16's): its engines and their refusals, note D (6) and the max_result_bytes rule of the list are this call's; a
 * result above max_result_bytes (4 bytes a token, 16 more with spans) answers 2 before it is allocated.  A host haystack is copied to
 * the device once.
 * Method: the text is cut into tiles of 4 KiB, a lane takes 16 bytes.  From the matches and document beginnings that touch its bytes
 * (found by one binary search per tile and one per lane inside the tile's range) and the gap rule a lane derives the 16-bit mask of
 * bytes at which a token begins; a count pass sums the masks per tile, an exclusive sum gives the tiles' bases, and after one read-back
 * of the totals the result is allocated and a write pass places ids and spans by wave and workgroup prefix sums.  Empty matches are
 * placed by an exclusive sum over the match list.  No atomics, integer work only: the result is a function of the input alone.
 * daac_last_kernel() says "tokenize matches=.. tokens=.." in front of what the tuple call reported. */
daac_status daac_tokenize(daac_pma *pma, int mode, int engine, const uint8_t *hay, size_t len, int hay_is_device, void *stream,
                          int gap, uint32_t gap_id,
                          uint32_t **dev_ids, uint64_t **dev_spans, uint64_t *n_tokens, uint64_t *n_matches);
/* The same for a batch (the batch arguments and their rules are daac_scan_batch_device16's): every document is tokenized as a haystack
 * of its own — no gap crosses a boundary, positions are relative to the document's first byte.  Document i's tokens are
 * [tok_offsets[i], tok_offsets[i+1]); *dev_tok_offsets (never NULL as an argument) holds n + 1 u64 in device memory (daac_device_free).
 * n = 0: *dev_ids = NULL and one offset, 0.  Note D names the document. */
daac_status daac_tokenize_batch(daac_pma *pma, int mode, int engine, const uint8_t *hay, const uint64_t *offsets, size_t n, int hay_is_device,
                                void *stream, int gap, uint32_t gap_id,
                                uint32_t **dev_ids, uint64_t **dev_spans, uint64_t **dev_tok_offsets, uint64_t *n_tokens, uint64_t *n_matches);

/* ---- tokenize_unigram: the segmentation whose pieces' scores sum highest ----------------------------------------------------------------
 * What the SentencePiece Unigram model and the minimum-cost lattice walk of a morphological analyser compute: not the longest match
 * first, but the best path through the lattice of all dictionary pieces.  Inputs: a Standard automaton (bytewise or charwise), a text or
 * a batch of documents, `scores` (n_scores float32, indexed by match value; a host array, copied once per call), `unk_score`, `gap`
 * (DAAC_GAP_BYTES or DAAC_GAP_CHARS) and `gap_id`.  Every document is a problem of its own.  For a document doc of L bytes:
 *   Nodes: the byte positions 0 .. L.
 *   Match edges: every match (start, end, value) of find_overlapping_iter(doc) with start < end is an edge start -> end with score
 *     scores[value] and id value.  Empty matches ("" among the patterns) are not edges.
 *   Unknown edges: the cuts are 0, L and — DAAC_GAP_BYTES: every position; DAAC_GAP_CHARS: every p with (doc[p] & 0xC0) != 0x80 (the
 *     single-byte rule of daac_gap, defined on any bytes).  Consecutive cuts c -> c' are an edge with score unk_score and id gap_id
 *     (_CHARS) or gap_id + doc[c] (_BYTES).  The cuts chain from 0 to L, so L is always reachable.
 *   Best score: best[0] = +0.0f.  For q = 1 .. L the incumbent starts at -inf with no edge; the candidates are visited in this order: the
 *     match edges into q in the order find_overlapping_iter reports them, then the unknown edge into q if q is a cut.  A candidate's score
 *     is the single float32 addition best[from] + score (round to nearest, nothing fused or reassociated) and replaces the incumbent only
 *     when strictly greater (>): ties go to the earliest match in the reference's order and to a match before the unknown edge.  An edge
 *     out of an unreachable node (-inf) is never recorded.
 *   Result: the edges on the back-pointer path from L to 0, in text order; a token is {id, start, end} with byte positions relative to
 *     the document, the document's score is best[L].  An empty document has no tokens and score +0.0f.
 * With this order and the single addition the ids, the spans and the 32 bits of every score are a function of the input alone.
 * Against SentencePiece itself (pieces but <unk> as patterns, value = id, U+2581 written for every space by the caller, unk_score = the
 * lowest piece score - 10, DAAC_GAP_CHARS with gap_id = unk_id) the ids are sentencepiece's with one deliberate difference: a run of
 * unknown code points is one token per code point here, each with its span, and one unk id there; a caller that wants that list drops
 * every unk id that follows one.  The tie order above is sentencepiece's (the longest piece into a position is met first).
 * Results follow daac_tokenize: *dev_ids holds *n_tokens u32 in device memory (NULL when there are none), dev_spans may be NULL (not
 * wanted), otherwise 2 * n_tokens u64; *n_matches = the tuples of the lattice, empty matches included; `score` (host, may be NULL)
 * receives best[L].  Buffers are released with daac_device_free.  The call returns after the stream has finished.  There is no mode: the
 * lattice is DAAC_FIND_OVERLAPPING.
 * Decided before a device is touched, in this order.  Status 1: a NULL dev_ids, n_tokens or n_matches (the batch: dev_tok_offsets too);
 * a gap that is neither DAAC_GAP_BYTES nor DAAC_GAP_CHARS; DAAC_GAP_BYTES with gap_id > 0xFFFFFFFF - 255; n_scores not above the largest
 * value among daac_pma_outputs; a score or unk_score that is NaN, infinite or above 1e20 in magnitude (a path has fewer than 2^32 edges,
 * so with that bound no path sum can overflow float32 on any text the call accepts); the batch's own offset rules, as in
 * daac_tokenize_batch.  Status 5: a leftmost automaton.  The tuple list is daac_scan_batch_device16's: its engines and their refusals
 * (6) and the max_result_bytes rule of the list are this call's; a token list above max_result_bytes (4 bytes a token, 16 more with
 * spans) answers 2 before it is allocated.  A host text is copied to the device once.
 * Method: the unit of parallelism is the document — one lane walks one document, 64 documents to a wave, which is what these tokenizers
 * are fed (words after the whitespace split, sentences: 10^5 .. 10^7 documents of 5 .. 300 bytes).  A forward pass walks q = 1 .. L
 * through the document's tuples (their ends do not decrease) and stores best[q] and the winning edge {length, id} per position (12 bytes
 * of scratch per byte of text); a count pass follows the back pointers from L, an exclusive sum of the counts gives tok_offsets and the
 * total (one read-back), and a write pass follows them again and fills the document's range from the back.  No atomics.
 * Limits: a wave takes as long as its longest document, and one long haystack runs on a single lane — daac_tokenize_unigram on a long
 * text is correct and slow.  A document of 2^32 - 1 bytes or more answers 6.
 * daac_last_kernel() says "unigram docs=.. matches=.. tokens=.." in front of what the tuple call reported. */
daac_status daac_tokenize_unigram(daac_pma *pma, int engine, const uint8_t *hay, size_t len, int hay_is_device, void *stream,
                                  const float *scores, size_t n_scores, float unk_score, int gap, uint32_t gap_id,
                                  uint32_t **dev_ids, uint64_t **dev_spans, uint64_t *n_tokens, uint64_t *n_matches, float *score);
/* The same for a batch (the batch arguments and their rules are daac_scan_batch_device16's).  Document i's tokens are
 * [tok_offsets[i], tok_offsets[i+1]); *dev_tok_offsets (never NULL as an argument) holds n + 1 u64 in device memory; dev_doc_scores may be
 * NULL (not wanted), otherwise *dev_doc_scores holds n float32 in device memory (both: daac_device_free).  n = 0: *dev_ids = NULL, one
 * offset, 0, and no scores. */
daac_status daac_tokenize_unigram_batch(daac_pma *pma, int engine, const uint8_t *hay, const uint64_t *offsets, size_t n, int hay_is_device,
                                        void *stream, const float *scores, size_t n_scores, float unk_score, int gap, uint32_t gap_id,
                                        uint32_t **dev_ids, uint64_t **dev_spans, uint64_t **dev_tok_offsets, float **dev_doc_scores,
                                        uint64_t *n_tokens, uint64_t *n_matches);

/* ---- tokenize_bpe: byte-pair merging in rank order ----------------------------------------------------------------------------------------
 * What tiktoken's byte_pair_merge computes for one piece of pre-split text (the cl100k / o200k, GPT-2, Llama and Mistral vocabularies):
 * neither the longest match first nor a best-scoring path, but the parts left when neighbouring parts have been merged in the order of
 * their ranks.  For "abcd" with "bc" ranked before "ab" and "bcd" in the vocabulary it gives a|bcd where longest-match-first gives
 * ab|c|d.  Inputs: a Standard automaton (bytewise or charwise), a text or a batch of documents, `ranks` (n_ranks uint32, indexed by
 * match value; a host array, copied once per call; ranks = NULL with n_ranks = 0: a piece's rank is its value), `gap` (DAAC_GAP_BYTES
 * or DAAC_GAP_CHARS) and `gap_id`.  Every document is a problem of its own.  For a document doc of L bytes:
 *   Pieces: piece(s, e) for 0 <= s < e <= L is the value v of the match (s, e, v) in find_overlapping_iter(doc); it is absent when there
 *     is no such match (patterns are unique, so there is at most one).  Empty matches ("" among the patterns) are not pieces.
 *     rank(s, e) is ranks[v], or v without a table.  A rank of 0xFFFFFFFF means the piece is never the product of a merge; such a piece
 *     can still be an initial part.
 *   Initial parts: the boundaries are the cuts of daac_gap — 0, L and — DAAC_GAP_BYTES: every position; DAAC_GAP_CHARS: every p with
 *     (doc[p] & 0xC0) != 0x80 (the single-byte rule, defined on any bytes).  Consecutive boundaries delimit the parts.
 *   Merge loop: with the live boundaries p_0 = 0 < p_1 < .. < p_k = L, among all i with piece(p_i, p_{i+2}) present and its rank not
 *     0xFFFFFFFF take the smallest rank, on ties the smallest i; remove p_{i+1}; repeat until no such i exists.  Ranks are looked up by
 *     the concatenated bytes, not by the pair (as tiktoken does; a merges.txt vocabulary keyed by pairs is another rule).
 *   Result: one token per final part (p_i, p_{i+1}), in text order.  Its id is piece(p_i, p_{i+1}) when present; otherwise the part is
 *     an initial part that the vocabulary lacks and its id is gap_id + doc[p_i] (_BYTES) or gap_id (_CHARS).  An absent initial part
 *     still takes part in merges like any other part: piece is defined on byte ranges only.  A token is {id, start, end} with byte
 *     positions relative to the document.  An empty document has no tokens.
 * The result does not depend on the order of tuples that share an end: it is a function of the input alone.
 * Results follow daac_tokenize: *dev_ids holds *n_tokens u32 in device memory (NULL when there are none), dev_spans may be NULL (not
 * wanted), otherwise 2 * n_tokens u64; *n_matches = the tuples of the scan, empty matches included.  Buffers are released with
 * daac_device_free.  The call returns after the stream has finished.  There is no mode: the pieces are DAAC_FIND_OVERLAPPING's.
 * Decided before a device is touched, in this order.  Status 1: a NULL dev_ids, n_tokens or n_matches (the batch: dev_tok_offsets too);
 * a gap that is neither DAAC_GAP_BYTES nor DAAC_GAP_CHARS; DAAC_GAP_BYTES with gap_id > 0xFFFFFFFF - 255; ranks == NULL with n_ranks != 0
 * or the reverse; a non-NULL ranks whose n_ranks is not above the largest value among daac_pma_outputs; the batch's own offset rules, as
 * in daac_tokenize_batch.  Status 5: a leftmost automaton.  Then the length cap: the merge loop scans a document's live parts once per
 * merge, up to L^2 / 2 part visits on one lane, so a document longer than option bpe_doc_max (4096 — about 8.4 M visits; 1 .. 65536)
 * answers 6 before a kernel of this call is launched, and the message names the document and says to pre-split the text (real BPE runs
 * behind a pre-tokenizer split: its inputs are words).  Host offsets are checked before a device is touched, device offsets by one
 * read-back of the first and last offset, and of all of them when those two are further apart than the cap.  The tuple list is
 * daac_scan_batch_device16's: its engines and their refusals (6) and the max_result_bytes rule of the list are this call's; a token list
 * above max_result_bytes (4 bytes a token, 16 more with spans) answers 2 before it is allocated.  A host text is copied to the device once.
 * Method: the unit of parallelism is the document — one lane per document, 64 documents to a wave.  The lane indexes its tuples by end
 * (piece(s, e) is then a look through the tuples that end at e), links the initial boundaries, caches the rank and value of every pair of
 * neighbours and loops: a linear minimum over the live pairs, unlink, recompute the two neighbouring pairs (24 bytes of scratch per byte
 * of text).  The live-part counts are summed to tok_offsets and the total (one read-back), and a write pass walks the links and fills
 * the document's range.  No atomics, integer work only.
 * daac_last_kernel() says "bpe docs=.. matches=.. tokens=.." in front of what the tuple call reported. */
daac_status daac_tokenize_bpe(daac_pma *pma, int engine, const uint8_t *hay, size_t len, int hay_is_device, void *stream,
                              const uint32_t *ranks, size_t n_ranks, int gap, uint32_t gap_id,
                              uint32_t **dev_ids, uint64_t **dev_spans, uint64_t *n_tokens, uint64_t *n_matches);
/* The same for a batch (the batch arguments and their rules are daac_scan_batch_device16's).  Document i's tokens are
 * [tok_offsets[i], tok_offsets[i+1]); *dev_tok_offsets (never NULL as an argument) holds n + 1 u64 in device memory (daac_device_free).
 * n = 0: *dev_ids = NULL and one offset, 0. */
daac_status daac_tokenize_bpe_batch(daac_pma *pma, int engine, const uint8_t *hay, const uint64_t *offsets, size_t n, int hay_is_device,
                                    void *stream, const uint32_t *ranks, size_t n_ranks, int gap, uint32_t gap_id,
                                    uint32_t **dev_ids, uint64_t **dev_spans, uint64_t **dev_tok_offsets,
                                    uint64_t *n_tokens, uint64_t *n_matches);

/* ---- split_batch: the pre-tokenizer split of a batch into words --------------------------------------------------------------------------
 * What stands in front of the three tokenizers above on real text: every document is cut into words, and (hay, word_offsets) is itself
 * a batch that every *_batch call accepts.  No automaton is involved: a splitter is a rule and a table of character classes.
 *   Units: a document is any bytes.  It is cut into units by the well-formed UTF-8 table (Unicode Table 3-7: lead bytes C2..F4 only;
 *     E0 / ED / F0 / F4 restrict their second byte; no overlong forms, no surrogates, nothing above U+10FFFF).  A well-formed sequence
 *     that lies wholly inside the document is one unit, and its class is the class of its code point.  Every other byte is a unit of its
 *     own, of class O.  Documents are independent: a sequence cut by a document's end is malformed, and no look-back or look-ahead
 *     leaves the document.
 *   Classes: L (letter), N (number), S (whitespace) and O (everything else).  Below U+0080 they are fixed: A-Z a-z are L, 0-9 are N,
 *     0x09..0x0D and 0x20 are S, the rest is O.  From U+0080 on they come from the splitter's table of sorted, disjoint ranges
 *     {first, last, cls}, cls in {1 = L, 2 = N, 3 = S}; a code point in no range is O.  Under DAAC_SPLIT_O200K alone cls may also be
 *     4 (an upper letter: general categories Lu, Lt), 5 (a lower letter: Ll) or 6 (a mark: M*); 1 then means a caseless letter (Lm, Lo),
 *     and below U+0080 A-Z are upper and a-z lower.  A splitter of any other rule refuses cls above 3.
 *   Rules: each partitions every document — its words are contiguous and cover it, nothing is dropped.
 *     DAAC_SPLIT_WHITESPACE: the words are the matches of \s+|\S+: maximal runs of S units and maximal runs of other units.
 *     DAAC_SPLIT_GPT2: the words are the successive matches of
 *       's|'t|'re|'ve|'m|'ll|'d| ?\p{L}+| ?\p{N}+| ?[^\s\p{L}\p{N}]+|\s+(?!\S)|\s+
 *     with \p{L} = L, \p{N} = N and \s = S, case-sensitive: the sequential scanner that tries the alternatives in order at each
 *     position, greedy, the fifth alternative backtracking.  (GPT-2, RoBERTa, BART and every byte-level BPE vocabulary trained with it.)
 *     DAAC_SPLIT_LLAMA3: the words are the successive matches of the pattern of Llama-3's tokenizer.json,
 *       (?i:'s|'t|'re|'ve|'m|'ll|'d)|[^\r\n\p{L}\p{N}]?\p{L}+|\p{N}{1,3}| ?[^\s\p{L}\p{N}]+[\r\n]*|\s*[\r\n]+|\s+(?!\S)|\s+
 *     DAAC_SPLIT_CL100K: the words are the successive matches of tiktoken's cl100k_base pattern,
 *       '(?i:[sdmt]|ll|ve|re)|[^\r\n\p{L}\p{N}]?+\p{L}++|\p{N}{1,3}+| ?[^\s\p{L}\p{N}]++[\r\n]*+|\s++$|\s*[\r\n]|\s+(?!\S)|\s+
 *     In both, \p{L} = L, \p{N} = N, \s = S, \r and \n are the bytes 0x0D and 0x0A, the space is the byte 0x20, `+` behind a
 *     quantifier makes it possessive ({1,3}+ included: up to three N units, nothing given back), and `$` is the document's end only, not
 *     a line's.  (?i:) is Unicode simple case folding: a contraction letter matches in either ASCII case, and U+017F (LATIN SMALL LETTER
 *     LONG S) matches s where the table has it in class L (char_classes() does); nothing else folds onto these letters (U+212A KELVIN
 *     SIGN folds to k).  The two rules differ only at a whitespace run that reaches the document's end: cl100k's \s++$ keeps the run
 *     as one word, Llama-3 cuts it behind its last newline.  The values 2 and 5 are reserved and refused.  (cl100k_base / GPT-4 vocabularies;
 *     Llama-3 and the vocabularies trained with its pattern.  `tokenizers` reads {1,3}+ as a repeated interval, so for the cl100k
 *     pattern as written it gives other words than tiktoken and this rule do: 1281 is 128|1 here.)
 *     DAAC_SPLIT_BERT: BERT's pre-tokenizer (BasicTokenizer's whitespace and punctuation split; `tokenizers`' BertPreTokenizer) as a
 *     partition: a maximal run of S units is a word, every O unit is a word of its own, a maximal run of L and N units is a word.  The
 *     words that are no whitespace (daac_split_words_space tells which are) are BertPreTokenizer's words when O is BERT's punctuation.
 *     Below U+0080 the fixed classes give that: every printable ASCII character that is neither alphanumeric nor a space is BERT
 *     punctuation.  From U+0080 on it takes a table with the categories P* in no range and M*, S*, C* and unassigned code points in L
 *     (the Python package's bert_char_classes()).  Two differences from `tokenizers` are deliberate.  ASCII control characters other
 *     than 0x09..0x0D are O here and become words of their own where `tokenizers` leaves them inside words: BERT's normalizer
 *     (clean_text) removes them before the split, which is the caller's job as lower-casing and accent stripping are.  Ill-formed UTF-8
 *     bytes are O units, as everywhere in the splitter.  The rule looks one unit back and launches no scan.
 *     DAAC_SPLIT_O200K: the words are the successive matches of tiktoken's o200k_base pattern,
 *       [^\r\n\p{L}\p{N}]?[\p{Lu}\p{Lt}\p{Lm}\p{Lo}\p{M}]*[\p{Ll}\p{Lm}\p{Lo}\p{M}]+(?i:'s|'t|'re|'ve|'m|'ll|'d)?
 *       |[^\r\n\p{L}\p{N}]?[\p{Lu}\p{Lt}\p{Lm}\p{Lo}\p{M}]+[\p{Ll}\p{Lm}\p{Lo}\p{M}]*(?i:'s|'t|'re|'ve|'m|'ll|'d)?
 *       |\p{N}{1,3}| ?[^\s\p{L}\p{N}]+[\r\n/]*|\s*[\r\n]+|\s+(?!\S)|\s+
 *     with \p{Lu}\p{Lt} = class 4, \p{Ll} = 5, \p{Lm}\p{Lo} = 1, \p{M} = 6, \p{L} = 1, 4 and 5, \p{N} = N, \s = S; bytes, folding and
 *     `(?i:)` as in the two rules above (U+017F matches s where the table has it as a letter of any case).  The quantifiers are greedy
 *     and give back.  How it differs from those two rules: (1) a word body is upper-or-caseless units (4, 1, 6) then at least one
 *     lower-or-caseless unit (5, 1, 6), or failing that at least one of the first kind then any of the second, so HTMLParser is one
 *     word, XMLHttpRequest is XMLHttp|Request, and a run of upper letters that reaches a non-letter backs off to the last caseless unit
 *     or mark in front of it (AB<Lo>CD -> AB<Lo>|CD, but AB<Lo>CDe is one word); (2) a mark is not \p{L}: it can be the optional
 *     prefix and belongs to the punctuation alternative, and it is also word body, so !<M>abc is one word while !!<M>abc is
 *     !!<M>|abc; (3) a contraction is a suffix of the word in front of it (don't and DON'T are one word, 1's is 1|'s), not a word of
 *     its own; (4) the punctuation alternative's trailer also takes / (!\n/! -> !\n/|!, !/! is one word); (5) numbers, newlines and
 *     whitespace are Llama-3's.  The value 7 is refused.  (o200k_base: GPT-4o and the vocabularies trained with its pattern; the Python
 *     package's o200k_char_classes() has the table.)
 *   The kernels evaluate an equivalent local form — whether a word starts at a unit follows from three units in front of it and one
 *     behind it (split_kernels.hip states it) — so the unit of parallelism is the byte.  A word start is always the first byte of a unit.
 *     DAAC_SPLIT_CL100K and DAAC_SPLIT_LLAMA3 read four more bits of a unit that depend on runs of any length (a digit's index in its
 *     run mod 3, a newline run behind punctuation, a newline farther on in a whitespace run, a whitespace run up to the document's
 *     end): segmented scans over the batch that start again at every document, two forwards and two backwards, in two more passes —
 *     per-tile summaries, then one workgroup that resolves the carries across tiles.  No workgroup waits for another, and the work at a
 *     byte does not depend on the length of the run it lies in.  Scratch for them: 12 bytes per 1024 bytes of text.
 *     DAAC_SPLIT_O200K runs the same three passes with kernels of its own: forwards one automaton of 13 states (the kind of match a
 *     unit lies in, the case phase of a word body, a digit's index mod 3) whose transitions compose as packed maps, backwards two bits
 *     (a newline farther on in a whitespace run; a run of upper letters that ends at a non-letter).  Scratch: 20 bytes per 1024 bytes.
 * daac_splitter_create builds a two-stage class table on the host from the ranges (n_ranges = 0: every code point from U+0080 on is O),
 * two bits a code point, four under DAAC_SPLIT_O200K;
 * the table is uploaded per device on first use.  Status 1: a NULL out, an unknown rule, ranges that are unsorted, overlapping, have
 * last < first, first < 0x80, last > 0x10FFFF or cls outside 1..3 (1..6 under DAAC_SPLIT_O200K).
 * daac_split_batch: *dev_word_offsets holds *n_words + 1 u64 positions in hay — absolute, entry 0 is offsets[0], the last entry is
 * offsets[n]; *dev_doc_words holds n + 1 u64: document i's words are [doc_words[i], doc_words[i+1]), an empty document has none,
 * doc_words[n] == n_words.  Both are device memory, released with daac_device_free.  The call returns after the stream has finished.
 * n = 0: one word offset and one doc_words entry, both 0, and *n_words = 0.  No byte outside [offsets[0], offsets[n]) is read.
 * Decided before a device is touched — status 1: a NULL sp, dev_word_offsets, dev_doc_words or n_words; the batch offset rules of
 * daac_scan_count_batch (host offsets; device offsets are validated as that call validates them, with one read-back).  Status 2: a
 * word list above the process-wide option max_result_bytes (8 bytes a word), answered before it is allocated.  A host haystack is
 * copied to the device once.  daac_last_kernel() says "split rule=.. docs=.. bytes=.. words=.." (rule=whitespace, gpt2, cl100k, llama3, bert or o200k).
 * Method: one lane per document marks its first byte in a bit array; a workgroup stages a tile of 1024 bytes, 12 in front and 7 behind
 * in LDS and each lane decides its byte; a wave ballot makes a 64-bit mask word; the per-tile popcounts are summed (one read-back of
 * the total) and a second pass writes every start at its rank.  Integer work only: the result is a function of the input alone. */
typedef enum {
    DAAC_SPLIT_WHITESPACE = 0,
    DAAC_SPLIT_GPT2 = 1,
    /* 2 is reserved (daac_splitter_create refuses it) */
    DAAC_SPLIT_CL100K = 3,
    DAAC_SPLIT_LLAMA3 = 4,
    /* 5 is refused, as it has been since the rules above were added */
    DAAC_SPLIT_BERT = 6,
    /* 7 is refused */
    DAAC_SPLIT_O200K = 8
} daac_split_rule;
typedef struct { uint32_t first, last, cls; } daac_char_range;
typedef struct daac_splitter daac_splitter;
daac_status daac_splitter_create(int rule, const daac_char_range *ranges, size_t n_ranges, daac_splitter **out);
void daac_splitter_free(daac_splitter *sp);
daac_status daac_split_batch(daac_splitter *sp, const uint8_t *hay, const uint64_t *offsets, size_t n, int hay_is_device, void *stream,
                             uint64_t **dev_word_offsets, uint64_t **dev_doc_words, uint64_t *n_words);
/* A single haystack: a batch of one document {0, len}. */
daac_status daac_split(daac_splitter *sp, const uint8_t *hay, size_t len, int hay_is_device, void *stream,
                       uint64_t **dev_word_offsets, uint64_t *n_words);
/* Which words are whitespace: *dev_flags holds n_words bytes in device memory (daac_device_free), flags[w] = 1 iff word w =
 * [word_offsets[w], word_offsets[w+1]) of hay is not empty and its first unit is of class S — the unit taken inside the word, by the
 * splitter's own unit rule and class table.  Under DAAC_SPLIT_WHITESPACE and DAAC_SPLIT_BERT such a word is all S.  dev_word_offsets
 * are n_words + 1 absolute positions in hay, in device memory, as daac_split_batch gives them; a host hay is copied to the device once
 * (one read-back of the first and last offset).  One lane per word.  Status 1: a NULL sp or dev_flags, or a NULL hay or
 * dev_word_offsets with n_words > 0.  n_words = 0: *dev_flags = NULL.  Returns after the stream has finished. */
daac_status daac_split_words_space(daac_splitter *sp, const uint8_t *hay, const uint64_t *dev_word_offsets, size_t n_words, int hay_is_device,
                                   void *stream, uint8_t **dev_flags);
/* out[i] = inner[outer[i]] for i < n_outer, all three in device memory (*dev_out: daac_device_free).  With inner = the token offsets of
 * the word batch and outer = doc_words (n + 1 entries) it gives the token offsets per document.  Status 1: a NULL argument. */
daac_status daac_offsets_compose(const uint64_t *dev_inner, const uint64_t *dev_outer, size_t n_outer, void *stream, uint64_t **dev_out);
/* The spans of a word batch's tokens ({start, end} relative to the token's word, in place) made relative to the word's document:
 * tok_offsets (n_words + 1) are the word batch's token offsets, word_offsets and doc_words daac_split_batch's, doc_offsets (n_docs + 1)
 * the offsets that call was given.  One lane per word.  Returns after the stream has finished. */
daac_status daac_spans_rebase(uint64_t *dev_spans, const uint64_t *dev_tok_offsets, const uint64_t *dev_word_offsets, const uint64_t *dev_doc_words,
                              const uint64_t *dev_doc_offsets, size_t n_words, size_t n_docs, void *stream);

/* ---- normalize_batch: a per-code-point rewrite of a batch, on the device ------------------------------------------------------------------
 * What a context-free normalizer computes: every character of a text replaced by a string of zero or more characters that depends on
 * the character alone.  `tokenizers`' BertNormalizer (clean_text, handle_chinese_chars, strip_accents, lowercase) is one but for the
 * canonical reordering of NFD (below); the Python package's bert_normalizer() builds its rules.  NFC and NFKC are not: composition
 * reads the characters around a character.
 * Definition.  A document is cut into the units of daac_split_batch: a well-formed UTF-8 sequence (Unicode Table 3-7) wholly inside its
 *   document is one unit with its code point; every other byte is a unit of its own and is copied unchanged (`tokenizers` cannot be
 *   handed such bytes: it takes a str).  Documents are independent.  The output is the concatenation, per document, of each unit's image
 *   under the rules: a sorted, disjoint list of {first, last, kind, off, len} over code points from U+0000 on; a code point in no rule is
 *   copied.  DAAC_NORM_DELETE: the image is empty.  DAAC_NORM_REPLACE: the image is pool[off .. off + len), the same for every code point
 *   of the range, len <= 255, the pool at most 2^21 bytes.  DAAC_NORM_PAD: 0x20, the unit's own bytes, 0x20.  DAAC_NORM_HANGUL: the
 *   arithmetic decomposition of a Hangul syllable into two or three jamo (Unicode 3.12), accepted only inside U+AC00 .. U+D7A3.  off and
 *   len are read for DAAC_NORM_REPLACE alone.
 * Deliberate differences from `tokenizers`' BertNormalizer with bert_normalizer()'s rules: no canonical reordering — after the marks of
 *   category Mn are dropped only the 23 other characters with a non-zero combining class could be reordered (U+1B44, U+1BAA, U+1BF2,
 *   U+1BF3, U+302E, U+302F, U+A953, U+A9C0, U+111C0, U+11235, U+1134D, U+116B6, U+1193D, U+16FF0, U+16FF1, U+1D165, U+1D166,
 *   U+1D16D .. U+1D172), and two of them side by side stay in the order of the input; ill-formed bytes are copied; the rules follow the
 *   Unicode version of the Python that built them.
 * daac_normalizer_create builds a two-stage table on the host (a direct table for U+0000 .. U+007F; equal blocks of 256 code points
 *   are stored once, so the private-use, CJK and Hangul ranges cost a block each; daac_normalizer_table_bytes says what it came to); it
 *   is uploaded per device on first use.  Status 1: a NULL out, a NULL rules or pool with a non-zero count, rules that are unsorted or
 *   overlap, last < first, last > 0x10FFFF, an unknown kind, a DAAC_NORM_REPLACE rule for one surrogate code point, with off + len
 *   beyond the pool or len above 255, a pool above 2^21 bytes, DAAC_NORM_HANGUL outside its block.
 * daac_normalize_batch: *dev_out holds *out_len bytes and *dev_out_offsets n + 1 u64 from 0, so (out, out_offsets) is a batch again;
 *   with want_src *dev_src holds one u32 per output byte: the offset, from the start of its input document, of the unit that byte came
 *   from (dev_src may be NULL without want_src).  All are device memory, released with daac_device_free.  The call returns after the
 *   stream has finished.  n = 0: no byte and one offset, 0.  No byte outside [offsets[0], offsets[n]) is read.  Decided before a device is
 *   touched — status 1: a NULL argument; the batch offset rules of daac_scan_count_batch (host offsets; device offsets are validated as
 *   that call validates them, with one read-back).  Status 2: an output above the process-wide option max_result_bytes (one byte, with
 *   src five bytes, per output byte), answered before it is allocated.  Status 6: with want_src, a document of 2^32 - 1 bytes or more
 *   (host offsets: before a device is touched).  daac_last_kernel() says "normalize rules=.. docs=.. bytes=.. out=.. src=..".
 * daac_spans_to_source rewrites n_tokens spans {start, end} that are relative to the normalized document, in place, into spans relative
 *   to the input document, as `tokenizers` reports offsets: start -> src[start]; end -> src[end - 1] plus the length of the input unit
 *   there (the splitter's unit rule, bounded by the document: that is why it takes the input text); an empty span at p -> src[p] twice,
 *   with src at a document's output length read as its input length.  dev_tok_offsets (n + 1): document i's spans are
 *   [tok_offsets[i], tok_offsets[i+1]); (hay, offsets, n, hay_is_device) is the batch daac_normalize_batch was given.  One lane per span.
 * Method: the splitter's mark pass; a workgroup stages a tile of 1024 bytes, 3 in front and 3 behind in LDS, a lane takes four
 *   positions, finds the units that start there and their images' lengths in the table, and the tile's sum is stored; the sums are added
 *   up (one read-back of the total); a second pass ranks the units inside the tile and the lane that owns a unit stores its image.
 *   Integer work only: the result is a function of the input alone. */
typedef enum { DAAC_NORM_DELETE = 1, DAAC_NORM_REPLACE = 2, DAAC_NORM_PAD = 3, DAAC_NORM_HANGUL = 4 } daac_norm_kind;
typedef struct { uint32_t first, last, kind, off, len; } daac_norm_rule;
typedef struct daac_normalizer daac_normalizer;
daac_status daac_normalizer_create(const daac_norm_rule *rules, size_t n_rules, const uint8_t *pool, size_t pool_len, daac_normalizer **out);
void daac_normalizer_free(daac_normalizer *nz);
size_t daac_normalizer_table_bytes(const daac_normalizer *nz);
daac_status daac_normalize_batch(daac_normalizer *nz, const uint8_t *hay, const uint64_t *offsets, size_t n, int hay_is_device, void *stream, int want_src,
                                 uint8_t **dev_out, uint64_t **dev_out_offsets, uint32_t **dev_src, uint64_t *out_len);
/* A single haystack: a batch of one document {0, len}. */
daac_status daac_normalize(daac_normalizer *nz, const uint8_t *hay, size_t len, int hay_is_device, void *stream, int want_src, uint8_t **dev_out,
                           uint32_t **dev_src, uint64_t *out_len);
daac_status daac_spans_to_source(uint64_t *dev_spans, const uint64_t *dev_tok_offsets, const uint64_t *dev_out_offsets, const uint32_t *dev_src, const uint8_t *hay,
                                 const uint64_t *offsets, size_t n, size_t n_tokens, int hay_is_device, void *stream);

/* ---- tokenize_wordpiece: BERT's WordPiece ---------------------------------------------------------------------------------------------------
 * What `tokenizers`' models.WordPiece (and BERT's WordpieceTokenizer) computes for one word of pre-split text: greedy longest-match-first
 * over two piece sets — the pieces a word may begin with and the "##" continuation pieces, which the text never spells out — with a
 * word that cannot be segmented completely, or that is too long, replaced by one unknown token.  It is not daac_tokenize: that call has
 * one piece set and emits a partial segmentation around a gap.  (BERT, DistilBERT, ELECTRA, MPNet, MiniLM and the embedding and reranker
 * models built on them.)  Inputs: a Standard automaton (bytewise or charwise) whose patterns are the pieces without their prefix, a text
 * or a batch whose documents are words, `first_ids` and `cont_ids` (n_ids uint32 each, indexed by match value; host arrays, copied once
 * per call; 0xFFFFFFFF: no such piece), `unk_id`, `max_chars` (1 .. 0xFFFFFFFF; 100 in BERT) and, for the batch, `dev_skip` (NULL, or n
 * bytes in device memory: a document whose byte is non-zero yields no tokens — the whitespace words of a split).  For a document of L
 * bytes:
 *   An empty or skipped document has no tokens.
 *   If the number of bytes b with (b & 0xC0) != 0x80 exceeds max_chars, the result is the one token {unk_id, 0, L}.
 *   Otherwise piece(s, e) is the value of the match (s, e, v) of find_overlapping_iter(doc), s < e; empty matches are not pieces.  Its id
 *     is first_ids[v] when s == 0 and cont_ids[v] otherwise; a piece whose id is 0xFFFFFFFF does not exist in that role.
 *   From p = 0: take the largest e such that piece(p, e) exists in its role, emit {id, p, e}, set p = e, repeat until p == L.
 *   If some p < L has no piece, the whole document is the one token {unk_id, 0, L}.
 * The result does not depend on the order of tuples that share an end: it is a function of the input alone.
 * Results, out-pointers, n_matches and the batch form (dev_tok_offsets, n + 1 u64) are daac_tokenize_bpe's and daac_tokenize_bpe_batch's.
 * Decided before a device is touched, in this order.  Status 1: a NULL pma, dev_ids, n_tokens or n_matches (the batch: dev_tok_offsets
 * too); max_chars == 0; a NULL first_ids or cont_ids; n_ids not above the largest value among daac_pma_outputs; the batch's own offset
 * rules, as in daac_tokenize_batch.  Status 5: a leftmost automaton.  Status 6: a document of 2^32 - 1 bytes or more (positions are kept
 * in 32 bits, as in daac_tokenize_unigram), and the tuple call's own refusals.  Status 2: a token list above max_result_bytes (4 bytes a
 * token, 16 more with spans), answered before it is allocated.  A host text is copied to the device once.
 * Method: one lane per document.  Count pass: the lane clears its L + 1 slots (8 bytes per byte of text), sweeps its tuples once into
 * best[start] = {end, id} — a tuple that exists in the role of its start replaces a shorter one — and walks p -> best[p].end; the number
 * of hops and a one-bit verdict (segmented, or unk_id) are stored.  The counts are summed to tok_offsets and the total (one read-back),
 * and a write pass walks best[] again.  The work of a document is L + its tuples, so there is no cap in the manner of bpe_doc_max.  No
 * atomics, no LDS, integer work only.
 * daac_last_kernel() says "wordpiece docs=.. matches=.. tokens=.." in front of what the tuple call reported. */
daac_status daac_tokenize_wordpiece(daac_pma *pma, int engine, const uint8_t *hay, size_t len, int hay_is_device, void *stream,
                                    const uint32_t *first_ids, const uint32_t *cont_ids, size_t n_ids, uint32_t unk_id, uint32_t max_chars,
                                    uint32_t **dev_ids, uint64_t **dev_spans, uint64_t *n_tokens, uint64_t *n_matches);
daac_status daac_tokenize_wordpiece_batch(daac_pma *pma, int engine, const uint8_t *hay, const uint64_t *offsets, size_t n, int hay_is_device,
                                          void *stream, const uint32_t *first_ids, const uint32_t *cont_ids, size_t n_ids, uint32_t unk_id,
                                          uint32_t max_chars, const uint8_t *dev_skip, uint32_t **dev_ids, uint64_t **dev_spans,
                                          uint64_t **dev_tok_offsets, uint64_t *n_tokens, uint64_t *n_matches);

/* ---- special tokens in raw text: cut a batch around them, splice the tokens back ------------------------------------------------------------
 * What `tokenizers`' AddedVocabulary does with added tokens that are special (`<|endoftext|>`, `[CLS]`, `[MASK]`), and tiktoken with
 * allowed_special: they are found in the raw text, leftmost-longest, in front of the normalizer; each is one token with its own id, and
 * every stretch of text between them is normalized, pre-tokenized and tokenized as a string of its own.  `special` is a leftmost
 * automaton (bytewise or charwise) whose patterns are the special tokens and whose values are their ids; the handle's own leftmost kind
 * decides among candidates (LeftmostLongest is what `tokenizers` uses).
 * daac_cut_batch.  For document i = hay[offsets[i], offsets[i+1]) take m_0 .. m_{k-1}, the tuples of leftmost_find_iter on that document
 *   alone, as daac_scan_batch_device16 with DAAC_LEFTMOST_FIND gives them: ascending, disjoint, none across a document boundary.  The
 *   document is partitioned into the *special* segments [start(m_j), end(m_j)) with the value value(m_j), and the non-empty stretches
 *   between them, in front of the first and behind the last: the *text* segments, with the value 0xFFFFFFFF.  There are no empty
 *   segments: an empty document has none, a document without a match is one text segment, two adjacent specials have nothing between
 *   them.  *dev_seg_offsets holds *n_segs + 1 u64 positions in hay — absolute, entry 0 is offsets[0], the last entry is offsets[n], so
 *   (hay, seg_offsets) is a batch that every *_batch call accepts; *dev_doc_segs holds n + 1 u64: document i's segments are
 *   [doc_segs[i], doc_segs[i+1]); *dev_seg_values holds *n_segs u32 (NULL when there is no segment).  *n_special is the number of
 *   matches.  All three are device memory, released with daac_device_free.  The call returns after the stream has finished.  n = 0: one
 *   offset and one doc_segs entry, both 0, and a NULL values pointer.
 *   Decided before a device is touched, in this order.  Status 1: a NULL special or out-pointer; the batch offset rules of
 *   daac_scan_count_batch (host offsets; device offsets are validated by the tuple call, with one read-back).  Status 5: a Standard
 *   automaton.  Status 1: an automaton with "" among its patterns (a record of length 0 among daac_pma_outputs: it cannot be a
 *   segment), then one with the value 0xFFFFFFFF.  Status 2: a doc_segs above option max_result_bytes (8 bytes a document); the segment
 *   list likewise (8 bytes a segment), answered before it is allocated.  The tuple list is daac_scan_batch_device16's: its engines and
 *   their refusals (6) and the max_result_bytes rule of the list are this call's.  A host haystack is copied to the device once.
 *   daac_last_kernel() says "cut docs=.. matches=.. segs=.." in front of what the tuple call reported.
 *   Method: one lane per item.  The items are, in document order, every document and behind it its matches: document i's item is
 *   i + doc_match_offsets[i], its j-th match's one more plus j; an item finds its document by binary search over that, so a document
 *   that is nothing but ten thousand specials costs what ten thousand documents with one special cost.  A document's item contributes
 *   1 segment when text stands in front of its first match, or when it has no match and is not empty; a match's item 1 for itself and 1
 *   more when text follows it.  The counts are summed (one read-back of the total) and a second pass writes each item's segment starts
 *   and values at its rank; doc_segs[i] is the rank of document i's item.  Integer work only, no atomics: the result is a function of
 *   the input alone.  Scratch: 8 bytes an item.
 * daac_tokens_splice.  dev_ids (and dev_spans: {start, end} relative to the segment's first byte; NULL: not wanted) are what some
 *   tokenizer produced over the segment batch, dev_seg_tok its n_segs + 1 token offsets per segment; dev_seg_values, dev_seg_offsets
 *   and dev_doc_segs are daac_cut_batch's, dev_doc_offsets (n_docs + 1) the offsets that call was given, all in device memory.  A text
 *   segment's tokens are copied; a special segment contributes exactly one token, whatever the tokenizer made of its bytes: its id is
 *   its value and its span is the segment.  Output spans are relative to the document's first byte: a text token's span plus
 *   seg_offsets[s] - doc_offsets[doc].  *dev_out_ids (*n_tokens u32; NULL when there are none), *dev_out_spans (*n_tokens pairs; a NULL
 *   dev_out_spans: not wanted, and neither with a NULL dev_spans unless the segment batch has no token) and *dev_doc_tok (n_docs + 1 u64 token offsets per document) are device
 *   memory, released with daac_device_free.  The call looks at CSR offsets only, so it serves daac_tokenize_batch, _unigram_batch,
 *   _bpe_batch and _wordpiece_batch alike.  Returns after the stream has finished.
 *   Status 1: a NULL argument other than dev_spans, dev_out_spans, dev_seg_values with n_segs = 0 and dev_ids when the segment batch has
 *   no token; n_segs > 0 with n_docs = 0.  Status 2: a result above the process-wide option max_result_bytes (8 bytes a document; 4
 *   bytes a token, 16 more with spans), answered before it is allocated.  daac_last_kernel() says "splice docs=.. segs=.. tokens=..".
 *   Method: one lane per segment counts its output tokens (seg_tok[s+1] - seg_tok[s], or 1); the counts are summed (one read-back of
 *   the total); a wave takes a segment and its lanes the segment's tokens, so a long text segment is not one lane's work; a segment
 *   finds its document by binary search in doc_segs; doc_tok is the new segment offsets composed with doc_segs (daac_offsets_compose's
 *   kernel).  Scratch: 8 bytes a segment. */
daac_status daac_cut_batch(daac_pma *special, int engine, const uint8_t *hay, const uint64_t *offsets, size_t n, int hay_is_device, void *stream,
                           uint64_t **dev_seg_offsets, uint64_t **dev_doc_segs, uint32_t **dev_seg_values,
                           uint64_t *n_segs, uint64_t *n_special);
daac_status daac_tokens_splice(const uint32_t *dev_ids, const uint64_t *dev_spans, const uint64_t *dev_seg_tok,
                               const uint32_t *dev_seg_values, const uint64_t *dev_seg_offsets, const uint64_t *dev_doc_segs,
                               const uint64_t *dev_doc_offsets, size_t n_segs, size_t n_docs, void *stream,
                               uint32_t **dev_out_ids, uint64_t **dev_out_spans, uint64_t **dev_doc_tok, uint64_t *n_tokens);

/* ---- model inputs: template, truncation and padding ------------------------------------------------------------------------------------------
 * What `tokenizers` calls the post-processor (TemplateProcessing) plus enable_truncation and enable_padding: the last step between a
 * token result and the tensors a model reads.
 * daac_tokens_pack.  Sequence A is a CSR token result of n documents as every token call leaves it in device memory: dev_a_ids
 *   (a_tokens u32), dev_a_spans (a_tokens pairs of u64 relative to the document, or NULL) and dev_a_offsets (n + 1 u64).  Sequence B,
 *   of the same n, is optional: with dev_b_offsets the whole batch is pairs, with NULL it is all singles.
 *   Template.  params->single (n_single pieces) serves singles, params->pair (n_pair) pairs; a template has at most
 *   DAAC_PACK_MAX_PIECES pieces {kind, id, type_id}.  DAAC_PACK_A occurs exactly once in each, DAAC_PACK_B exactly once in pair and
 *   never in single; a DAAC_PACK_SPECIAL piece is one token.  n_added is the number of special pieces of the template in use.  n_pair
 *   may be 0 when no B is given.
 *   Truncation (params->truncate != 0) runs before the template, as in `tokenizers`, on budget = max_length - n_added.  With budget 0
 *   both sequences keep 0 tokens, whatever the strategy.  A single of n1 tokens keeps min(n1, budget).  A pair with n1 + n2 <= budget
 *   keeps all; otherwise, with need = n1 + n2 - budget: DAAC_TRUNC_LONGEST_FIRST takes the two lengths as a <= b (swapped if n1 > n2),
 *   sets b = a if a > budget, else b = max(a, budget - a), then, if a + b > budget, a = budget / 2 and b = a + budget % 2, and swaps
 *   back; DAAC_TRUNC_ONLY_FIRST keeps n1 - need of A and all of B, and the document is in error when n1 - need <= 0;
 *   DAAC_TRUNC_ONLY_SECOND is the same on B.  truncate_left = 0 keeps a sequence's first tokens, 1 its last.
 *   Rows.  A row is the template walked in order: a special piece gives (id, type_id, special 1, attention 1, span (0, 0)), a sequence
 *   piece its kept tokens as (id, the piece's type_id, 0, 1, the token's span); a B token's span is relative to document B.
 *   Padding.  DAAC_PAD_LONGEST, or DAAC_PAD_FIXED with pad_length: L = the longest row, or max(pad_length, longest row), rounded up to
 *   pad_multiple (1: none).  A padding slot is (pad_id, pad_type_id, special 1, attention 0, span (0, 0)), to the right of the row or,
 *   with pad_left = 1, to its left.  The result is dense: *dev_input_ids, *dev_token_type_ids, *dev_attention_mask and
 *   *dev_special_tokens_mask are [n, L] planes of params->width bytes an element (4: int32, 8: int64; an id is zero-extended),
 *   *dev_offsets is [n, L, 2] u64; *row_length = L, *n_slots = n * L.  DAAC_PAD_NONE: the result is CSR, the cu_seqlens form of
 *   variable-length attention: the same planes as flat [R] arrays, no attention mask (*dev_attention_mask = NULL), and
 *   *dev_row_offsets holds n + 1 u64; *row_length = the longest row, *n_slots = R.  Every plane but dev_input_ids may be NULL as an
 *   argument: not wanted.  dev_row_offsets is written in the CSR form only (otherwise *dev_row_offsets = NULL).  A plane of no element
 *   is NULL.  All are device memory, released with daac_device_free.  n = 0: NULL planes, L = 0 and, in the CSR form, one 0 in
 *   row_offsets.  The call is ordered on `stream` and returns after it has finished.
 *   Deliberate differences from `tokenizers`: max_length < n_added is status 1 (`tokenizers` silently does not truncate);
 *   DAAC_PAD_FIXED with a longer row widens L (`tokenizers` returns a ragged batch); stride and overflowing pieces, word_ids and
 *   sequence ids, special pieces of several ids and batches that mix singles and pairs are out of scope.
 *   Decided before a device is touched, in this order, all status 1: a NULL params, dev_input_ids, row_length or n_slots, a NULL
 *   dev_a_offsets with n > 0, a NULL ids list with tokens; a struct_size other than sizeof(daac_pack_params); a template that breaks
 *   the rules above (a pair batch without a pair template included); a width other than 4 or 8; a strategy or padding outside its
 *   enum, or a pad_multiple of 0; DAAC_TRUNC_ONLY_SECOND without B; max_length < n_added; the CSR form without dev_row_offsets;
 *   dev_offsets without the spans of a sequence that has tokens.  Then status 2: row_offsets above the process-wide option
 *   max_result_bytes (8 bytes a document).
 *   After the header pass, one read-back: a document whose offsets decrease or leave [0, tokens] answers 1, and so does the first
 *   document that ONLY_FIRST / ONLY_SECOND cannot truncate ("document <i>: ..."); nothing is handed over and every out-pointer stays
 *   NULL.  A result above max_result_bytes (width bytes a slot and wanted plane, 16 more with offsets) answers 2 before it is
 *   allocated.  daac_last_kernel() says "pack docs=.. pair=.. row=.. tokens=.. dropped=..".
 *   Method: one lane per document writes a row header (what A and B keep and where) and folds the longest row, the first document in
 *   error, the slots and the dropped tokens into four words, a wave reduction and one atomic per wave; CSR: the rows' lengths are
 *   summed to row_offsets; one lane per output slot of the flat n * L (or R) index space finds its row and column, its source —
 *   padding, a template piece, a token of A or B — and stores that slot of every plane: 64 consecutive elements per wave, no atomics.
 *   Scratch: 32 bytes a document. */
typedef enum { DAAC_PACK_SPECIAL = 0, DAAC_PACK_A = 1, DAAC_PACK_B = 2 } daac_pack_piece_kind;
typedef enum { DAAC_TRUNC_LONGEST_FIRST = 0, DAAC_TRUNC_ONLY_FIRST = 1, DAAC_TRUNC_ONLY_SECOND = 2 } daac_pack_strategy;
typedef enum { DAAC_PAD_NONE = 0, DAAC_PAD_LONGEST = 1, DAAC_PAD_FIXED = 2 } daac_pack_padding;
#define DAAC_PACK_MAX_PIECES 16
typedef struct {
    uint32_t kind;      /* daac_pack_piece_kind */
    uint32_t id;        /* DAAC_PACK_SPECIAL: the token */
    uint32_t type_id;
} daac_pack_piece;
typedef struct {
    uint32_t struct_size;   /* sizeof(daac_pack_params) */
    uint32_t n_single, n_pair;
    daac_pack_piece single[DAAC_PACK_MAX_PIECES], pair[DAAC_PACK_MAX_PIECES];
    uint32_t truncate;      /* 0: no truncation (strategy, truncate_left and max_length are not read) */
    uint32_t strategy;      /* daac_pack_strategy */
    uint32_t truncate_left;
    uint32_t padding;       /* daac_pack_padding */
    uint32_t pad_left;
    uint32_t pad_id, pad_type_id;
    uint32_t width;         /* 4 or 8 */
    uint64_t max_length;
    uint64_t pad_length;    /* DAAC_PAD_FIXED */
    uint64_t pad_multiple;  /* 1: none */
} daac_pack_params;
daac_status daac_tokens_pack(const daac_pack_params *params, const uint32_t *dev_a_ids, const uint64_t *dev_a_spans, const uint64_t *dev_a_offsets,
                             uint64_t a_tokens, const uint32_t *dev_b_ids, const uint64_t *dev_b_spans, const uint64_t *dev_b_offsets,
                             uint64_t b_tokens, size_t n, void *stream, void **dev_input_ids, void **dev_token_type_ids,
                             void **dev_attention_mask, void **dev_special_tokens_mask, uint64_t **dev_offsets, uint64_t **dev_row_offsets,
                             uint64_t *row_length, uint64_t *n_slots);

/* ---- token ids back to text -------------------------------------------------------------------------------------------------------------
 * What `tokenizers` calls the decoder, and the other direction of every token call above.
 * A decoder is a table over the ids 0 .. n_ids - 1.  Each id has an image rest (any bytes, possibly none), an image first, used when the
 *   token is the first KEPT token of its document, and flags: DAAC_DECODE_SPECIAL, and DAAC_DECODE_ABSENT for an id that has no entry
 *   (its images are not read).  Every id from n_ids on has no entry either.
 * Definition.  A document's tokens t_0 .. t_{m-1} decode as follows.  A token is kept unless skip_special is set and its id is special,
 *   or its id has no entry and unknown_skip is set (without unknown_skip such a token is an error).  The document's text is
 *   first[k_0] + rest[k_1] + rest[k_2] + ... over the kept tokens in order.  The result is bytes: nothing is validated or replaced as
 *   UTF-8.  This one rule covers `tokenizers`' ByteLevel, WordPiece (cleanup included: it is applied per token) and Metaspace /
 *   ByteFallback decoders, each of which is a function of the token and of whether it is the first after the specials are filtered; the
 *   Python package's Decoder.byte_level / .wordpiece / .metaspace build their tables.
 * daac_decoder_create copies the table: `pool` (pool_bytes, below 4 GiB) holds the images' bytes and pieces[id] = {off, len, first_off,
 *   first_len} says where rest and first lie in it; flags[id] is a byte.  Status 1: a NULL out, a NULL pool, pieces or flags with
 *   elements to read, a pool of 4 GiB or more, more than 2^32 ids, a flag bit other than the two, an image that leaves the pool.  The
 *   table goes to a device the first time a call runs there; daac_decoder_free releases it everywhere.
 * daac_tokens_decode.  The tokens are in device memory, in one of two forms.  CSR (dev_offsets != NULL): dev_ids holds n_tokens u32
 *   (id_width 4) and dev_offsets n + 1 u64 token offsets, as every token call leaves them; tokens in front of dev_offsets[0] or behind
 *   dev_offsets[n] belong to no document and are not looked at.  Dense (dev_offsets == NULL): dev_ids is an [n, row_length] plane of
 *   id_width-byte elements (4: int32 / uint32, 8: int64), daac_tokens_pack's planes or a model's output; row d is tokens d * row_length
 *   .. d * row_length + row_length - 1, n_tokens is not read, and an 8-byte element outside [0, 2^32), -100 for instance, is an id
 *   without an entry.  Padding is just a special id.
 *   Result, in device memory, released with daac_device_free: *dev_out, *out_bytes bytes of text (never NULL when n > 0: a text of no
 *   byte is a granule nobody reads); *dev_out_offsets, n + 1 u64 from 0, document d's text is [out_offsets[d], out_offsets[d + 1]) — a
 *   batch again, as every batch call takes it; and, where dev_token_starts is not NULL, *dev_token_starts: n_tokens + 1 (dense: n *
 *   row_length + 1) u64, the position in the text at which each token's image begins, the total as the closing entry (a token that is
 *   not kept has the position of the next one).  n = 0: one 0 in out_offsets and no other buffer.  The call is ordered on `stream` and
 *   returns after it has finished.
 *   Deliberate differences from `tokenizers`: the result is raw bytes, as tiktoken's decode_bytes (`tokenizers` turns ill-formed UTF-8
 *   into U+FFFD); an id without an entry is an error unless unknown_skip is set (`tokenizers` drops it silently: unknown_skip);
 *   `transformers`' clean_up_tokenization_spaces over the joined string, and incremental decoding that keeps state between calls, are out
 *   of scope.
 *   Decided before a device is touched, in this order: status 1 for a NULL dec, dev_out, dev_out_offsets or out_bytes, or a NULL
 *   dev_ids with tokens to read; an id_width other than 4 or 8, or 8 with dev_offsets; neither dev_offsets nor a row_length while n > 0;
 *   then status 2 where out_offsets (8 bytes a document), a dense plane's token count (8 bytes a token of scratch) or token_starts (8
 *   bytes a token) exceed the process-wide option max_result_bytes.  A call refused so far leaves its out-pointers as given.
 *   After the sizing pass, one read-back: the first document whose offsets decrease or leave [0, n_tokens] answers 1 ("document <d>:
 *   ..."), then the lowest token whose id has no entry ("document <d>, token <i>: ...", i the flat index), then a text above
 *   max_result_bytes answers 2 before it is allocated; nothing is handed over and every out-pointer is NULL.
 *   daac_last_kernel() says "decode docs=.. tokens=.. kept=.. bytes=..".
 *   Method: one lane per token writes the length of its rest image (0 if it is not kept) and folds the lowest token without an entry
 *   (a max over the complement) and the kept tokens, a wave reduction and one atomic per wave on scratch; one lane per document checks
 *   its offsets, walks to its first kept token and overrides that token's length with its first image's (a document of nothing but
 *   skipped tokens costs its lane one read per token); an exclusive sum gives every token's start; the copy is output-parallel: a
 *   workgroup owns 4 KiB of text, a lane 16 bytes and one aligned 16-byte store, the tile's token starts are staged in LDS (up to 4096
 *   of them; a tile of more, which takes empty images, searches them in HBM), and a lane finds the token of its first byte as the largest i with start[i] <= q,
 *   which steps over empty images, and gathers its bytes from the pool.  Positions are 64-bit, no pass uses atomics on the output.
 *   Scratch: 9 bytes a token (1 with token_starts, which are the starts themselves) and 8 bytes per 4 KiB of text. */
#define DAAC_DECODE_SPECIAL 1u
#define DAAC_DECODE_ABSENT 2u
typedef struct {
    uint32_t off, len;               /* rest = pool[off, off + len) */
    uint32_t first_off, first_len;   /* first = pool[first_off, first_off + first_len) */
} daac_decode_piece;
typedef struct daac_decoder daac_decoder;
daac_status daac_decoder_create(const uint8_t *pool, uint64_t pool_bytes, const daac_decode_piece *pieces, const uint8_t *flags, uint64_t n_ids,
                                daac_decoder **out);
void daac_decoder_free(daac_decoder *dec);
daac_status daac_tokens_decode(daac_decoder *dec, const void *dev_ids, uint32_t id_width, const uint64_t *dev_offsets, uint64_t n_tokens, size_t n,
                               uint64_t row_length, int skip_special, int unknown_skip, void *stream, uint8_t **dev_out, uint64_t **dev_out_offsets,
                               uint64_t **dev_token_starts, uint64_t *out_bytes);

/* The same over the tail of a haystack: counts the matches with end in (begin, len] — what one
 * shard of a haystack split across devices contributes.  Bytes before begin - Lmax are never read (they need
 * not be resident), byte 0 of the haystack is still `hay`.  For the overlapping modes any `begin` works (charwise:
 * also inside a character).  DAAC_FIND / DAAC_LEFTMOST_FIND are chains through their own matches: there `begin`
 * must be a position where the iterator restarts (0, or the end of a match it reported), and the call reports
 * what the iterator reports from there on.  These two modes settle the chain before counting and synchronise
 * the stream even when `result_dev` is given. */
daac_status daac_scan_count_range(daac_pma *pma, int mode, int engine, const uint8_t *hay, size_t len, size_t begin,
                                  int hay_is_device, void *stream, uint64_t *count, uint64_t *checksum,
                                  uint64_t *result_dev);

/* Lazy façade = Iterator::next() (iter.rs:58, 133, 195, 272): scans the haystack window by
 * window on the device and hands tuples out one at a time.  The haystack must stay alive until
 * close (the Rust iterator owns/borrows `P` the same way). */
daac_status daac_iter_open(daac_pma *pma, int mode, int engine, const uint8_t *hay, size_t len,
                           int hay_is_device, void *stream, daac_iter **out);
int daac_iter_next(daac_iter *it, daac_match *m); /* 1 = Some(m), 0 = None, <0 = -daac_status */
/* The same stream, a run at a time and without a copy: `*batch` points at the next `*n` >= 1 matches in the iterator's own
 * (page-locked) window buffer, as the crate keeps a Match (lib.rs:287-291: end, length, value); valid until the next call on this
 * iterator.  1 = a run, 0 = exhausted, <0 = -daac_status.  May be mixed with daac_iter_next (both advance the same position).
 * Behind both: a worker thread scans the windows (option iter_window, 64 MiB) ahead of the consumer with three stages in flight
 * on their own streams — host-to-device copy of window k + 1, scan of window k, device-to-host copy of window k - 1's 16-byte tuples. */
int daac_iter_next_batch(daac_iter *it, const daac_match16 **batch, size_t *n);
/* The compact form of the same iterator.  On match-dense text `next()` is bound by the tuples' way back over PCIe (cfg3: 10 GB of
 * 16-byte tuples per GiB of haystack at the link's ~50 GB/s), so an iterator opened with daac_iter_open_compact sends 8 bytes per tuple:
 * the value, and one word that holds the end relative to the window's first byte in its low `end_bits` bits and the length above them
 * (end_bits = 32 - the bits of the longest pattern's length; windows are kept below 2^end_bits bytes).  daac_iter_next_batch8 hands out
 * runs of them:  end = *end_base + (t.end_len & ((1 << *end_bits) - 1)),  length = t.end_len >> *end_bits,  start = end - length.
 * daac_iter_next works on either kind; daac_iter_next_batch only on the 16-byte kind and daac_iter_next_batch8 only on the compact one
 * (status 6 otherwise); daac_iter_open_compact itself answers 6 for dictionaries with patterns of several KB (no room for a window). */
typedef struct daac_match8 {
    uint32_t value;
    uint32_t end_len;
} daac_match8;
daac_status daac_iter_open_compact(daac_pma *pma, int mode, int engine, const uint8_t *hay, size_t len,
                                   int hay_is_device, void *stream, daac_iter **out);
int daac_iter_next_batch8(daac_iter *it, const daac_match8 **batch, size_t *n, uint64_t *end_base, uint32_t *end_bits);
void daac_iter_close(daac_iter *it);

/* Chunk-fed steppers = FindOverlappingStepper / FindStepper (bytewise/iter.rs:344-475, charwise/iter.rs:403-534)
 * and the *_from_iter entry points (bytewise.rs:238-251, 353-375) for haystacks that arrive piecewise: feed the
 * text chunk by chunk (any sizes, cuts may fall inside UTF-8 characters); every call returns the matches it can
 * already decide — for the overlapping modes everything ending inside the chunk, for DAAC_FIND the chain up to
 * the end of the data — in stream coordinates, so that the concatenation over all calls is exactly what the
 * iterator reports on the concatenated text.  The library keeps at most max-pattern-length bytes (DAAC_FIND: the
 * undecided tail) of earlier chunks on the device.  Modes: DAAC_FIND_OVERLAPPING, DAAC_FIND,
 * DAAC_FIND_OVERLAPPING_NO_SUFFIX (the reference has no leftmost stepper: a leftmost match needs lookahead). */
typedef struct daac_stream daac_stream;
daac_status daac_stream_open(daac_pma *pma, int mode, int engine, void *stream, daac_stream **out);
daac_status daac_stream_feed(daac_stream *s, const uint8_t *chunk, size_t len, int chunk_is_device, daac_matches **out);
/* The same feed with the matches as 8-byte tuples (ABI 6; the form daac_iter_next_batch8 hands out): `*batch` points at `*n` tuples in a
 * page-locked block of the stream object, valid until the next feed or close;  end = *end_base + (t.end_len & ((1 << *end_bits) - 1)),
 * length = t.end_len >> *end_bits.  A third of daac_match's bytes over PCIe and nothing to allocate or free per feed.  A chunk (plus the
 * bytes kept of earlier ones) must stay below 2^end_bits bytes (end_bits = 32 - the bits of the longest pattern's length): status 6 otherwise. */
daac_status daac_stream_feed_compact(daac_stream *s, const uint8_t *chunk, size_t len, int chunk_is_device, const daac_match8 **batch,
                                     size_t *n, uint64_t *end_base, uint32_t *end_bits);
void daac_stream_close(daac_stream *s);

/* ---- tuning knobs (optional) ----------------------------------------------------------------- */
/* Process-wide name/value pairs for experiments; defaults in parentheses.  Options that shape the device tables
 * ("lds_budget", "dense_depth", "rows_share_pct", "gram_lds_budget", "gram_rank_in_lds", "char_map_lds") are read
 * when an automaton is uploaded, the others at every scan.
 *   seg_bytes (0 = auto)        bytes of haystack per lane-segment of the segment scanners
 *   threads (1024), blocks_per_cu (0 = auto)   launch shape of the overlapping scanners
 *   lds_budget (98304), dense_depth (-1 = auto), rows_share_pct (45)   TIERED re-pack, read at upload:
 *                               lds_budget     bytes of LDS the tables may take per workgroup, 0 .. 163840 (what a workgroup can have: every
 *                                              accepted budget gives tables the segment, histogram and batch kernels can be launched with;
 *                                              one too small for ROOT's row leaves the automaton without the TIERED engine)
 *                               dense_depth    states up to this depth get a dense, fail-resolved row (0 = ROOT alone); -1 = the deepest level
 *                                              whose rows fit rows_share_pct of the budget (the whole automaton where all of it fits); a depth
 *                                              whose rows do not fit the budget leaves the automaton without the TIERED engine
 *                               rows_share_pct 0 .. 100
 *                               a value outside these ranges (a negative budget, dense_depth < -1): status 1
 *   gram_lds_budget (161792), gram_region (0 = auto: 16384 for the first table set, 65536 for the second and PFX, 262144 from 2 GiB on; rounded down to a power of two >= 2048), gram_slab (4096), gram_region_small (0 = auto: 32768; gram4: bytes of the small regions the haystack's end is cut into, a power of two <= gram_region), gram_taper_split (-1 = auto; gram4: the byte the small regions begin at, rounded down to a whole region; past the end: none; expert knobs for tests and timing runs: a split in front of the launch's first whole round of large regions makes every wave claim at the start of the scan, and that many adds to one counter at once queue for tens of microseconds), gram_dense (-1 = auto), gram_rank_in_lds (-1 = auto),
 *   gram_ppl (0 = auto: 32 positions per lane and step for automata without short patterns, else 16)
 *   gram_version (0 = auto: `.count()` on the gram4 kernel over the renumbered second table set, count + checksum on the first where it applies;
 *                 1 = first table set only, 2 = gram2 kernels only, 4 (3: its name in ABI 4) = gram4 for `.count()` or an error), gram2_dpp (1: DPP wave shifts),
 *   gram2_rfull (1)             rank directory with one entry per M word when LDS allows (0: one per four words)
 *   gram_tail (alias gram3_tail; -1 = every workgroup samples its text and picks; 0 / 1: the plain / the tail-record body of the gram4 kernel),
 *   gram4_arith (1: byte classes by arithmetic where the dictionary's bytes are one range; 0: the class table in LDS)
 *   gram4_filter (1)            the gram4 kernel's LDS filter in front of rank + gather (gram4_filter.hpp, ABI 6): a hit asks the L2 for its record
 *                               only if a Bloom word says the state may end a pattern or go on; workgroups whose text is made of dictionary
 *                               words keep the per-word directory and the tail-record body.  0: round 5's bodies
 *   gram4_mph (8; read at upload)  a hit that passes that filter finds its record by a perfect hash of its K+1 bytes (gram4_mph.hpp) instead of by its
 *                               rank: seeds the table builder may try; a dictionary too dense for a displacement table the size of its coarse rank
 *                               directory keeps the rank path (daac_last_kernel() says mph=0).  0: records by rank
 *   find3 (1)                   find_iter's count (+ checksum) by selection over the tuple emitter's per-position flags (find3_kernels.hip;
 *                               Standard bytewise dictionaries with K = 3 tables and no pattern beyond 19 bytes) instead of the chain walkers,
 *                               in windows of find3_window (2^30) end positions, each restarting at the last match of the one before; a handle
 *                               whose last such request met text made of dictionary words goes back to the walkers (2: never), 0: off
 *   left3 (1)                   leftmost_find_iter's count (+ checksum) likewise (left3_kernels.hip): at upload a leftmost handle's patterns are
 *                               read back from its trie and built into a Standard automaton whose detection tables the selection — by match
 *                               STARTS — runs on; same conditions, same windows, same fallback as find3 (2: whatever the text, 0: off — set
 *                               before the upload to save the second build)
 *   select_emit (1)             the tuple LIST of find_iter / leftmost_find_iter (daac_scan, daac_scan_device[16], the lazy iterator's windows) from
 *                               those selection kernels' emitting form, where find3 / left3 apply; 0: the chain walkers' speculate / reconcile / emit
 *   workspace_keep (8 GiB)      bytes of scratch (annotated stream, record list: ~2 per haystack byte) a handle keeps between its tuple-emitter
 *                               and find3 calls instead of asking the pool every time (tools/micro/pool_ops.hip); 0: none
 *   pfx_probe (16384)           AUTO, count (+ checksum) of a dictionary PFX serves: a synchronous scan of a device haystack >= 32 MiB samples
 *                               65 536 positions; where more than this many survive PFX's filter the micro-step walker over the double array
 *                               takes the scan (the verdict stays in the handle for the asynchronous calls); 0 = never ask, always PFX
 *   pfx (1)                     PFX tables (any byte alphabet): 1 = built where no GRAM table set applies, 2 = for every automaton they can
 *                               serve (DAAC_ENGINE_PFX then selects them explicitly), 0 = never; read at upload
 *   emit (1)                    materialising overlapping scans through the tuple emitter (emit3_kernels.hip: detection once, then expansion;
 *                               GRAM tables, or PFX's for any byte alphabet) where it applies (0: segment scanners);
 *   emit_rec_per_kib (32)       deep-match records per KiB of haystack the record list is first sized for (a handle remembers what its
 *                               last scan met; a list that proves too short is sized exactly and the detection is rerun once)
 *   restart_chain (1)           find_iter / leftmost_find_iter as speculate-reconcile-emit chains (0: sync-point scanners)
 *   chain_rounds (24)           reconciliation rounds before falling back to the sync-point scanners
 *   restart_bpc (8)             256-lane workgroups per CU of the chain walkers (they are bound by VALU issue at full occupancy)
 *   char_map_lds (1)            charwise walkers: ASCII and the populated stretch of the code mapper staged in LDS when they fit 32 KB
 *   char_row_lds (1)            ... and ROOT's row of children beside it when both fit 80 KB (read at upload)
 *   overlap_micro (1)           count (+ checksum) of overlapping scans the GRAM tables do not serve: 1 = the micro-step walker for
 *                               charwise automata and the double array, 2 = also in place of the TIERED engine, 0 = the segment scanners
 *   pool (1), pool_keep (0)     scratch and result buffers from the device's stream-ordered pool, which keeps up to pool_keep bytes
 *                               between calls (0 = 1/8 of the device memory, at most 32 GiB); read at the first scan of the process
 *   iter_window (64 MiB)        haystack bytes per window of the lazy iterator (the first windows are 16 and 32 MiB: matches arrive early)
 *   max_result_bytes (8 GiB)    largest match list daac_scan may materialise
 *   batch_piece (4096)          batches, find_overlapping modes: bytes of a document one lane scans (a piece; entered up to the halo early)
 *   batch_lane_max (16384)      batches, find_iter / leftmost_find_iter: longest document one lane walks; longer ones take the single-haystack path
 *   bpe_doc_max (4096)          daac_tokenize_bpe[_batch]: the longest document, in bytes, the merge loop takes (its work on one lane grows with
 *                               the square of the length); 1 .. 65536, any other value: status 1; a longer document answers 6
 *   batch_hist_wave_max (2048)  per-document pattern counts: most match records of a document that one wave sorts in LDS (clamped to 4096)
 *   batch_hist_sort_max (16384) ... and that one workgroup sorts (clamped to 32768, what 160 KB of LDS hold); documents with more take a row
 *                               of outputs_len counters in HBM.  Neither is read at upload; negative values are status 1.  The defaults are
 *                               the winners of tools/time_batch_hist.py's sweep (profiles/r12_batch_hist_time.json)
 *   hist_lds_bins (16384)       histograms: the first slots (the shortest patterns: slots are in BFS order of the trie) a workgroup counts in LDS
 *                               before it flushes them to the global counters; clamped to what 160 KB minus the engine's tables hold; 0 = all
 *                               hits go to global atomics (13 to 27 times slower on the cfg3 dictionary); negative: status 1.  The default is the
 *                               winner of tools/time_hist.py's sweep on TIERED and DARRAY (profiles/r11_hist_time.json)
 *   debug_fill (-1)             tests: 0 .. 255 = every scratch, staging and result buffer the library allocates (the pool's blocks, a handle's
 *                               kept workspace, the staging copies of host text, the iterators' and steppers' buffers) is set to that byte
 *                               when it is handed out, on the call's stream, in front of the call's own clears and copies; -1 = off (the
 *                               contents are undefined, as always); any other value: status 1.  Results never depend on it (DESIGN.md 4.24;
 *                               tests/test_gpu_uninitialised.py).  Not read at upload; process-wide only */
daac_status daac_set_option(const char *name, int64_t value);
/* The same option for ONE handle (ABI 5): overrides the process-wide value for every scan, iterator and stream of `pma`, whichever thread runs
 * them (the worker threads of the lazy iterator and of daac_scan_count_multi included).  Two threads scanning two handles with different
 * settings do not share state.  unset != 0 removes the override.  The options read when the tables are laid out (lds_budget, dense_depth,
 * rows_share_pct, gram_lds_budget, gram_rank_in_lds, pfx, char_map_lds, char_row_lds) are set BEFORE the handle's first upload: on a handle
 * that already has tables on a device they could not take effect, and the call says so (status 6, ABI 6) instead of answering OK.
 * `pool` / `pool_keep` / `debug_fill` belong to the device's allocator, not to a handle (status 1). */
daac_status daac_pma_set_option(daac_pma *pma, const char *name, int64_t value, int unset);

#ifdef __cplusplus
}
#endif
#endif
