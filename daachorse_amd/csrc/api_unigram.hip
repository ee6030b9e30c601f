// C ABI (include/daachorse_amd.h), part 10: the best-scoring segmentation of a text or a batch on the device (daac_tokenize_unigram,
// daac_tokenize_unigram_batch).  The piece lattice is the tuple CSR of daac_scan_batch_device16(DAAC_FIND_OVERLAPPING): its engines,
// refusals and max_result_bytes rule are this call's; the kernels are unigram_kernels.hip.  This file validates its own arguments,
// copies the scores, runs the forward and count passes, sums the counts (one read-back), allocates the result and runs the write pass.
// The batch arguments' rules, the staging of a host text, the length check of device offsets and the single haystack as a batch of one
// document are the batch front door's (api_internal.hpp, "api_batch.hip").
#include <cmath>

#include "api_internal.hpp"
#include "unigram.hpp"

namespace {

// |score| <= kUniMaxScore: a path has fewer than 2^32 edges (a document of 2^32 - 1 bytes or more is refused), so no sum of them exceeds
// 2^32 * 1e20 < 4.3e29 in magnitude and rounding cannot lift it to float32's 3.4e38: best[] never overflows to an infinity.
constexpr float kUniMaxScore = 1e20f;
constexpr uint64_t kUniMaxDoc = 0xFFFFFFFFull;   // bytes of a document: an edge's length is kept in 32 bits

bool score_ok(float s) { return std::isfinite(s) && std::fabs(s) <= kUniMaxScore; }

// Status 1, then status 5, before a device is touched.
daac_status unigram_precheck(const daac_pma *pma, const float *scores, size_t n_scores, float unk_score, int gap, uint32_t gap_id, bool outs_ok) {
    if (!pma || !outs_ok) { set_error("null argument"); return DAAC_ERR_INVALID_ARGUMENT; }
    if (gap != DAAC_GAP_BYTES && gap != DAAC_GAP_CHARS) { set_error("gap is neither DAAC_GAP_BYTES nor DAAC_GAP_CHARS: the unknown edges must reach the text's end"); return DAAC_ERR_INVALID_ARGUMENT; }
    if (gap == DAAC_GAP_BYTES && gap_id > 0xFFFFFFFFu - 255u) { set_error("DAAC_GAP_BYTES: gap_id + 255 does not fit 32 bits"); return DAAC_ERR_INVALID_ARGUMENT; }
    const std::vector<daac::OutputRec> &outs = pma->charwise ? pma->chost.outputs : pma->host.outputs;
    uint64_t need = 0;   // the largest value + 1
    for (const daac::OutputRec &o : outs) need = std::max<uint64_t>(need, static_cast<uint64_t>(o.value) + 1);
    if (n_scores < need) { set_error("n_scores = " + std::to_string(n_scores) + " does not cover the largest match value, " + std::to_string(need - 1)); return DAAC_ERR_INVALID_ARGUMENT; }
    if (n_scores && !scores) { set_error("scores is NULL"); return DAAC_ERR_INVALID_ARGUMENT; }
    if (!score_ok(unk_score)) { set_error("unk_score is NaN, infinite or above 1e20 in magnitude"); return DAAC_ERR_INVALID_ARGUMENT; }
    for (size_t i = 0; i < n_scores; ++i)
        if (!score_ok(scores[i])) { set_error("scores[" + std::to_string(i) + "] is NaN, infinite or above 1e20 in magnitude"); return DAAC_ERR_INVALID_ARGUMENT; }
    return DAAC_OK;
}

daac_status unigram_kind(const daac_pma *pma) { return check_mode_kind(pma, DAAC_FIND_OVERLAPPING); }

daac_status doc_too_long(uint64_t d, uint64_t len) {
    set_error("document " + std::to_string(d) + " has " + std::to_string(len) + " bytes: tokenize_unigram walks a document on one lane and serves fewer than 2^32 - 1 bytes");
    return DAAC_ERR_UNSUPPORTED;
}

struct Outs {   // the caller's out-pointers; the optional ones may be NULL
    uint32_t **dev_ids;
    uint64_t **dev_spans;
    uint64_t **dev_tok_offsets;   // NULL: a single haystack
    float **dev_doc_scores;
    float *score;                 // a single haystack's
    uint64_t *n_tokens, *n_matches;
};

// `text`: byte 0 of document 0 on the device, `len` bytes; `d_off`: the n + 1 offsets on the device (n >= 1), `begin` = offsets[0].
daac_status segment(daac_pma *pma, int engine, const uint8_t *dev_hay, uint64_t begin, uint64_t len, const unsigned long long *d_off, uint64_t n, hipStream_t stream,
                    const float *scores, size_t n_scores, float unk_score, int gap, uint32_t gap_id, const Outs &o) {
    daac_match16 *list = nullptr;
    uint64_t *doc_first = nullptr;
    uint64_t k = 0;
    daac_status st = daac_scan_batch_device16(pma, DAAC_FIND_OVERLAPPING, engine, dev_hay, reinterpret_cast<const uint64_t *>(d_off), n, 1, stream, &list, &doc_first, &k);
    if (st != DAAC_OK) return st;
    auto g_list = dev_guard(list, stream), g_first = dev_guard(doc_first, stream);

    daac::UnigramArgs a{};
    a.hay = dev_hay + begin;
    a.seg = reinterpret_cast<const daac::UniTuple *>(list);
    a.doc_first = reinterpret_cast<const unsigned long long *>(doc_first);
    a.doc_off = d_off;
    a.n_docs = n;
    a.n_scores = n_scores;
    a.unk_score = unk_score;
    a.gap = gap;
    a.gap_id = gap_id;
    // back (8 bytes a position), best and the scores (4), a single haystack's tok_offsets, the total, the sum's scratch
    const uint64_t pos = len + n, m = n + 1;
    DevBuf work;
    HIP_TRY(work.alloc(pos * sizeof(daac::UniBack) + (2 + m + exclusive_scan_scratch(m)) * sizeof(unsigned long long) + (pos + n_scores + n) * sizeof(float), stream));
    a.back = static_cast<daac::UniBack *>(work.p);
    unsigned long long *hdr = reinterpret_cast<unsigned long long *>(a.back + pos);
    unsigned long long *own_off = hdr + 2;
    unsigned long long *scan_scratch = own_off + m;
    a.best = reinterpret_cast<float *>(scan_scratch + exclusive_scan_scratch(m));
    float *d_scores = a.best + pos;
    float *own_doc_scores = d_scores + n_scores;
    if (n_scores) HIP_TRY(hipMemcpyAsync(d_scores, scores, n_scores * sizeof(float), hipMemcpyHostToDevice, stream));
    a.scores = d_scores;

    void *tok_off = nullptr, *doc_scores = nullptr;
    if (o.dev_tok_offsets) HIP_TRY(dev_malloc(&tok_off, m * sizeof(uint64_t), stream));
    auto g_off = dev_guard(tok_off, stream);
    if (o.dev_doc_scores) HIP_TRY(dev_malloc(&doc_scores, n * sizeof(float), stream));
    auto g_scores = dev_guard(doc_scores, stream);
    a.tok_offsets = tok_off ? static_cast<unsigned long long *>(tok_off) : own_off;
    a.doc_scores = doc_scores ? static_cast<float *>(doc_scores) : o.score ? own_doc_scores : nullptr;

    HIP_TRY(daac::launch_unigram_forward(a, stream));
    HIP_TRY(daac::launch_unigram_count(a, stream));
    HIP_TRY(daac::launch_exclusive_scan(a.tok_offsets, m, hdr, scan_scratch, stream));
    unsigned long long total = 0;
    HIP_TRY(hipMemcpyAsync(&total, hdr, sizeof(total), hipMemcpyDeviceToHost, stream));
    if (o.score) HIP_TRY(hipMemcpyAsync(o.score, a.doc_scores, sizeof(float), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    if (total > len) { set_error("the token count does not fit the text"); return DAAC_ERR_DEVICE; }   // (never seen: every edge has a byte)
    const uint64_t per_token = sizeof(uint32_t) + (o.dev_spans ? 2 * sizeof(uint64_t) : 0);
    if (total > static_cast<uint64_t>(OPT(max_result_bytes)) / per_token) {
        set_error("the result of " + std::to_string(total) + " tokens exceeds max_result_bytes");
        return DAAC_ERR_AUTOMATON_SCALE;
    }
    void *ids = nullptr, *spans = nullptr;
    if (total) HIP_TRY(dev_malloc(&ids, total * sizeof(uint32_t), stream));
    auto g_ids = dev_guard(ids, stream);
    if (total && o.dev_spans) HIP_TRY(dev_malloc(&spans, total * 2 * sizeof(uint64_t), stream));
    auto g_spans = dev_guard(spans, stream);
    a.ids = static_cast<uint32_t *>(ids);
    a.spans = static_cast<unsigned long long *>(spans);
    if (total) HIP_TRY(daac::launch_unigram_write(a, stream));
    HIP_TRY(hipStreamSynchronize(stream));   // the call's scratch is released next; the result is the caller's from here
    g_last_kernel = "unigram docs=" + std::to_string(n) + " matches=" + std::to_string(k) + " tokens=" + std::to_string(total) + " " + g_last_kernel;
    *o.dev_ids = static_cast<uint32_t *>(g_ids.release());
    if (o.dev_spans) *o.dev_spans = static_cast<uint64_t *>(g_spans.release());
    if (o.dev_tok_offsets) *o.dev_tok_offsets = static_cast<uint64_t *>(g_off.release());
    if (o.dev_doc_scores) *o.dev_doc_scores = static_cast<float *>(g_scores.release());
    *o.n_tokens = total;
    *o.n_matches = k;
    return DAAC_OK;
}

}  // namespace

extern "C" {

daac_status daac_tokenize_unigram(daac_pma *pma, int engine, const uint8_t *hay, size_t len, int hay_is_device, void *stream_, const float *scores, size_t n_scores,
                                  float unk_score, int gap, uint32_t gap_id, uint32_t **dev_ids, uint64_t **dev_spans, uint64_t *n_tokens, uint64_t *n_matches,
                                  float *score) {
    PmaScope scope_(pma);
    daac_status st = unigram_precheck(pma, scores, n_scores, unk_score, gap, gap_id, dev_ids && n_tokens && n_matches);
    if (st != DAAC_OK) return st;
    if (len && !hay) { set_error("hay is NULL"); return DAAC_ERR_INVALID_ARGUMENT; }
    if ((st = unigram_kind(pma)) != DAAC_OK) return st;
    *dev_ids = nullptr;
    if (dev_spans) *dev_spans = nullptr;
    *n_tokens = 0;
    *n_matches = 0;
    if (score) *score = 0.0f;
    if (len >= kUniMaxDoc) return doc_too_long(0, len);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    DeviceTables *t = nullptr;
    if ((st = get_tables(pma, &t)) != DAAC_OK) return st;   // (no device: 7, before anything is staged)
    StagedBatch b;
    if ((st = stage_one(hay, len, hay_is_device, stream, b)) != DAAC_OK) return st;
    const Outs o{dev_ids, dev_spans, nullptr, nullptr, score, n_tokens, n_matches};
    return segment(pma, engine, b.dev_hay, 0, len, b.d_off, 1, stream, scores, n_scores, unk_score, gap, gap_id, o);
}

daac_status daac_tokenize_unigram_batch(daac_pma *pma, int engine, const uint8_t *hay, const uint64_t *offsets, size_t n, int hay_is_device, void *stream_,
                                        const float *scores, size_t n_scores, float unk_score, int gap, uint32_t gap_id, uint32_t **dev_ids, uint64_t **dev_spans,
                                        uint64_t **dev_tok_offsets, float **dev_doc_scores, uint64_t *n_tokens, uint64_t *n_matches) {
    PmaScope scope_(pma);
    daac_status st = unigram_precheck(pma, scores, n_scores, unk_score, gap, gap_id, dev_ids && dev_tok_offsets && n_tokens && n_matches);
    if (st != DAAC_OK) return st;
    if ((st = check_batch_args(hay, offsets, n, hay_is_device)) != DAAC_OK) return st;
    if ((st = unigram_kind(pma)) != DAAC_OK) return st;
    *dev_ids = nullptr;
    if (dev_spans) *dev_spans = nullptr;
    *dev_tok_offsets = nullptr;
    if (dev_doc_scores) *dev_doc_scores = nullptr;
    *n_tokens = 0;
    *n_matches = 0;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (n == 0) {   // no document: the tuple call's one offset, 0, is this call's
        daac_match16 *list = nullptr;
        uint64_t *doc_first = nullptr;
        uint64_t k = 0;
        if ((st = daac_scan_batch_device16(pma, DAAC_FIND_OVERLAPPING, engine, hay, offsets, 0, hay_is_device, stream_, &list, &doc_first, &k)) != DAAC_OK) return st;
        *dev_tok_offsets = doc_first;
        g_last_kernel = "unigram docs=0 matches=0 tokens=0 " + g_last_kernel;
        return DAAC_OK;
    }
    LongDoc over;   // host offsets: before a device is looked for
    if (!hay_is_device) (void)first_doc_over(kUniMaxDoc - 1, offsets, n, nullptr, stream, over);
    if (over) return doc_too_long(over.doc, over.len);
    DeviceTables *t = nullptr;
    if ((st = get_tables(pma, &t)) != DAAC_OK) return st;   // (no device: 7, before anything is staged)
    StagedBatch b;   // a decreasing pair between the ends is the tuple call's to refuse
    if ((st = stage_batch(hay, offsets, n, hay_is_device, stream, BatchCheck::ends, b)) != DAAC_OK) return st;
    if (hay_is_device && (st = first_doc_over(kUniMaxDoc - 1, offsets, n, b.ends, stream, over)) != DAAC_OK) return st;
    if (over) return doc_too_long(over.doc, over.len);
    const Outs o{dev_ids, dev_spans, dev_tok_offsets, dev_doc_scores, nullptr, n_tokens, n_matches};
    return segment(pma, engine, b.dev_hay, b.ends[0], b.ends[1] - b.ends[0], b.d_off, n, stream, scores, n_scores, unk_score, gap, gap_id, o);
}

}  // extern "C"
