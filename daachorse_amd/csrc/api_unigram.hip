// C ABI (include/daachorse_amd.h), part 10: the best-scoring segmentation of a text or a batch on the device (daac_tokenize_unigram,
// daac_tokenize_unigram_batch).  The piece lattice is the tuple CSR of daac_scan_batch_device16(DAAC_FIND_OVERLAPPING): its engines,
// refusals and max_result_bytes rule are this call's; the kernels are unigram_kernels.hip.  This file holds what is the call's own: its
// precheck, its length limit and message, the scores' upload, the forward and count passes, the scores of the documents and the write
// pass.  The order of an entry's checks, the lattice, the scratch's layout, the sum of the counts and its read-back, the limits, the
// result's buffers and their hand-over are the token calls' back door's (api_internal.hpp, "api_tokens.hip"), which goes through the
// batch front door ("api_batch.hip").
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

daac_status doc_too_long(uint64_t d, uint64_t len) {
    set_error("document " + std::to_string(d) + " has " + std::to_string(len) + " bytes: tokenize_unigram walks a document on one lane and serves fewer than 2^32 - 1 bytes");
    return DAAC_ERR_UNSUPPORTED;
}

struct UniOuts : TokenOuts {   // ... and unigram's own, both optional
    float **dev_doc_scores;
    float *score;   // a single haystack's
    void clear() const {
        TokenOuts::clear();
        if (dev_doc_scores) *dev_doc_scores = nullptr;
        if (score) *score = 0.0f;
    }
};

struct Model {
    const float *scores;
    size_t n_scores;
    float unk_score;
    int gap;
    uint32_t gap_id;
};

// the scratch: back (8 bytes a position) in front; best, the scores and a single haystack's doc_scores (4 bytes each) behind
daac_status segment(const LatticeIn &in, const Model &m, const UniOuts &o) {
    const uint64_t pos = in.len + in.n;
    hipStream_t stream = in.stream;
    DevPtr g_scores;
    daac_status st = lattice_tokens<daac::UnigramArgs>("unigram", in, pos * sizeof(daac::UniBack), (pos + m.n_scores + in.n) * sizeof(float), o,
        [&](daac::UnigramArgs &a, void *front, void *behind) -> daac_status {
            a.n_scores = m.n_scores;
            a.unk_score = m.unk_score;
            a.gap = m.gap;
            a.gap_id = m.gap_id;
            a.back = static_cast<daac::UniBack *>(front);
            a.best = static_cast<float *>(behind);
            float *d_scores = a.best + pos, *own_doc_scores = d_scores + m.n_scores;
            if (m.n_scores) HIP_TRY(hipMemcpyAsync(d_scores, m.scores, m.n_scores * sizeof(float), hipMemcpyHostToDevice, stream));
            a.scores = d_scores;
            void *doc_scores = nullptr;
            if (o.dev_doc_scores) HIP_TRY(dev_malloc(&doc_scores, in.n * sizeof(float), stream));
            g_scores = dev_guard(doc_scores, stream);
            a.doc_scores = doc_scores ? static_cast<float *>(doc_scores) : o.score ? own_doc_scores : nullptr;
            HIP_TRY(daac::launch_unigram_forward(a, stream));
            HIP_TRY(daac::launch_unigram_count(a, stream));
            if (o.score) HIP_TRY(hipMemcpyAsync(o.score, a.doc_scores, sizeof(float), hipMemcpyDeviceToHost, stream));   // (waited for with the total)
            return DAAC_OK;
        },
        [&](const daac::UnigramArgs &a) -> daac_status { HIP_TRY(daac::launch_unigram_write(a, stream)); return DAAC_OK; });
    if (st == DAAC_OK && o.dev_doc_scores) *o.dev_doc_scores = static_cast<float *>(g_scores.release());
    return st;
}

}  // namespace

extern "C" {

daac_status daac_tokenize_unigram(daac_pma *pma, int engine, const uint8_t *hay, size_t len, int hay_is_device, void *stream_, const float *scores, size_t n_scores,
                                  float unk_score, int gap, uint32_t gap_id, uint32_t **dev_ids, uint64_t **dev_spans, uint64_t *n_tokens, uint64_t *n_matches,
                                  float *score) {
    PmaScope scope_(pma);
    const UniOuts o{{dev_ids, dev_spans, nullptr, n_tokens, n_matches}, nullptr, score};
    const Model m{scores, n_scores, unk_score, gap, gap_id};
    return lattice_entry(pma, unigram_precheck(pma, scores, n_scores, unk_score, gap, gap_id, o.ok(false)), engine, hay, len, hay_is_device, stream_, kUniMaxDoc - 1,
                         doc_too_long, o, [&](const LatticeIn &in) { return segment(in, m, o); });
}

daac_status daac_tokenize_unigram_batch(daac_pma *pma, int engine, const uint8_t *hay, const uint64_t *offsets, size_t n, int hay_is_device, void *stream_,
                                        const float *scores, size_t n_scores, float unk_score, int gap, uint32_t gap_id, uint32_t **dev_ids, uint64_t **dev_spans,
                                        uint64_t **dev_tok_offsets, float **dev_doc_scores, uint64_t *n_tokens, uint64_t *n_matches) {
    PmaScope scope_(pma);
    const UniOuts o{{dev_ids, dev_spans, dev_tok_offsets, n_tokens, n_matches}, dev_doc_scores, nullptr};
    const Model m{scores, n_scores, unk_score, gap, gap_id};
    return lattice_entry_batch(pma, unigram_precheck(pma, scores, n_scores, unk_score, gap, gap_id, o.ok(true)), engine, hay, offsets, n, hay_is_device, stream_,
                               "unigram docs=0 matches=0 tokens=0 ", kUniMaxDoc - 1, doc_too_long, o, [&](const LatticeIn &in) { return segment(in, m, o); });
}

}  // extern "C"
