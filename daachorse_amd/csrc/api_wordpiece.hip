// C ABI (include/daachorse_amd.h), part 13: BERT's WordPiece token ids of a word or a batch of words on the device
// (daac_tokenize_wordpiece, daac_tokenize_wordpiece_batch).  The pieces are the tuple CSR of
// daac_scan_batch_device16(DAAC_FIND_OVERLAPPING): its engines, refusals and max_result_bytes rule are this call's; the kernels are
// wordpiece_kernels.hip.  This file holds what is the call's own: its precheck, its length limit and message, the two id tables' upload,
// the count pass and the write pass.  The order of an entry's checks, the lattice, the scratch's layout, the sum of the counts and its
// read-back, the limits, the result's buffers and their hand-over are the token calls' back door's (api_internal.hpp, "api_tokens.hip"),
// which goes through the batch front door ("api_batch.hip").
#include "api_internal.hpp"
#include "wordpiece.hpp"

namespace {

// Status 1 before a device is touched.
daac_status wp_precheck(const daac_pma *pma, const uint32_t *first_ids, const uint32_t *cont_ids, size_t n_ids, uint32_t max_chars, bool outs_ok) {
    if (!pma || !outs_ok) { set_error("null argument"); return DAAC_ERR_INVALID_ARGUMENT; }
    if (max_chars == 0) { set_error("max_chars is 0 (1 .. 0xFFFFFFFF; BERT has 100)"); return DAAC_ERR_INVALID_ARGUMENT; }
    if (!first_ids) { set_error("first_ids is NULL"); return DAAC_ERR_INVALID_ARGUMENT; }
    if (!cont_ids) { set_error("cont_ids is NULL"); return DAAC_ERR_INVALID_ARGUMENT; }
    const std::vector<daac::OutputRec> &outs = pma->charwise ? pma->chost.outputs : pma->host.outputs;
    uint64_t need = 0;   // the largest value + 1
    for (const daac::OutputRec &o : outs) need = std::max<uint64_t>(need, static_cast<uint64_t>(o.value) + 1);
    if (n_ids < need) { set_error("n_ids = " + std::to_string(n_ids) + " does not cover the largest match value, " + std::to_string(need - 1)); return DAAC_ERR_INVALID_ARGUMENT; }
    return DAAC_OK;
}

daac_status doc_too_long(uint64_t d, uint64_t len) {
    set_error("document " + std::to_string(d) + " has " + std::to_string(len) + " bytes: tokenize_wordpiece walks a document on one lane and serves fewer than 2^32 - 1 bytes");
    return DAAC_ERR_UNSUPPORTED;
}

struct Model {
    const uint32_t *first_ids, *cont_ids;
    size_t n_ids;
    uint32_t unk_id, max_chars;
    const uint8_t *dev_skip;
};

// the scratch: the slots (8 bytes a position) in front; the two id tables behind
daac_status segment(const LatticeIn &in, const Model &m, const TokenOuts &o) {
    const uint64_t pos = in.len + in.n;
    hipStream_t stream = in.stream;
    return lattice_tokens<daac::WpArgs>("wordpiece", in, pos * sizeof(daac::WpSlot), 2 * m.n_ids * sizeof(uint32_t), o,
        [&](daac::WpArgs &a, void *front, void *behind) -> daac_status {
            a.n_ids = m.n_ids;
            a.unk_id = m.unk_id;
            a.max_chars = m.max_chars;
            a.skip = m.dev_skip;
            a.slots = static_cast<daac::WpSlot *>(front);
            uint32_t *d_first = static_cast<uint32_t *>(behind), *d_cont = d_first + m.n_ids;
            if (m.n_ids) {
                HIP_TRY(hipMemcpyAsync(d_first, m.first_ids, m.n_ids * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
                HIP_TRY(hipMemcpyAsync(d_cont, m.cont_ids, m.n_ids * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
            }
            a.first_ids = d_first;
            a.cont_ids = d_cont;
            HIP_TRY(daac::launch_wordpiece_count(a, stream));
            return DAAC_OK;
        },
        [&](const daac::WpArgs &a) -> daac_status { HIP_TRY(daac::launch_wordpiece_write(a, stream)); return DAAC_OK; });
}

}  // namespace

extern "C" {

daac_status daac_tokenize_wordpiece(daac_pma *pma, int engine, const uint8_t *hay, size_t len, int hay_is_device, void *stream_, const uint32_t *first_ids,
                                    const uint32_t *cont_ids, size_t n_ids, uint32_t unk_id, uint32_t max_chars, uint32_t **dev_ids, uint64_t **dev_spans,
                                    uint64_t *n_tokens, uint64_t *n_matches) {
    PmaScope scope_(pma);
    const TokenOuts o{dev_ids, dev_spans, nullptr, n_tokens, n_matches};
    const Model m{first_ids, cont_ids, n_ids, unk_id, max_chars, nullptr};
    return lattice_entry(pma, wp_precheck(pma, first_ids, cont_ids, n_ids, max_chars, o.ok(false)), engine, hay, len, hay_is_device, stream_, daac::kWpMaxDoc - 1,
                         doc_too_long, o, [&](const LatticeIn &in) { return segment(in, m, o); });
}

daac_status daac_tokenize_wordpiece_batch(daac_pma *pma, int engine, const uint8_t *hay, const uint64_t *offsets, size_t n, int hay_is_device, void *stream_,
                                          const uint32_t *first_ids, const uint32_t *cont_ids, size_t n_ids, uint32_t unk_id, uint32_t max_chars,
                                          const uint8_t *dev_skip, uint32_t **dev_ids, uint64_t **dev_spans, uint64_t **dev_tok_offsets, uint64_t *n_tokens,
                                          uint64_t *n_matches) {
    PmaScope scope_(pma);
    const TokenOuts o{dev_ids, dev_spans, dev_tok_offsets, n_tokens, n_matches};
    const Model m{first_ids, cont_ids, n_ids, unk_id, max_chars, dev_skip};
    return lattice_entry_batch(pma, wp_precheck(pma, first_ids, cont_ids, n_ids, max_chars, o.ok(true)), engine, hay, offsets, n, hay_is_device, stream_,
                               "wordpiece docs=0 matches=0 tokens=0 ", daac::kWpMaxDoc - 1, doc_too_long, o, [&](const LatticeIn &in) { return segment(in, m, o); });
}

}  // extern "C"
