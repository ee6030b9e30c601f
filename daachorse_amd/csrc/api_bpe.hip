// C ABI (include/daachorse_amd.h), part 11: the byte-pair-merge token ids of a text or a batch on the device (daac_tokenize_bpe,
// daac_tokenize_bpe_batch).  The pieces are the tuple CSR of daac_scan_batch_device16(DAAC_FIND_OVERLAPPING): its engines, refusals and
// max_result_bytes rule are this call's; the kernels are bpe_kernels.hip.  This file holds what is the call's own: its precheck, its
// length limit (option bpe_doc_max) and message, the ranks' upload, the merge pass and the write pass.  The order of an entry's checks,
// the lattice, the scratch's layout, the sum of the counts and its read-back, the limits, the result's buffers and their hand-over are
// the token calls' back door's (api_internal.hpp, "api_tokens.hip"), which goes through the batch front door ("api_batch.hip").
#include "api_internal.hpp"
#include "bpe.hpp"

namespace {

// Status 1, then status 5, before a device is touched.
daac_status bpe_precheck(const daac_pma *pma, const uint32_t *ranks, size_t n_ranks, int gap, uint32_t gap_id, bool outs_ok) {
    if (!pma || !outs_ok) { set_error("null argument"); return DAAC_ERR_INVALID_ARGUMENT; }
    if (gap != DAAC_GAP_BYTES && gap != DAAC_GAP_CHARS) { set_error("gap is neither DAAC_GAP_BYTES nor DAAC_GAP_CHARS: the initial parts must tile the text"); return DAAC_ERR_INVALID_ARGUMENT; }
    if (gap == DAAC_GAP_BYTES && gap_id > 0xFFFFFFFFu - 255u) { set_error("DAAC_GAP_BYTES: gap_id + 255 does not fit 32 bits"); return DAAC_ERR_INVALID_ARGUMENT; }
    if (!ranks && n_ranks) { set_error("ranks is NULL with n_ranks = " + std::to_string(n_ranks)); return DAAC_ERR_INVALID_ARGUMENT; }
    if (ranks && !n_ranks) { set_error("n_ranks is 0 with a ranks table (no table: ranks = NULL)"); return DAAC_ERR_INVALID_ARGUMENT; }
    if (ranks) {
        const std::vector<daac::OutputRec> &outs = pma->charwise ? pma->chost.outputs : pma->host.outputs;
        uint64_t need = 0;   // the largest value + 1
        for (const daac::OutputRec &o : outs) need = std::max<uint64_t>(need, static_cast<uint64_t>(o.value) + 1);
        if (n_ranks < need) { set_error("n_ranks = " + std::to_string(n_ranks) + " does not cover the largest match value, " + std::to_string(need - 1)); return DAAC_ERR_INVALID_ARGUMENT; }
    }
    return DAAC_OK;
}

uint64_t bpe_doc_max() { return static_cast<uint64_t>(std::min<int64_t>(std::max<int64_t>(1, OPT(bpe_doc_max)), static_cast<int64_t>(daac::kBpeDocCap))); }

daac_status doc_too_long(uint64_t d, uint64_t len, uint64_t cap) {
    set_error("document " + std::to_string(d) + " has " + std::to_string(len) + " bytes, above bpe_doc_max (" + std::to_string(cap) +
              "): tokenize_bpe merges a document on one lane in up to L^2 / 2 steps; pre-split the text (BPE runs behind a pre-tokenizer), or raise the option (at most 65536)");
    return DAAC_ERR_UNSUPPORTED;
}

struct Model {
    const uint32_t *ranks;
    size_t n_ranks;
    uint64_t cap;   // no document is longer
    int gap;
    uint32_t gap_id;
};

// the scratch: the slots (24 bytes a position) in front; the ranks behind
daac_status merge(const LatticeIn &in, const Model &m, const TokenOuts &o) {
    const uint64_t pos = in.len + in.n;
    hipStream_t stream = in.stream;
    return lattice_tokens<daac::BpeArgs>("bpe", in, pos * sizeof(daac::BpeSlot), m.n_ranks * sizeof(uint32_t), o,
        [&](daac::BpeArgs &a, void *front, void *behind) -> daac_status {
            a.n_ranks = m.n_ranks;
            a.doc_max = m.cap;
            a.gap = m.gap;
            a.gap_id = m.gap_id;
            a.slots = static_cast<daac::BpeSlot *>(front);
            if (m.n_ranks) HIP_TRY(hipMemcpyAsync(behind, m.ranks, m.n_ranks * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
            a.ranks = m.n_ranks ? static_cast<const uint32_t *>(behind) : nullptr;
            HIP_TRY(daac::launch_bpe_merge(a, stream));
            return DAAC_OK;
        },
        [&](const daac::BpeArgs &a) -> daac_status { HIP_TRY(daac::launch_bpe_write(a, stream)); return DAAC_OK; });
}

}  // namespace

extern "C" {

daac_status daac_tokenize_bpe(daac_pma *pma, int engine, const uint8_t *hay, size_t len, int hay_is_device, void *stream_, const uint32_t *ranks, size_t n_ranks,
                              int gap, uint32_t gap_id, uint32_t **dev_ids, uint64_t **dev_spans, uint64_t *n_tokens, uint64_t *n_matches) {
    PmaScope scope_(pma);
    const TokenOuts o{dev_ids, dev_spans, nullptr, n_tokens, n_matches};
    const Model m{ranks, n_ranks, bpe_doc_max(), gap, gap_id};
    return lattice_entry(pma, bpe_precheck(pma, ranks, n_ranks, gap, gap_id, o.ok(false)), engine, hay, len, hay_is_device, stream_, m.cap,
                         [&](uint64_t d, uint64_t l) { return doc_too_long(d, l, m.cap); }, o, [&](const LatticeIn &in) { return merge(in, m, o); });
}

daac_status daac_tokenize_bpe_batch(daac_pma *pma, int engine, const uint8_t *hay, const uint64_t *offsets, size_t n, int hay_is_device, void *stream_,
                                    const uint32_t *ranks, size_t n_ranks, int gap, uint32_t gap_id, uint32_t **dev_ids, uint64_t **dev_spans,
                                    uint64_t **dev_tok_offsets, uint64_t *n_tokens, uint64_t *n_matches) {
    PmaScope scope_(pma);
    const TokenOuts o{dev_ids, dev_spans, dev_tok_offsets, n_tokens, n_matches};
    const Model m{ranks, n_ranks, bpe_doc_max(), gap, gap_id};
    return lattice_entry_batch(pma, bpe_precheck(pma, ranks, n_ranks, gap, gap_id, o.ok(true)), engine, hay, offsets, n, hay_is_device, stream_,
                               "bpe docs=0 matches=0 tokens=0 ", m.cap, [&](uint64_t d, uint64_t l) { return doc_too_long(d, l, m.cap); }, o,
                               [&](const LatticeIn &in) { return merge(in, m, o); });
}

}  // extern "C"
