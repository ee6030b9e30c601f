// C ABI (include/daachorse_amd.h), part 11: the byte-pair-merge token ids of a text or a batch on the device (daac_tokenize_bpe,
// daac_tokenize_bpe_batch).  The pieces are the tuple CSR of daac_scan_batch_device16(DAAC_FIND_OVERLAPPING): its engines, refusals and
// max_result_bytes rule are this call's; the kernels are bpe_kernels.hip.  This file validates its own arguments, refuses a document
// above option bpe_doc_max, copies the ranks, runs the merge pass, sums the counts (one read-back), allocates the result and runs the
// write pass.  The batch arguments' rules, the staging of a host text, the length check of device offsets and the single haystack as a
// batch of one document are the batch front door's (api_internal.hpp, "api_batch.hip").
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

struct Outs {   // the caller's out-pointers; the optional ones may be NULL
    uint32_t **dev_ids;
    uint64_t **dev_spans;
    uint64_t **dev_tok_offsets;   // NULL: a single haystack
    uint64_t *n_tokens, *n_matches;
};

// `dev_hay`: the haystack on the device, document 0 begins at `begin`; `len`: the bytes of all documents; `d_off`: the n + 1 offsets on
// the device (n >= 1).  No document is longer than `cap`.
daac_status merge(daac_pma *pma, int engine, const uint8_t *dev_hay, uint64_t begin, uint64_t len, const unsigned long long *d_off, uint64_t n, hipStream_t stream,
                  const uint32_t *ranks, size_t n_ranks, uint64_t cap, int gap, uint32_t gap_id, const Outs &o) {
    daac_match16 *list = nullptr;
    uint64_t *doc_first = nullptr;
    uint64_t k = 0;
    daac_status st = daac_scan_batch_device16(pma, DAAC_FIND_OVERLAPPING, engine, dev_hay, reinterpret_cast<const uint64_t *>(d_off), n, 1, stream, &list, &doc_first, &k);
    if (st != DAAC_OK) return st;
    auto g_list = dev_guard(list, stream), g_first = dev_guard(doc_first, stream);

    daac::BpeArgs a{};
    a.hay = dev_hay + begin;
    a.seg = reinterpret_cast<const daac::BpeTuple *>(list);
    a.doc_first = reinterpret_cast<const unsigned long long *>(doc_first);
    a.doc_off = d_off;
    a.n_docs = n;
    a.n_ranks = n_ranks;
    a.doc_max = cap;
    a.gap = gap;
    a.gap_id = gap_id;
    // the slots (24 bytes a position), a single haystack's tok_offsets, the total, the sum's scratch, the ranks
    const uint64_t pos = len + n, m = n + 1;
    DevBuf work;
    HIP_TRY(work.alloc(pos * sizeof(daac::BpeSlot) + (2 + m + exclusive_scan_scratch(m)) * sizeof(unsigned long long) + n_ranks * sizeof(uint32_t), stream));
    a.slots = static_cast<daac::BpeSlot *>(work.p);
    unsigned long long *hdr = reinterpret_cast<unsigned long long *>(a.slots + pos);
    unsigned long long *own_off = hdr + 2;
    unsigned long long *scan_scratch = own_off + m;
    uint32_t *d_ranks = reinterpret_cast<uint32_t *>(scan_scratch + exclusive_scan_scratch(m));
    if (n_ranks) HIP_TRY(hipMemcpyAsync(d_ranks, ranks, n_ranks * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
    a.ranks = n_ranks ? d_ranks : nullptr;

    void *tok_off = nullptr;
    if (o.dev_tok_offsets) HIP_TRY(dev_malloc(&tok_off, m * sizeof(uint64_t), stream));
    auto g_off = dev_guard(tok_off, stream);
    a.tok_offsets = tok_off ? static_cast<unsigned long long *>(tok_off) : own_off;

    HIP_TRY(daac::launch_bpe_merge(a, stream));
    HIP_TRY(daac::launch_exclusive_scan(a.tok_offsets, m, hdr, scan_scratch, stream));
    unsigned long long total = 0;
    HIP_TRY(hipMemcpyAsync(&total, hdr, sizeof(total), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    if (total > len) { set_error("the token count does not fit the text"); return DAAC_ERR_DEVICE; }   // (never seen: every part has a byte)
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
    if (total) HIP_TRY(daac::launch_bpe_write(a, stream));
    HIP_TRY(hipStreamSynchronize(stream));   // the call's scratch is released next; the result is the caller's from here
    g_last_kernel = "bpe docs=" + std::to_string(n) + " matches=" + std::to_string(k) + " tokens=" + std::to_string(total) + " " + g_last_kernel;
    *o.dev_ids = static_cast<uint32_t *>(g_ids.release());
    if (o.dev_spans) *o.dev_spans = static_cast<uint64_t *>(g_spans.release());
    if (o.dev_tok_offsets) *o.dev_tok_offsets = static_cast<uint64_t *>(g_off.release());
    *o.n_tokens = total;
    *o.n_matches = k;
    return DAAC_OK;
}

}  // namespace

extern "C" {

daac_status daac_tokenize_bpe(daac_pma *pma, int engine, const uint8_t *hay, size_t len, int hay_is_device, void *stream_, const uint32_t *ranks, size_t n_ranks,
                              int gap, uint32_t gap_id, uint32_t **dev_ids, uint64_t **dev_spans, uint64_t *n_tokens, uint64_t *n_matches) {
    PmaScope scope_(pma);
    daac_status st = bpe_precheck(pma, ranks, n_ranks, gap, gap_id, dev_ids && n_tokens && n_matches);
    if (st != DAAC_OK) return st;
    if (len && !hay) { set_error("hay is NULL"); return DAAC_ERR_INVALID_ARGUMENT; }
    if ((st = check_mode_kind(pma, DAAC_FIND_OVERLAPPING)) != DAAC_OK) return st;
    *dev_ids = nullptr;
    if (dev_spans) *dev_spans = nullptr;
    *n_tokens = 0;
    *n_matches = 0;
    const uint64_t cap = bpe_doc_max();
    if (len > cap) return doc_too_long(0, len, cap);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    DeviceTables *t = nullptr;
    if ((st = get_tables(pma, &t)) != DAAC_OK) return st;   // (no device: 7, before anything is staged)
    StagedBatch b;
    if ((st = stage_one(hay, len, hay_is_device, stream, b)) != DAAC_OK) return st;
    const Outs o{dev_ids, dev_spans, nullptr, n_tokens, n_matches};
    return merge(pma, engine, b.dev_hay, 0, len, b.d_off, 1, stream, ranks, n_ranks, cap, gap, gap_id, o);
}

daac_status daac_tokenize_bpe_batch(daac_pma *pma, int engine, const uint8_t *hay, const uint64_t *offsets, size_t n, int hay_is_device, void *stream_,
                                    const uint32_t *ranks, size_t n_ranks, int gap, uint32_t gap_id, uint32_t **dev_ids, uint64_t **dev_spans,
                                    uint64_t **dev_tok_offsets, uint64_t *n_tokens, uint64_t *n_matches) {
    PmaScope scope_(pma);
    daac_status st = bpe_precheck(pma, ranks, n_ranks, gap, gap_id, dev_ids && dev_tok_offsets && n_tokens && n_matches);
    if (st != DAAC_OK) return st;
    if ((st = check_batch_args(hay, offsets, n, hay_is_device)) != DAAC_OK) return st;
    if ((st = check_mode_kind(pma, DAAC_FIND_OVERLAPPING)) != DAAC_OK) return st;
    *dev_ids = nullptr;
    if (dev_spans) *dev_spans = nullptr;
    *dev_tok_offsets = nullptr;
    *n_tokens = 0;
    *n_matches = 0;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (n == 0) {   // no document: the tuple call's one offset, 0, is this call's
        daac_match16 *list = nullptr;
        uint64_t *doc_first = nullptr;
        uint64_t k = 0;
        if ((st = daac_scan_batch_device16(pma, DAAC_FIND_OVERLAPPING, engine, hay, offsets, 0, hay_is_device, stream_, &list, &doc_first, &k)) != DAAC_OK) return st;
        *dev_tok_offsets = doc_first;
        g_last_kernel = "bpe docs=0 matches=0 tokens=0 " + g_last_kernel;
        return DAAC_OK;
    }
    const uint64_t cap = bpe_doc_max();
    LongDoc over;   // host offsets: before a device is looked for
    if (!hay_is_device) (void)first_doc_over(cap, offsets, n, nullptr, stream, over);
    if (over) return doc_too_long(over.doc, over.len, cap);
    DeviceTables *t = nullptr;
    if ((st = get_tables(pma, &t)) != DAAC_OK) return st;   // (no device: 7, before anything is staged)
    StagedBatch b;   // a decreasing pair between the ends is the tuple call's to refuse (before the merge pass)
    if ((st = stage_batch(hay, offsets, n, hay_is_device, stream, BatchCheck::ends, b)) != DAAC_OK) return st;
    if (hay_is_device && (st = first_doc_over(cap, offsets, n, b.ends, stream, over)) != DAAC_OK) return st;
    if (over) return doc_too_long(over.doc, over.len, cap);
    const Outs o{dev_ids, dev_spans, dev_tok_offsets, n_tokens, n_matches};
    return merge(pma, engine, b.dev_hay, b.ends[0], b.ends[1] - b.ends[0], b.d_off, n, stream, ranks, n_ranks, cap, gap, gap_id, o);
}

}  // extern "C"
