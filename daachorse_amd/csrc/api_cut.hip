// C ABI (include/daachorse_amd.h), part 15: special tokens in raw text — a batch cut into segments around the matches of a leftmost
// automaton (daac_cut_batch) and a tokenizer's result over the segment batch put back together per document (daac_tokens_splice).
// The tuple list comes from the call that already produces it (daac_scan_batch_device16 with DAAC_LEFTMOST_FIND: its engines, refusals
// and max_result_bytes rule are this call's); the kernels are cut_kernels.hip and, for the token offsets per document,
// split_kernels.hip's offsets_compose.  This file validates its own arguments, counts (an exclusive sum and one read-back per call),
// allocates the result and runs the write pass; the splice's read-back, token limit, buffers and hand-over are the token calls' back
// door's (api_internal.hpp, "api_tokens.hip").  The batch arguments' rules and the staging of a host batch are the batch front door's
// ("api_batch.hip").
#include "api_internal.hpp"
#include "cut.hpp"
#include "split.hpp"

namespace {

// Everything that is decided before a device is touched, in the header's order: statuses 1, 1 (the offsets), 5, 1, 1, 2.
daac_status cut_precheck(const daac_pma *pma, const uint8_t *hay, const uint64_t *offsets, size_t n, int hay_is_device, bool outs_ok) {
    if (!pma || !outs_ok) { set_error("null argument"); return DAAC_ERR_INVALID_ARGUMENT; }
    daac_status st = check_batch_args(hay, offsets, n, hay_is_device);
    if (st != DAAC_OK) return st;
    if ((st = check_mode_kind(pma, DAAC_LEFTMOST_FIND)) != DAAC_OK) return st;
    std::vector<uint32_t> recs(3 * daac_pma_outputs(pma, nullptr, 0));
    daac_pma_outputs(pma, recs.data(), recs.size() / 3);
    for (size_t i = 0; i < recs.size(); i += 3)
        if (recs[i + 1] == 0) { set_error("the empty pattern is among the special tokens: a segment has at least one byte"); return DAAC_ERR_INVALID_ARGUMENT; }
    for (size_t i = 0; i < recs.size(); i += 3)
        if (recs[i] == daac::kCutText) { set_error("a special token has the value 0xFFFFFFFF, which marks a text segment"); return DAAC_ERR_INVALID_ARGUMENT; }
    if (n + 1 > static_cast<uint64_t>(OPT(max_result_bytes)) / sizeof(uint64_t)) {
        set_error("doc_segs of " + std::to_string(n) + " documents exceeds max_result_bytes");
        return DAAC_ERR_AUTOMATON_SCALE;
    }
    return DAAC_OK;
}

}  // namespace

extern "C" {

daac_status daac_cut_batch(daac_pma *special, int engine, const uint8_t *hay, const uint64_t *offsets, size_t n, int hay_is_device, void *stream_,
                           uint64_t **dev_seg_offsets, uint64_t **dev_doc_segs, uint32_t **dev_seg_values, uint64_t *n_segs, uint64_t *n_special) {
    PmaScope scope_(special);
    daac_status st = cut_precheck(special, hay, offsets, n, hay_is_device, dev_seg_offsets && dev_doc_segs && dev_seg_values && n_segs && n_special);
    if (st != DAAC_OK) return st;
    *dev_seg_offsets = nullptr;
    *dev_doc_segs = nullptr;
    *dev_seg_values = nullptr;
    *n_segs = 0;
    *n_special = 0;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    TupleList tl(stream);
    uint64_t k = 0;
    if (n == 0) {   // no document: the tuple call's one offset, 0, is seg_offsets; doc_segs is one more
        if ((st = daac_scan_batch_device16(special, DAAC_LEFTMOST_FIND, engine, hay, offsets, 0, hay_is_device, stream_, reinterpret_cast<daac_match16 **>(&tl.list), &tl.doc_first, &k)) != DAAC_OK) return st;
        DevPtr g_ds;
        if ((st = zero_word(stream, g_ds)) != DAAC_OK) return st;
        HIP_TRY(hipStreamSynchronize(stream));
        g_last_kernel = "cut docs=0 matches=0 segs=0 " + g_last_kernel;
        *dev_seg_offsets = tl.doc_first;
        tl.doc_first = nullptr;
        *dev_doc_segs = static_cast<uint64_t *>(g_ds.release());
        return DAAC_OK;
    }
    DeviceTables *t = nullptr;
    if ((st = get_tables(special, &t)) != DAAC_OK) return st;   // (no device: 7, before anything is staged)
    StagedBatch b;   // no kernel of this call reads the text, so the ends are not needed: device offsets are validated by the tuple call
    if ((st = stage_batch(hay, offsets, n, hay_is_device, stream, BatchCheck::none, b)) != DAAC_OK) return st;
    if ((st = daac_scan_batch_device16(special, DAAC_LEFTMOST_FIND, engine, b.dev_hay, reinterpret_cast<const uint64_t *>(b.d_off), n, 1, stream_,
                                       reinterpret_cast<daac_match16 **>(&tl.list), &tl.doc_first, &k)) != DAAC_OK) return st;
    daac::CutArgs a{};
    a.seg = static_cast<const daac::CutTuple *>(tl.list);
    a.doc_first = reinterpret_cast<const unsigned long long *>(tl.doc_first);
    a.doc_off = b.d_off;
    a.n_docs = n;
    a.k = k;
    // the scratch: the items' counts with the closing entry, their sum, the sum's scratch
    const uint64_t items = n + k;
    DevBuf work;
    HIP_TRY(work.alloc((items + 1 + 1 + exclusive_scan_scratch(items + 1)) * sizeof(unsigned long long), stream));
    a.counts = static_cast<unsigned long long *>(work.p);
    unsigned long long *sum = a.counts + items + 1, *scan_scratch = sum + 1;
    HIP_TRY(daac::launch_cut_count(a, stream));
    HIP_TRY(daac::launch_exclusive_scan(a.counts, items + 1, sum, scan_scratch, stream));
    unsigned long long segs = 0;
    HIP_TRY(hipMemcpyAsync(&segs, sum, sizeof(segs), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    if (segs > n + 2 * k) { set_error("the segment count does not fit the documents and their matches"); return DAAC_ERR_DEVICE; }   // (never seen)
    if (segs + 1 > static_cast<uint64_t>(OPT(max_result_bytes)) / sizeof(uint64_t)) {
        set_error("the list of " + std::to_string(segs) + " segments exceeds max_result_bytes");
        return DAAC_ERR_AUTOMATON_SCALE;
    }
    void *so = nullptr, *ds = nullptr, *sv = nullptr;
    HIP_TRY(dev_malloc(&so, (segs + 1) * sizeof(uint64_t), stream));
    DevPtr g_so = dev_guard(so, stream);
    HIP_TRY(dev_malloc(&ds, (n + 1) * sizeof(uint64_t), stream));
    DevPtr g_ds = dev_guard(ds, stream);
    if (segs) HIP_TRY(dev_malloc(&sv, segs * sizeof(uint32_t), stream));
    DevPtr g_sv = dev_guard(sv, stream);
    a.seg_offsets = static_cast<unsigned long long *>(so);
    a.doc_segs = static_cast<unsigned long long *>(ds);
    a.seg_values = static_cast<uint32_t *>(sv);
    HIP_TRY(daac::launch_cut_write(a, stream));
    HIP_TRY(hipStreamSynchronize(stream));   // the call's scratch is released next; the result is the caller's from here
    g_last_kernel = "cut docs=" + std::to_string(n) + " matches=" + std::to_string(k) + " segs=" + std::to_string(segs) + " " + g_last_kernel;
    *dev_seg_offsets = static_cast<uint64_t *>(g_so.release());
    *dev_doc_segs = static_cast<uint64_t *>(g_ds.release());
    *dev_seg_values = static_cast<uint32_t *>(g_sv.release());
    *n_segs = segs;
    *n_special = k;
    return DAAC_OK;
}

daac_status daac_tokens_splice(const uint32_t *dev_ids, const uint64_t *dev_spans, const uint64_t *dev_seg_tok, const uint32_t *dev_seg_values,
                               const uint64_t *dev_seg_offsets, const uint64_t *dev_doc_segs, const uint64_t *dev_doc_offsets, size_t n_segs, size_t n_docs,
                               void *stream_, uint32_t **dev_out_ids, uint64_t **dev_out_spans, uint64_t **dev_doc_tok, uint64_t *n_tokens) {
    PmaScope scope_(nullptr);   // no handle: the process-wide options
    uint64_t no_matches = 0;   // (the splice has no match count)
    const TokenOuts o{dev_out_ids, dev_out_spans, dev_doc_tok, n_tokens, &no_matches};
    if (!dev_seg_tok || !dev_seg_offsets || !dev_doc_segs || !dev_doc_offsets || !o.ok(true) || (n_segs && !dev_seg_values)) {
        set_error("null argument");
        return DAAC_ERR_INVALID_ARGUMENT;
    }
    if (n_segs && !n_docs) { set_error("segments without a document"); return DAAC_ERR_INVALID_ARGUMENT; }
    o.clear();
    if (n_docs + 1 > static_cast<uint64_t>(OPT(max_result_bytes)) / sizeof(uint64_t)) { set_error("doc_tok of " + std::to_string(n_docs) + " documents exceeds max_result_bytes"); return DAAC_ERR_AUTOMATON_SCALE; }
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    daac::SpliceArgs a{};
    a.ids = dev_ids;
    a.seg_tok = reinterpret_cast<const unsigned long long *>(dev_seg_tok);
    a.seg_values = dev_seg_values;
    a.seg_offsets = reinterpret_cast<const unsigned long long *>(dev_seg_offsets);
    a.doc_segs = reinterpret_cast<const unsigned long long *>(dev_doc_segs);
    a.doc_off = reinterpret_cast<const unsigned long long *>(dev_doc_offsets);
    a.n_segs = n_segs;
    a.n_docs = n_docs;
    // the scratch: the segments' new token offsets with the closing entry, {their sum, the tokens that came in}, the sum's scratch
    DevBuf work;
    HIP_TRY(work.alloc((n_segs + 1 + 2 + exclusive_scan_scratch(n_segs + 1)) * sizeof(unsigned long long), stream));
    a.out_seg_tok = static_cast<unsigned long long *>(work.p);
    unsigned long long *hdr = a.out_seg_tok + n_segs + 1, *scan_scratch = hdr + 2;
    HIP_TRY(daac::launch_splice_count(a, stream));
    HIP_TRY(daac::launch_exclusive_scan(a.out_seg_tok, n_segs + 1, hdr, scan_scratch, stream));
    HIP_TRY(hipMemcpyAsync(hdr + 1, a.seg_tok + n_segs, sizeof(unsigned long long), hipMemcpyDeviceToDevice, stream));
    unsigned long long h[2] = {0, 0};
    daac_status st = read_totals(hdr, 2, stream, h);
    if (st != DAAC_OK) return st;
    const uint64_t total = h[0];
    if (!dev_ids && h[1]) { set_error("dev_ids is NULL with " + std::to_string(h[1]) + " tokens"); return DAAC_ERR_INVALID_ARGUMENT; }
    // spans: wanted with dev_out_spans, unless the tokens that came in have none (without such tokens the specials' spans are all there is);
    // not wanted, the guard stays empty and the hand-over leaves NULL in dev_out_spans
    const bool want_spans = dev_out_spans && (dev_spans || !h[1]);
    a.spans = reinterpret_cast<const unsigned long long *>(dev_spans);
    TokenBufs r;
    if ((st = token_buffers(total, total, want_spans, true, n_docs, stream, r)) != DAAC_OK) return st;   // (fit = total: the splice has no such bound)
    a.out_ids = static_cast<uint32_t *>(r.ids.get());
    a.out_spans = static_cast<unsigned long long *>(r.spans.get());
    if (total) HIP_TRY(daac::launch_splice_write(a, stream));
    HIP_TRY(daac::launch_offsets_compose(a.out_seg_tok, a.doc_segs, n_docs + 1, static_cast<unsigned long long *>(r.tok_offsets.get()), stream));
    HIP_TRY(hipStreamSynchronize(stream));   // the call's scratch is released next; the result is the caller's from here
    g_last_kernel = "splice docs=" + std::to_string(n_docs) + " segs=" + std::to_string(n_segs) + " tokens=" + std::to_string(total);
    hand_over(r, o, total, 0);
    return DAAC_OK;
}

}  // extern "C"
