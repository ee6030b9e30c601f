// C ABI (include/daachorse_amd.h), part 9: tokenize on the device (daac_tokenize, daac_tokenize_batch).
// The tuple list comes from the calls that already produce it (daac_scan_device16, daac_scan_batch_device16: their engines, refusals,
// note D and max_result_bytes rule are this call's); the kernels are tokenize_kernels.hip.  This file validates its own arguments,
// counts the tokens (two exclusive sums) and runs the write pass; the read-back of the totals, the max_result_bytes rule, the result's
// buffers and their hand-over are the token calls' back door's (api_internal.hpp, "api_tokens.hip").  A batch's argument rules and its
// staging are the batch front door's ("api_batch.hip"); the single haystack stages its host text here, once.
#include "api_internal.hpp"
#include "tokenize.hpp"

namespace {

// Everything that is decided before a device is touched: statuses 1, 6 and 5, in that order.
daac_status tokenize_precheck(const daac_pma *pma, int mode, int gap, uint32_t gap_id, bool outs_ok) {
    if (!pma || !outs_ok) { set_error("null argument"); return DAAC_ERR_INVALID_ARGUMENT; }
    if (gap < DAAC_GAP_SKIP || gap > DAAC_GAP_CHARS) { set_error("gap is none of DAAC_GAP_SKIP, _UNK, _BYTES, _CHARS"); return DAAC_ERR_INVALID_ARGUMENT; }
    if (gap == DAAC_GAP_BYTES && gap_id > 0xFFFFFFFFu - 255u) { set_error("DAAC_GAP_BYTES: gap_id + 255 does not fit 32 bits"); return DAAC_ERR_INVALID_ARGUMENT; }
    if (mode == DAAC_FIND_OVERLAPPING || mode == DAAC_FIND_OVERLAPPING_NO_SUFFIX) {
        set_error("tokenize serves DAAC_FIND and DAAC_LEFTMOST_FIND: overlapping matches have no gaps");
        return DAAC_ERR_UNSUPPORTED;
    }
    return check_mode_kind(pma, mode);
}

// The tokens of `text` (device, `len` bytes) with the k tuples of `tl`; a batch (d_doc_off != NULL) also gets its tok_offsets.
daac_status tokens(const uint8_t *text, uint64_t len, TupleList &tl, uint64_t k, const unsigned long long *d_doc_off, uint64_t n_docs, int gap,
                   uint32_t gap_id, hipStream_t stream, const TokenOuts &o) {
    TokenizeArgs a{};
    a.hay = text;
    a.len = len;
    a.seg = static_cast<const uint4 *>(tl.list);
    a.k = k;
    a.gap = gap;
    a.gap_id = gap_id;
    a.tiles = len / kTokTile + 1;
    // {flagged bytes, empty matches}, a single haystack's two offsets, A, E, the three per-tile arrays, the sums' scratch
    const uint64_t m = k + 1, tl1 = a.tiles + 1;
    DevBuf work;
    HIP_TRY(work.alloc((4 + 2 + k + m + 3 * tl1 + exclusive_scan_scratch(std::max(m, tl1))) * sizeof(unsigned long long), stream));
    unsigned long long *hdr = static_cast<unsigned long long *>(work.p);
    unsigned long long *pair = hdr + 4;
    a.aend = pair + 2;
    a.epre = a.aend + k;
    a.tile_lo = a.epre + m;
    a.tile_doc = a.tile_lo + tl1;
    a.tile_cnt = a.tile_doc + tl1;
    unsigned long long *scan_scratch = a.tile_cnt + tl1;
    const unsigned long long one_doc[2] = {0, len};
    if (d_doc_off) {
        a.doc_first = reinterpret_cast<const unsigned long long *>(tl.doc_first);
        a.doc_off = d_doc_off;
        a.n_docs = n_docs;
    } else {
        HIP_TRY(hipMemcpyAsync(pair, one_doc, sizeof(one_doc), hipMemcpyHostToDevice, stream));
        a.doc_off = pair;
        a.n_docs = 1;
    }
    HIP_TRY(launch_tokenize_prep(a, stream));
    HIP_TRY(launch_exclusive_scan(a.epre, m, hdr + 1, scan_scratch, stream));
    HIP_TRY(launch_tokenize_count(a, stream));
    HIP_TRY(launch_exclusive_scan(a.tile_cnt, tl1, hdr, scan_scratch, stream));
    unsigned long long h[2];
    daac_status st = read_totals(hdr, 2, stream, h);
    if (st != DAAC_OK) return st;
    const uint64_t flagged = h[0];
    a.n_empty = h[1];
    if (flagged > len || a.n_empty > k) { set_error("the token count does not fit the text and its matches"); return DAAC_ERR_DEVICE; }   // (never seen)
    const uint64_t total = flagged + a.n_empty;
    TokenBufs r;
    if ((st = token_buffers(total, total, o.dev_spans != nullptr, d_doc_off != nullptr, n_docs, stream, r)) != DAAC_OK) return st;   // (fit = total: the check above is this call's)
    a.ids = static_cast<uint32_t *>(r.ids.get());
    a.spans = static_cast<unsigned long long *>(r.spans.get());
    a.tok_offsets = static_cast<unsigned long long *>(r.tok_offsets.get());
    if (total || a.tok_offsets) HIP_TRY(launch_tokenize_write(a, total, stream));
    HIP_TRY(hipStreamSynchronize(stream));   // the call's scratch is released next; the result is the caller's from here
    g_last_kernel = "tokenize matches=" + std::to_string(k) + " tokens=" + std::to_string(total) + " " + g_last_kernel;
    hand_over(r, o, total, k);
    return DAAC_OK;
}

}  // namespace

extern "C" {

daac_status daac_tokenize(daac_pma *pma, int mode, int engine, const uint8_t *hay, size_t len, int hay_is_device, void *stream_, int gap, uint32_t gap_id,
                          uint32_t **dev_ids, uint64_t **dev_spans, uint64_t *n_tokens, uint64_t *n_matches) {
    PmaScope scope_(pma);
    const TokenOuts o{dev_ids, dev_spans, nullptr, n_tokens, n_matches};
    daac_status st = tokenize_precheck(pma, mode, gap, gap_id, o.ok(false));
    if (st != DAAC_OK) return st;
    if (len && !hay) { set_error("hay is NULL"); return DAAC_ERR_INVALID_ARGUMENT; }
    o.clear();
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    DeviceTables *t = nullptr;
    if ((st = get_tables(pma, &t)) != DAAC_OK) return st;   // (no device: 7, before anything is staged)
    void *staged = nullptr;
    const uint8_t *text = hay;
    if (!hay_is_device && len) {   // the passes read the text on the device: the whole haystack, once
        if ((st = stage_window(hay, 0, len, stream, &staged, &text)) != DAAC_OK) return st;
    }
    std::unique_ptr<void, void (*)(void *)> g1(staged, [](void *p) { if (p) (void)hipFree(p); });
    TupleList tl(stream);
    uint64_t k = 0;
    g_last_kernel.clear();   // (the single-haystack tuple call names no kernel: without this the line below kept every earlier call's line behind it)
    if ((st = daac_scan_device16(pma, mode, engine, len ? text : nullptr, len, 1, stream_, reinterpret_cast<daac_match16 **>(&tl.list), &k)) != DAAC_OK) return st;
    return tokens(text, len, tl, k, nullptr, 0, gap, gap_id, stream, o);
}

daac_status daac_tokenize_batch(daac_pma *pma, int mode, int engine, const uint8_t *hay, const uint64_t *offsets, size_t n, int hay_is_device, void *stream_,
                                int gap, uint32_t gap_id, uint32_t **dev_ids, uint64_t **dev_spans, uint64_t **dev_tok_offsets, uint64_t *n_tokens,
                                uint64_t *n_matches) {
    PmaScope scope_(pma);
    const TokenOuts o{dev_ids, dev_spans, dev_tok_offsets, n_tokens, n_matches};
    daac_status st = tokenize_precheck(pma, mode, gap, gap_id, o.ok(true));
    if (st != DAAC_OK) return st;
    if ((st = check_batch_args(hay, offsets, n, hay_is_device)) != DAAC_OK) return st;
    o.clear();
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (n == 0) return no_document(pma, mode, engine, hay, offsets, hay_is_device, stream, "tokenize matches=0 tokens=0 ", o);
    TupleList tl(stream);
    uint64_t k = 0;
    DeviceTables *t = nullptr;
    if ((st = get_tables(pma, &t)) != DAAC_OK) return st;   // (no device: 7, before anything is staged)
    StagedBatch b;   // a decreasing pair between the ends is the tuple call's to refuse
    if ((st = stage_batch(hay, offsets, n, hay_is_device, stream, BatchCheck::ends, b)) != DAAC_OK) return st;
    if ((st = daac_scan_batch_device16(pma, mode, engine, b.dev_hay, reinterpret_cast<const uint64_t *>(b.d_off), n, 1, stream_,
                                       reinterpret_cast<daac_match16 **>(&tl.list), &tl.doc_first, &k)) != DAAC_OK) return st;
    return tokens(b.dev_hay + b.ends[0], b.ends[1] - b.ends[0], tl, k, b.d_off, n, gap, gap_id, stream, o);
}

}  // extern "C"
