// C ABI (include/daachorse_amd.h), part 8: replace_all on the device (daac_replace_all, daac_replace_all_batch).
// The tuple list comes from the calls that already produce it (daac_scan_device16, daac_scan_batch_device16: their engines, refusals,
// note D and max_result_bytes rule are this call's); the kernels are replace_kernels.hip.  This file validates its own arguments,
// sizes the result (two exclusive sums and one read-back), allocates it and runs the splice.  A batch's argument rules and its staging
// are the batch front door's (api_internal.hpp, "api_batch.hip"); the single haystack stages its host text here, once.
#include "api_internal.hpp"
#include "replace.hpp"

namespace {

constexpr unsigned long long kNone = ~0ull;

// Everything that is decided before a device is touched: statuses 1, 6 and 5, in that order.
daac_status replace_precheck(const daac_pma *pma, int mode, const uint8_t *repl, const uint64_t *repl_offsets, size_t n_repl, bool outs_ok) {
    if (!pma || !outs_ok) { set_error("null argument"); return DAAC_ERR_INVALID_ARGUMENT; }
    if (n_repl == 0 || !repl_offsets) { set_error("replacements: n_repl is 0 or repl_offsets is NULL"); return DAAC_ERR_INVALID_ARGUMENT; }
    for (size_t i = 0; i < n_repl; ++i)
        if (repl_offsets[i + 1] < repl_offsets[i]) { set_error("repl_offsets decrease at replacement " + std::to_string(i)); return DAAC_ERR_INVALID_ARGUMENT; }
    if (!repl && repl_offsets[n_repl] != repl_offsets[0]) { set_error("repl is NULL"); return DAAC_ERR_INVALID_ARGUMENT; }
    if (repl_offsets[n_repl] >= (1ull << 32)) { set_error("the replacements' bytes end at 4 GiB or beyond"); return DAAC_ERR_INVALID_ARGUMENT; }
    if (mode == DAAC_FIND_OVERLAPPING || mode == DAAC_FIND_OVERLAPPING_NO_SUFFIX) {
        set_error("replace_all serves DAAC_FIND and DAAC_LEFTMOST_FIND: overlapping matches have no splice");
        return DAAC_ERR_UNSUPPORTED;
    }
    return check_mode_kind(pma, mode);
}

// The splice of `text` (device, `len` bytes) with the k tuples of `tl`; a batch (n_docs != 0) also gets its out_offsets.
daac_status splice(DeviceTables *t, const uint8_t *text, uint64_t len, TupleList &tl, uint64_t k, const unsigned long long *d_doc_off, uint64_t n_docs,
                   const uint8_t *repl, const uint64_t *repl_offsets, size_t n_repl, hipStream_t stream, uint8_t **dev_out, uint64_t **dev_out_offsets,
                   uint64_t *out_len) {
    ReplaceArgs a{};
    a.hay = text;
    a.len = len;
    a.seg = static_cast<uint4 *>(tl.list);
    a.k = k;
    a.n_repl = n_repl;
    a.doc_first = reinterpret_cast<const unsigned long long *>(tl.doc_first);
    a.doc_off = d_doc_off;
    a.n_docs = n_docs;
    // the replacements: offsets, then the bytes [repl_offsets[0], repl_offsets[n_repl]) at their own positions
    const uint64_t blob_end = repl_offsets[n_repl];
    DevBuf rbuf;
    HIP_TRY(rbuf.alloc((n_repl + 1) * sizeof(uint64_t) + blob_end, stream));
    HIP_TRY(hipMemcpyAsync(rbuf.p, repl_offsets, (n_repl + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, stream));
    a.roff = static_cast<const unsigned long long *>(rbuf.p);
    a.repl = static_cast<const uint8_t *>(rbuf.p) + (n_repl + 1) * sizeof(uint64_t);
    a.repl_bytes = blob_end;
    if (blob_end > repl_offsets[0])
        HIP_TRY(hipMemcpyAsync(const_cast<uint8_t *>(a.repl) + repl_offsets[0], repl + repl_offsets[0], blob_end - repl_offsets[0], hipMemcpyHostToDevice, stream));
    // sizing: {first bad match, sum of match lengths, sum of replacement lengths}, the two arrays of k + 1 sums, the scans' scratch
    const uint64_t m = k + 1;
    DevBuf work;
    HIP_TRY(work.alloc((4 + 2 * m + exclusive_scan_scratch(m)) * sizeof(unsigned long long), stream));
    unsigned long long *hdr = static_cast<unsigned long long *>(work.p);
    a.bad = hdr;
    a.rpre = hdr + 4;
    a.lpre = a.rpre + m;
    unsigned long long *scan_scratch = a.lpre + m;
    HIP_TRY(hipMemsetAsync(hdr, 0xff, sizeof(unsigned long long), stream));
    HIP_TRY(launch_replace_size(a, stream));
    HIP_TRY(launch_exclusive_scan(a.lpre, m, hdr + 1, scan_scratch, stream));
    HIP_TRY(launch_exclusive_scan(a.rpre, m, hdr + 2, scan_scratch, stream));
    unsigned long long *pin = reinterpret_cast<unsigned long long *>(pinned_words());
    unsigned long long local[3];
    unsigned long long *h = pin ? pin : local;
    HIP_TRY(hipMemcpyAsync(h, hdr, 3 * sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    const uint64_t bad = h[0], sum_l = h[1], sum_r = h[2];
    if (bad != kNone) {
        daac_match16 mt{};
        HIP_TRY(hipMemcpyAsync(&mt, a.seg + bad, sizeof(mt), hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        set_error("match " + std::to_string(bad) + " (start " + std::to_string(mt.end - mt.length) + (n_docs ? " in its document" : "") + ") has value " +
                  std::to_string(mt.value) + ": there are " + std::to_string(n_repl) + " replacements");
        return DAAC_ERR_INVALID_ARGUMENT;
    }
    if (sum_l > len) { set_error("the match list covers more bytes than the text has"); return DAAC_ERR_DEVICE; }   // (not ordered and disjoint: never seen)
    const uint64_t total = len - sum_l + sum_r;
    if (total > static_cast<uint64_t>(OPT(max_result_bytes))) {
        set_error("the result of " + std::to_string(total) + " bytes exceeds max_result_bytes");
        return DAAC_ERR_AUTOMATON_SCALE;
    }
    unsigned long long *out_offsets = nullptr;
    if (n_docs) {
        HIP_TRY(dev_malloc(reinterpret_cast<void **>(&out_offsets), (n_docs + 1) * sizeof(unsigned long long), stream));
        HIP_TRY(launch_replace_doc_offsets(a, out_offsets, stream));
    }
    DevPtr off_guard = dev_guard(out_offsets, stream);
    void *out = nullptr;
    DevBuf tiles;
    if (total) {
        a.tiles = (total + kSpliceTile - 1) / kSpliceTile;
        HIP_TRY(dev_malloc(&out, (total + 15) & ~15ull, stream));
    }
    DevPtr out_guard = dev_guard(out, stream);
    if (total) {
        HIP_TRY(tiles.alloc((a.tiles + 1) * sizeof(long long), stream));
        a.tile_lo = static_cast<long long *>(tiles.p);
        a.out = static_cast<uint8_t *>(out);
        a.out_len = total;
        HIP_TRY(launch_replace_finish(a, stream));
        HIP_TRY(launch_replace_splice(a, static_cast<uint32_t>(t->num_cu), stream));
    }
    HIP_TRY(hipStreamSynchronize(stream));   // the call's scratch is released next; the result is the caller's from here
    g_last_kernel = "replace matches=" + std::to_string(k) + " out=" + std::to_string(total) + " " + g_last_kernel;
    *dev_out = static_cast<uint8_t *>(out_guard.release());
    if (dev_out_offsets) *dev_out_offsets = reinterpret_cast<uint64_t *>(off_guard.release());
    *out_len = total;
    return DAAC_OK;
}

}  // namespace

extern "C" {

daac_status daac_replace_all(daac_pma *pma, int mode, int engine, const uint8_t *hay, size_t len, int hay_is_device, void *stream_, const uint8_t *repl,
                             const uint64_t *repl_offsets, size_t n_repl, uint8_t **dev_out, uint64_t *out_len, uint64_t *n_replaced) {
    PmaScope scope_(pma);
    daac_status st = replace_precheck(pma, mode, repl, repl_offsets, n_repl, dev_out && out_len && n_replaced);
    if (st != DAAC_OK) return st;
    if (len && !hay) { set_error("hay is NULL"); return DAAC_ERR_INVALID_ARGUMENT; }
    *dev_out = nullptr;
    *out_len = 0;
    *n_replaced = 0;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    DeviceTables *t = nullptr;
    if ((st = get_tables(pma, &t)) != DAAC_OK) return st;
    void *staged = nullptr;
    const uint8_t *text = hay;
    if (!hay_is_device && len) {   // the splice reads the text on the device: the whole haystack, once
        if ((st = stage_window(hay, 0, len, stream, &staged, &text)) != DAAC_OK) return st;
    }
    std::unique_ptr<void, void (*)(void *)> g1(staged, [](void *p) { if (p) (void)hipFree(p); });
    TupleList tl(stream);
    uint64_t k = 0;
    g_last_kernel.clear();   // (the single-haystack tuple call names no kernel: without this the line below kept every earlier call's line behind it)
    if ((st = daac_scan_device16(pma, mode, engine, len ? text : nullptr, len, 1, stream_, reinterpret_cast<daac_match16 **>(&tl.list), &k)) != DAAC_OK) return st;
    if ((st = splice(t, text, len, tl, k, nullptr, 0, repl, repl_offsets, n_repl, stream, dev_out, nullptr, out_len)) != DAAC_OK) return st;
    *n_replaced = k;
    return DAAC_OK;
}

daac_status daac_replace_all_batch(daac_pma *pma, int mode, int engine, const uint8_t *hay, const uint64_t *offsets, size_t n, int hay_is_device, void *stream_,
                                   const uint8_t *repl, const uint64_t *repl_offsets, size_t n_repl, uint8_t **dev_out, uint64_t **dev_out_offsets,
                                   uint64_t *out_len, uint64_t *n_replaced) {
    PmaScope scope_(pma);
    daac_status st = replace_precheck(pma, mode, repl, repl_offsets, n_repl, dev_out && dev_out_offsets && out_len && n_replaced);
    if (st != DAAC_OK) return st;
    if ((st = check_batch_args(hay, offsets, n, hay_is_device)) != DAAC_OK) return st;
    *dev_out = nullptr;
    *dev_out_offsets = nullptr;
    *out_len = 0;
    *n_replaced = 0;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    TupleList tl(stream);
    uint64_t k = 0;
    if (n == 0) {   // nothing to replace: the tuple call's one offset, 0, is this call's
        if ((st = daac_scan_batch_device16(pma, mode, engine, hay, offsets, 0, hay_is_device, stream_, reinterpret_cast<daac_match16 **>(&tl.list), &tl.doc_first, &k)) != DAAC_OK) return st;
        *dev_out_offsets = tl.doc_first;
        tl.doc_first = nullptr;
        g_last_kernel = "replace matches=0 out=0 " + g_last_kernel;
        return DAAC_OK;
    }
    DeviceTables *t = nullptr;
    if ((st = get_tables(pma, &t)) != DAAC_OK) return st;
    StagedBatch b;   // a decreasing pair between the ends is the tuple call's to refuse
    if ((st = stage_batch(hay, offsets, n, hay_is_device, stream, BatchCheck::ends, b)) != DAAC_OK) return st;
    if ((st = daac_scan_batch_device16(pma, mode, engine, b.dev_hay, reinterpret_cast<const uint64_t *>(b.d_off), n, 1, stream_,
                                       reinterpret_cast<daac_match16 **>(&tl.list), &tl.doc_first, &k)) != DAAC_OK) return st;
    if ((st = splice(t, b.dev_hay + b.ends[0], b.ends[1] - b.ends[0], tl, k, b.d_off, n, repl, repl_offsets, n_repl, stream, dev_out, dev_out_offsets, out_len)) != DAAC_OK) return st;
    *n_replaced = k;
    return DAAC_OK;
}

}  // extern "C"
