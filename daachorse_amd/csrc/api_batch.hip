// C ABI (include/daachorse_amd.h), part 6: batches — many independent documents in one call (daac_scan_count_batch,
// daac_scan_batch_device16, daac_scan_histogram_batch).  The kernels are batch_kernels.hip and batch_hist_kernels.hip; this file
// validates, stages host haystacks in windows of whole documents, routes the documents the chain modes cannot give one lane to the
// single-haystack path, and assembles the results.  It also holds the front door the other batch calls share (api_internal.hpp, "api_batch.hip";
// DESIGN.md, "The batch front door"): the argument rules, the staging of a batch in one piece, the per-document length limit and the
// single haystack as a batch of one.
#include "api_internal.hpp"
#include "batch.hpp"

namespace daac {
namespace api {

daac_status offsets_decrease(uint64_t doc) {
    set_error("offsets decrease at document " + std::to_string(doc));
    return DAAC_ERR_INVALID_ARGUMENT;
}

daac_status check_batch_args(const uint8_t *hay, const uint64_t *offsets, size_t n, int hay_is_device) {
    if (n && !offsets) { set_error("offsets is NULL with n > 0"); return DAAC_ERR_INVALID_ARGUMENT; }
    if (n && !hay_is_device) {
        for (size_t i = 0; i < n; ++i)
            if (offsets[i + 1] < offsets[i]) return offsets_decrease(i);
        if (!hay && offsets[n] != offsets[0]) { set_error("hay is NULL"); return DAAC_ERR_INVALID_ARGUMENT; }
    }
    if (n && hay_is_device && !hay) { set_error("hay is NULL"); return DAAC_ERR_INVALID_ARGUMENT; }
    return DAAC_OK;
}

daac_status stage_batch(const uint8_t *hay, const uint64_t *offsets, size_t n, int hay_is_device, hipStream_t stream, BatchCheck check, StagedBatch &b) {
    b.dev_hay = hay;
    b.d_off = reinterpret_cast<const unsigned long long *>(offsets);
    if (!hay_is_device) {
        b.ends[0] = offsets[0];
        b.ends[1] = offsets[n];
        const daac_status st = stage_window(hay, b.ends[0], b.ends[1], stream, &b.staged, &b.dev_hay);
        if (st != DAAC_OK) return st;
        HIP_TRY(b.off_buf.alloc((n + 1) * sizeof(uint64_t), stream));
        HIP_TRY(hipMemcpyAsync(b.off_buf.p, offsets, (n + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, stream));
        b.d_off = static_cast<const unsigned long long *>(b.off_buf.p);
    } else if (check == BatchCheck::kernel) {
        HIP_TRY(b.off_buf.alloc(3 * sizeof(unsigned long long), stream));
        unsigned long long *flags = static_cast<unsigned long long *>(b.off_buf.p);
        HIP_TRY(hipMemsetAsync(flags, 0xff, sizeof(unsigned long long), stream));
        HIP_TRY(launch_batch_plan(b.d_off, n, 1, nullptr, flags, stream));
        HIP_TRY(hipMemcpyAsync(flags + 1, b.d_off, sizeof(uint64_t), hipMemcpyDeviceToDevice, stream));
        HIP_TRY(hipMemcpyAsync(flags + 2, b.d_off + n, sizeof(uint64_t), hipMemcpyDeviceToDevice, stream));
        unsigned long long h[3] = {0, 0, 0};
        HIP_TRY(hipMemcpyAsync(h, flags, sizeof(h), hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        if (h[0] != kNoDoc) return offsets_decrease(h[0]);
        b.ends[0] = h[1];
        b.ends[1] = h[2];
    } else if (check == BatchCheck::ends) {
        HIP_TRY(hipMemcpyAsync(&b.ends[0], b.d_off, sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipMemcpyAsync(&b.ends[1], b.d_off + n, sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        if (b.ends[1] < b.ends[0]) { set_error("offsets decrease"); return DAAC_ERR_INVALID_ARGUMENT; }
    }
    return DAAC_OK;
}

daac_status stage_one(const uint8_t *hay, uint64_t len, int hay_is_device, hipStream_t stream, StagedBatch &b) {
    b.dev_hay = hay;
    b.ends[0] = 0;
    b.ends[1] = len;
    if (!hay_is_device && len) {   // the passes read the text on the device: the whole haystack, once
        const daac_status st = stage_window(hay, 0, len, stream, &b.staged, &b.dev_hay);
        if (st != DAAC_OK) return st;
    }
    HIP_TRY(b.off_buf.alloc(2 * sizeof(b.ends), stream));   // the two offsets, and 16 bytes for an empty text to be
    HIP_TRY(hipMemcpyAsync(b.off_buf.p, b.ends, sizeof(b.ends), hipMemcpyHostToDevice, stream));
    b.d_off = static_cast<const unsigned long long *>(b.off_buf.p);
    if (!len) b.dev_hay = static_cast<const uint8_t *>(b.off_buf.p) + sizeof(b.ends);
    return DAAC_OK;
}

daac_status first_doc_over(uint64_t max_len, const uint64_t *offsets, size_t n, const uint64_t *ends, hipStream_t stream, LongDoc &out) {
    std::vector<uint64_t> h;
    if (ends) {
        if (ends[1] - ends[0] <= max_len) return DAAC_OK;
        h.resize(n + 1);
        HIP_TRY(hipMemcpyAsync(h.data(), offsets, (n + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        offsets = h.data();
        for (size_t i = 0; i < n; ++i)
            if (offsets[i + 1] < offsets[i]) return offsets_decrease(i);
    }
    for (size_t i = 0; i < n; ++i)
        if (offsets[i + 1] - offsets[i] > max_len) { out.doc = i; out.len = offsets[i + 1] - offsets[i]; return DAAC_OK; }
    return DAAC_OK;
}

daac_status zero_word(hipStream_t stream, DevPtr &out) {
    void *z = nullptr;
    HIP_TRY(dev_malloc(&z, sizeof(uint64_t), stream));
    out = dev_guard(z, stream);
    HIP_TRY(hipMemsetAsync(z, 0, sizeof(uint64_t), stream));
    return DAAC_OK;
}

}  // namespace api
}  // namespace daac

namespace {

constexpr uint64_t kBatchWindow = 256ull << 20;  // host haystacks: bytes staged to the device at a time (whole documents)
constexpr unsigned long long kNone = ~0ull;

struct BatchPlan {
    bool chain = false, leftmost = false, heads = false, tier = false;
    uint64_t piece = 4096, lane_max = 16384;
    uint32_t halo = 0, threads = 1024;
};

// the engine rules of the single-haystack calls (make_plan), and the batch's own: GRAM and PFX do not serve batches
daac_status batch_engine(const daac_pma *pma, const DeviceTables *t, int mode, int engine, BatchPlan &bp) {
    bp.chain = mode == DAAC_FIND || mode == DAAC_LEFTMOST_FIND;
    bp.leftmost = mode == DAAC_LEFTMOST_FIND;
    bp.heads = mode == DAAC_FIND_OVERLAPPING_NO_SUFFIX;
    if (engine != DAAC_ENGINE_AUTO && engine != DAAC_ENGINE_TIERED && engine != DAAC_ENGINE_DARRAY) {
        set_error(engine == DAAC_ENGINE_GRAM || engine == DAAC_ENGINE_PFX ? "the GRAM and PFX engines do not serve batches (engine AUTO, TIERED or DARRAY)"
                                                                          : "unknown engine");
        return DAAC_ERR_UNSUPPORTED;
    }
    if (pma->charwise && engine == DAAC_ENGINE_TIERED) {
        set_error("charwise automata run on their double array only (engine AUTO or DARRAY)");
        return DAAC_ERR_UNSUPPORTED;
    }
    if (bp.chain && engine == DAAC_ENGINE_TIERED) {
        set_error("find_iter / leftmost_find_iter run on the DARRAY tables only");
        return DAAC_ERR_UNSUPPORTED;
    }
    if (t && engine == DAAC_ENGINE_TIERED && !t->tier_ok) {
        set_error("TIERED engine not available for this automaton (more than 31 distinct pattern bytes, not standard, or dense_depth's rows do not fit lds_budget)");
        return DAAC_ERR_UNSUPPORTED;
    }
    bp.tier = t && !pma->charwise && !bp.chain && (engine == DAAC_ENGINE_TIERED || (engine == DAAC_ENGINE_AUTO && t->tier_ok));
    bp.piece = static_cast<uint64_t>(std::max<int64_t>(64, OPT(batch_piece)));
    bp.lane_max = static_cast<uint64_t>(std::min<int64_t>(std::max<int64_t>(0, OPT(batch_lane_max)), (1ll << 30) - 1));
    bp.halo = pma->halo();
    uint32_t threads = static_cast<uint32_t>(OPT(threads));
    bp.threads = std::min(1024u, std::max(64u, threads & ~63u));
    return DAAC_OK;
}

daac_status note_d(uint64_t doc) {
    set_error("document " + std::to_string(doc) + ": the reference iterator does not terminate on it (leftmost kind, empty pattern, the document ends "
              "inside a pattern)");
    return DAAC_ERR_UNSUPPORTED;
}

// The arguments checked before the device is touched: statuses 1 and 5.
daac_status batch_precheck(const daac_pma *pma, int mode, const uint8_t *hay, const uint64_t *offsets, size_t n, int hay_is_device) {
    if (!pma) { set_error("null handle"); return DAAC_ERR_INVALID_ARGUMENT; }
    if (n && !offsets) { set_error("offsets is NULL with n > 0"); return DAAC_ERR_INVALID_ARGUMENT; }
    daac_status st = check_mode_kind(pma, mode);   // (5 comes between the two kinds of 1: these three calls' documented order)
    if (st != DAAC_OK) return st;
    return check_batch_args(hay, offsets, n, hay_is_device);
}

struct Route { uint64_t pieces = 0, lane_docs = 0, long_docs = 0; };

// Validates device offsets (a decreasing pair: status 1) and, for the overlapping modes, lays out the pieces: first[] (n + 1 entries,
// first[n] = the number of pieces).  One small read-back.
daac_status batch_layout(const BatchPlan &bp, const unsigned long long *d_off, uint64_t n, hipStream_t stream, DevBuf &layout, unsigned long long *&flags,
                         unsigned long long *&first, uint64_t &npieces) {
    const uint64_t m = n + 1;
    HIP_TRY(layout.alloc((4 + (bp.chain ? 0 : m + exclusive_scan_scratch(m))) * sizeof(unsigned long long), stream));
    flags = static_cast<unsigned long long *>(layout.p);   // [0] first decreasing offset, [1] first note D document, [2] pieces
    first = bp.chain ? nullptr : flags + 4;
    HIP_TRY(hipMemsetAsync(flags, 0xff, 2 * sizeof(unsigned long long), stream));
    HIP_TRY(hipMemsetAsync(flags + 2, 0, sizeof(unsigned long long), stream));
    HIP_TRY(launch_batch_plan(d_off, n, bp.piece, first, flags, stream));
    if (first) HIP_TRY(launch_exclusive_scan(first, m, flags + 2, first + m, stream));
    unsigned long long *pin = reinterpret_cast<unsigned long long *>(pinned_words());
    unsigned long long local[3];
    unsigned long long *h = pin ? pin : local;
    HIP_TRY(hipMemcpyAsync(h, flags, 3 * sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    if (h[0] != kNone) return offsets_decrease(h[0]);
    npieces = h[2];
    return DAAC_OK;
}

// the documents the chain modes send through the single-haystack path
daac_status long_docs(const BatchPlan &bp, const unsigned long long *d_off, const uint64_t *h_off, uint64_t n, hipStream_t stream,
                      std::vector<uint64_t> &off_host, std::vector<uint64_t> &longs) {
    if (!h_off) {
        off_host.resize(n + 1);
        HIP_TRY(hipMemcpyAsync(off_host.data(), d_off, (n + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        h_off = off_host.data();
    } else {
        off_host.assign(h_off, h_off + n + 1);
    }
    for (uint64_t i = 0; i < n; ++i)
        if (h_off[i + 1] - h_off[i] > bp.lane_max) longs.push_back(i);
    return DAAC_OK;
}

// counts[i] (and checksums[i]) of documents [0, n) of a device haystack; counts / checksums are device arrays
daac_status count_window(daac_pma *pma, DeviceTables *t, const BatchPlan &bp, int mode, int engine, const uint8_t *hay, const unsigned long long *d_off,
                         const uint64_t *h_off, uint64_t n, hipStream_t stream, unsigned long long *counts, unsigned long long *checksums, Route &route) {
    DevBuf layout;
    unsigned long long *flags = nullptr, *first = nullptr;
    uint64_t npieces = 0;
    daac_status st = batch_layout(bp, d_off, n, stream, layout, flags, first, npieces);
    if (st != DAAC_OK) return st;
    BatchArgs a{};
    a.hay = hay;
    a.off = d_off;
    a.n = n;
    a.first_piece = first;
    a.npieces = npieces;
    a.piece_bytes = bp.piece;
    a.halo = bp.halo;
    a.lane_max = bp.lane_max;
    a.flags = flags;
    DevBuf res;
    if (!bp.chain) {
        HIP_TRY(res.alloc(3 * std::max<uint64_t>(npieces, 1) * sizeof(unsigned long long), stream));
        a.res = static_cast<unsigned long long *>(res.p);
        HIP_TRY(launch_batch_pieces(bp.tier ? &t->tier : nullptr, (!bp.tier && !pma->charwise) ? &t->da : nullptr, pma->charwise ? &t->chr : nullptr, a, 0,
                                    bp.heads, static_cast<uint32_t>(t->num_cu), bp.threads, stream));
        HIP_TRY(launch_batch_reduce(first, a.res, n, counts, checksums, stream));
        route.pieces += npieces;
        route.lane_docs += n;
        return DAAC_OK;
    }
    std::vector<uint64_t> off_host, longs;
    if ((st = long_docs(bp, d_off, h_off, n, stream, off_host, longs)) != DAAC_OK) return st;
    HIP_TRY(res.alloc(3 * std::max<uint64_t>(n, 1) * sizeof(unsigned long long), stream));
    a.res = static_cast<unsigned long long *>(res.p);
    HIP_TRY(hipMemsetAsync(a.res, 0, 3 * n * sizeof(unsigned long long), stream));
    HIP_TRY(launch_batch_chain(pma->charwise ? nullptr : &t->da, pma->charwise ? &t->chr : nullptr, a, 0, bp.leftmost, static_cast<uint32_t>(t->num_cu), stream));
    uint64_t first_d = kNone;
    for (uint64_t i : longs) {   // (each call settles its chain and synchronises: about a call's overhead per document)
        const uint64_t b = off_host[i], len = off_host[i + 1] - b;
        st = daac_scan_count_range(pma, mode, engine, hay + b, len, 0, 1, stream, nullptr, nullptr, reinterpret_cast<uint64_t *>(a.res + 3 * i));
        if (st == DAAC_ERR_UNSUPPORTED && bp.leftmost && pma->root_has_output()) { first_d = i; break; }
        if (st != DAAC_OK) return st;
    }
    HIP_TRY(launch_batch_reduce(nullptr, a.res, n, counts, checksums, stream));
    if (bp.leftmost && pma->root_has_output()) {   // the one request with a document on which the reference does not end
        unsigned long long f = kNone;
        HIP_TRY(hipMemcpyAsync(&f, flags + 1, sizeof(f), hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        if (std::min<uint64_t>(f, first_d) != kNone) return note_d(std::min<uint64_t>(f, first_d));
    }
    route.lane_docs += n - longs.size();
    route.long_docs += longs.size();
    return DAAC_OK;
}

// All tuples of documents [0, n) of a device haystack as one CSR list: *list (16-byte tuples, ends relative to the document), *doc_off
// (n + 1 entries, device), *total.
daac_status tuples_window(daac_pma *pma, DeviceTables *t, const BatchPlan &bp, int mode, int engine, const uint8_t *hay, const unsigned long long *d_off,
                          const uint64_t *h_off, uint64_t n, hipStream_t stream, void **list, unsigned long long **doc_off, uint64_t *total, Route &route) {
    *list = nullptr;
    *doc_off = nullptr;
    *total = 0;
    DevBuf layout;
    unsigned long long *flags = nullptr, *first = nullptr;
    uint64_t npieces = 0;
    daac_status st = batch_layout(bp, d_off, n, stream, layout, flags, first, npieces);
    if (st != DAAC_OK) return st;
    BatchArgs a{};
    a.hay = hay;
    a.off = d_off;
    a.n = n;
    a.first_piece = first;
    a.npieces = npieces;
    a.piece_bytes = bp.piece;
    a.halo = bp.halo;
    a.lane_max = bp.lane_max;
    a.flags = flags;
    // counts per piece (overlapping) or per document (chain), n + 1 / npieces + 1 of them: their exclusive scan is the CSR layout
    const uint64_t units = bp.chain ? n : npieces;
    DevBuf cnt;
    HIP_TRY(cnt.alloc((units + 4 + exclusive_scan_scratch(units + 1)) * sizeof(unsigned long long), stream));
    a.counts = static_cast<unsigned long long *>(cnt.p);
    unsigned long long *d_total = a.counts + units + 1;
    HIP_TRY(hipMemsetAsync(a.counts, 0, (units + 2) * sizeof(unsigned long long), stream));
    const TierDev *tier = bp.tier ? &t->tier : nullptr;
    const DArrayDev *da = (!bp.tier && !pma->charwise) ? &t->da : nullptr;
    const CharDev *chr = pma->charwise ? &t->chr : nullptr;
    std::vector<uint64_t> off_host, longs;
    std::vector<api::DevMatches> long_lists;
    std::vector<unsigned long long> long_counts;
    if (!bp.chain) {
        HIP_TRY(launch_batch_pieces(tier, da, chr, a, 1, bp.heads, static_cast<uint32_t>(t->num_cu), bp.threads, stream));
    } else {
        if ((st = long_docs(bp, d_off, h_off, n, stream, off_host, longs)) != DAAC_OK) return st;
        HIP_TRY(launch_batch_chain(da, chr, a, 1, bp.leftmost, static_cast<uint32_t>(t->num_cu), stream));
        long_lists = std::vector<api::DevMatches>(longs.size());
        long_counts.resize(longs.size());
        uint64_t first_d = kNone;
        for (size_t k = 0; k < longs.size(); ++k) {   // materialised first: their counts enter the scan
            const uint64_t i = longs[k], b = off_host[i], len = off_host[i + 1] - b;
            st = scan_range_device(pma, t, mode, engine, hay + b, 0, len, len, stream, long_lists[k], nullptr);
            if (st == DAAC_ERR_UNSUPPORTED && bp.leftmost && pma->root_has_output()) { first_d = i; break; }
            if (st != DAAC_OK) return st;
            long_counts[k] = long_lists[k].n;
            HIP_TRY(hipMemcpyAsync(a.counts + i, &long_counts[k], sizeof(unsigned long long), hipMemcpyHostToDevice, stream));
        }
        if (bp.leftmost && pma->root_has_output()) {
            unsigned long long f = kNone;
            HIP_TRY(hipMemcpyAsync(&f, flags + 1, sizeof(f), hipMemcpyDeviceToHost, stream));
            HIP_TRY(hipStreamSynchronize(stream));
            if (std::min<uint64_t>(f, first_d) != kNone) return note_d(std::min<uint64_t>(f, first_d));
        }
    }
    HIP_TRY(launch_exclusive_scan(a.counts, units + 1, d_total, d_total + 3, stream));
    unsigned long long tot = 0;
    HIP_TRY(hipMemcpyAsync(&tot, d_total, sizeof(tot), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    if (tot * 16 > static_cast<unsigned long long>(OPT(max_result_bytes))) {
        set_error("match list of " + std::to_string(tot) + " tuples exceeds max_result_bytes");
        return DAAC_ERR_AUTOMATON_SCALE;
    }
    void *out = nullptr;
    unsigned long long *doffs = nullptr;
    HIP_TRY(dev_malloc(&out, std::max<uint64_t>(tot, 1) * 16, stream));
    DevPtr out_guard = dev_guard(out, stream);
    HIP_TRY(dev_malloc(reinterpret_cast<void **>(&doffs), (n + 1) * sizeof(unsigned long long), stream));
    DevPtr off_guard = dev_guard(doffs, stream);
    a.out = static_cast<uint4 *>(out);
    if (!bp.chain) {
        if (tot) HIP_TRY(launch_batch_pieces(tier, da, chr, a, 2, bp.heads, static_cast<uint32_t>(t->num_cu), bp.threads, stream));
        HIP_TRY(launch_batch_doc_offsets(first, a.counts, n, d_total, doffs, stream));
        route.pieces += npieces;
        route.lane_docs += n;
    } else {
        if (tot) HIP_TRY(launch_batch_chain(da, chr, a, 2, bp.leftmost, static_cast<uint32_t>(t->num_cu), stream));
        HIP_TRY(hipMemcpyAsync(doffs, a.counts, (n + 1) * sizeof(unsigned long long), hipMemcpyDeviceToDevice, stream));
        if (!longs.empty()) {   // the long documents' lists into their CSR slots
            std::vector<unsigned long long> at(n + 1);
            HIP_TRY(hipMemcpyAsync(at.data(), a.counts, (n + 1) * sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
            HIP_TRY(hipStreamSynchronize(stream));
            for (size_t k = 0; k < longs.size(); ++k) {
                api::DevMatches &dm = long_lists[k];
                if (dm.n == 0) continue;
                void *dst = static_cast<char *>(out) + at[longs[k]] * 16;
                if (dm.f16_done) HIP_TRY(hipMemcpyAsync(dst, dm.p, dm.n * 16, hipMemcpyDeviceToDevice, stream));
                else HIP_TRY(launch_repack16(dm.p, dst, dm.n, stream));
            }
        }
        route.lane_docs += n - longs.size();
        route.long_docs += longs.size();
    }
    (void)off_guard.release();
    *list = out_guard.release();
    *doc_off = doffs;
    *total = tot;
    return DAAC_OK;
}

// Host haystacks: windows of whole documents [i0, i1) of at most kBatchWindow bytes (a longer document is a window of its own).
template <class F>
daac_status for_windows(const uint8_t *hay, const uint64_t *offsets, uint64_t n, hipStream_t stream, F &&fn) {
    uint64_t i0 = 0;
    while (i0 < n) {
        uint64_t i1 = i0 + 1;
        while (i1 < n && offsets[i1 + 1] - offsets[i0] <= kBatchWindow) ++i1;
        void *staged = nullptr;
        const uint8_t *dev_hay = nullptr;
        daac_status st = stage_window(hay, offsets[i0], offsets[i1], stream, &staged, &dev_hay);
        if (st != DAAC_OK) return st;
        std::unique_ptr<void, void (*)(void *)> g(staged, [](void *p) { if (p) (void)hipFree(p); });
        DevBuf d_off;
        HIP_TRY(d_off.alloc((i1 - i0 + 1) * sizeof(uint64_t), stream));
        HIP_TRY(hipMemcpyAsync(d_off.p, offsets + i0, (i1 - i0 + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, stream));
        if ((st = fn(dev_hay, static_cast<const unsigned long long *>(d_off.p), offsets + i0, i0, i1 - i0)) != DAAC_OK) return st;
        HIP_TRY(hipStreamSynchronize(stream));   // (the window's buffer is freed next)
        i0 = i1;
    }
    return DAAC_OK;
}

// A host batch's CSR result from its windows': fn(window) -> a device list of `elem`-byte entries, its m + 1 offsets and its total.
// One list: the windows' entries back to back, their offsets shifted by the entries before them.
template <class F>
daac_status windows_to_csr(const uint8_t *hay, const uint64_t *offsets, uint64_t n, hipStream_t stream, uint64_t elem, F &&fn, void **list,
                           unsigned long long **doc_off, uint64_t *total) {
    std::vector<std::pair<void *, uint64_t>> parts;
    std::vector<uint64_t> h_doc(n + 1, 0);
    uint64_t tot = 0;
    auto free_parts = [&]() { for (auto &p : parts) dev_free(p.first, stream); parts.clear(); };
    daac_status st = for_windows(hay, offsets, n, stream, [&](const uint8_t *dh, const unsigned long long *d_off, const uint64_t *h_off, uint64_t i0, uint64_t m) {
        void *wl = nullptr;
        unsigned long long *wo = nullptr;
        uint64_t wt = 0;
        daac_status s = fn(dh, d_off, h_off, i0, m, &wl, &wo, &wt);
        if (s != DAAC_OK) return s;
        parts.emplace_back(wl, wt);
        std::vector<uint64_t> w(m + 1);
        hipError_t e = hipMemcpyAsync(w.data(), wo, (m + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, stream);
        if (e == hipSuccess) e = hipStreamSynchronize(stream);
        dev_free(wo, stream);
        if (e != hipSuccess) return hip_fail(e, "batch window offsets");
        for (uint64_t k = 0; k <= m; ++k) h_doc[i0 + k] = tot + w[k];
        tot += wt;
        return DAAC_OK;
    });
    if (st != DAAC_OK) { free_parts(); return st; }
    hipError_t e = dev_malloc(list, std::max<uint64_t>(tot, 1) * elem, stream);
    if (e == hipSuccess) e = dev_malloc(reinterpret_cast<void **>(doc_off), (n + 1) * sizeof(uint64_t), stream);
    uint64_t at = 0;
    for (auto &p : parts) {
        if (e == hipSuccess && p.second) e = hipMemcpyAsync(static_cast<char *>(*list) + at * elem, p.first, p.second * elem, hipMemcpyDeviceToDevice, stream);
        at += p.second;
    }
    if (e == hipSuccess) e = hipMemcpyAsync(*doc_off, h_doc.data(), (n + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);   // (h_doc goes out of scope)
    free_parts();
    if (e != hipSuccess) { dev_free(*list, stream); dev_free(*doc_off, stream); *list = nullptr; *doc_off = nullptr; return hip_fail(e, "batch list assembly"); }
    *total = tot;
    return DAAC_OK;
}

void report(const BatchPlan &bp, const Route &r) {
    g_last_engine = bp.tier ? DAAC_ENGINE_TIERED : DAAC_ENGINE_DARRAY;
    g_last_kernel = "batch pieces=" + std::to_string(r.pieces) + " lane_docs=" + std::to_string(r.lane_docs) + " long_docs=" + std::to_string(r.long_docs);
}

// ---- per-document pattern counts (daac_scan_histogram_batch) ----
struct HistRoute { uint64_t pieces = 0, records = 0, wave_docs = 0, group_docs = 0, dense_docs = 0; };
constexpr uint64_t kHistDocMax = (1ull << 32) - 2;         // longest document: a slot takes one match per position and ROOT's at 0, so a u32 count holds
constexpr uint64_t kHistDenseScratch = 256ull << 20;       // bytes of counter rows the dense route keeps per launch
constexpr uint32_t kHistDenseDocs = 1024;                  // ... and documents per launch at most

uint64_t hist_doc_limit(const BatchPlan &bp) { return bp.chain ? std::min(bp.lane_max, kHistDocMax) : kHistDocMax; }

daac_status hist_doc_too_long(const BatchPlan &bp, uint64_t doc, uint64_t len) {
    if (len > kHistDocMax) {
        set_error("document " + std::to_string(doc) + " has " + std::to_string(len) + " bytes: a per-document count is 32 bits wide (documents below 2^32 - 1 bytes)");
    } else {
        set_error("document " + std::to_string(doc) + " has " + std::to_string(len) + " bytes: find_iter / leftmost_find_iter count a document on one lane, up to option "
                  "batch_lane_max (" + std::to_string(bp.lane_max) + ") bytes; raise the option for longer ones");
    }
    return DAAC_ERR_UNSUPPORTED;
}

// The rows of documents [0, n) of a device haystack as one CSR list: *rows ({slot, count} of 8 bytes), *doc_off (n + 1 entries,
// device), *total.  `doc0` is the call's number of the window's first document (for the messages).
daac_status hist_window(daac_pma *pma, DeviceTables *t, const BatchPlan &bp, const uint8_t *hay, const unsigned long long *d_off, uint64_t n, uint64_t doc0,
                        hipStream_t stream, void **rows, unsigned long long **doc_off, uint64_t *total, HistRoute &route) {
    *rows = nullptr;
    *doc_off = nullptr;
    *total = 0;
    DevBuf layout;
    unsigned long long *flags = nullptr, *first = nullptr;
    uint64_t npieces = 0;
    daac_status st = batch_layout(bp, d_off, n, stream, layout, flags, first, npieces);
    if (st != DAAC_OK) return st;
    BatchArgs a{};
    a.hay = hay;
    a.off = d_off;
    a.n = n;
    a.first_piece = first;
    a.npieces = npieces;
    a.piece_bytes = bp.piece;
    a.halo = bp.halo;
    a.lane_max = bp.lane_max;
    a.flags = flags;
    // 1. matches per piece (overlapping) or per document (chain); their exclusive scan places the records
    const uint64_t units = bp.chain ? n : npieces;
    DevBuf cnt;
    HIP_TRY(cnt.alloc((units + 4 + exclusive_scan_scratch(units + 1)) * sizeof(unsigned long long), stream));
    a.counts = static_cast<unsigned long long *>(cnt.p);
    unsigned long long *d_total = a.counts + units + 1;
    HIP_TRY(hipMemsetAsync(a.counts, 0, (units + 2) * sizeof(unsigned long long), stream));
    const TierDev *tier = bp.tier ? &t->tier : nullptr;
    const DArrayDev *da = (!bp.tier && !pma->charwise) ? &t->da : nullptr;
    const CharDev *chr = pma->charwise ? &t->chr : nullptr;
    if (!bp.chain) HIP_TRY(launch_batch_pieces(tier, da, chr, a, 1, bp.heads, static_cast<uint32_t>(t->num_cu), bp.threads, stream));
    else HIP_TRY(launch_batch_chain(da, chr, a, 1, bp.leftmost, static_cast<uint32_t>(t->num_cu), stream));
    HIP_TRY(launch_exclusive_scan(a.counts, units + 1, d_total, d_total + 3, stream));
    // 2. records per document -> the document's route; the lengths the counts cannot serve
    const uint64_t m = n + 1;
    DevBuf work;   // roff[m] (overlapping modes), rowcnt[m], the rows' total, 3 words of scan scratch head room, cls[4], the two lists, scan scratch
    HIP_TRY(work.alloc(((bp.chain ? 0 : m) + m + 8 + 2 * n + exclusive_scan_scratch(m)) * sizeof(unsigned long long), stream));
    unsigned long long *roff = bp.chain ? a.counts : static_cast<unsigned long long *>(work.p);   // (chain: the scan of n + 1 counts is the layout)
    BatchHistArgs h{};
    h.roff = roff;
    h.n = n;
    h.rowcnt = static_cast<unsigned long long *>(work.p) + (bp.chain ? 0 : m);
    unsigned long long *d_rows_total = h.rowcnt + m;
    h.cls = d_rows_total + 4;
    h.group_list = h.cls + 4;
    h.dense_list = h.group_list + n;
    unsigned long long *scan_scratch = h.dense_list + n;
    h.wave_max = static_cast<uint64_t>(std::min<int64_t>(std::max<int64_t>(0, OPT(batch_hist_wave_max)), kBatchHistWaveCap));
    h.sort_max = static_cast<uint64_t>(std::min<int64_t>(std::max<int64_t>(0, OPT(batch_hist_sort_max)), kBatchHistGroupCap));
    HIP_TRY(hipMemsetAsync(h.cls, 0, 2 * sizeof(unsigned long long), stream));
    HIP_TRY(hipMemsetAsync(h.cls + 2, 0xff, sizeof(unsigned long long), stream));
    if (!bp.chain) HIP_TRY(launch_batch_doc_offsets(first, a.counts, n, d_total, roff, stream));
    HIP_TRY(launch_batch_hist_classify(h, d_off, hist_doc_limit(bp), stream));
    unsigned long long *pin = reinterpret_cast<unsigned long long *>(pinned_words());
    unsigned long long local[5];
    unsigned long long *hw = pin ? pin : local;   // {group docs, dense docs, first too long document, records, first note D document}
    HIP_TRY(hipMemcpyAsync(hw, h.cls, 3 * sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipMemcpyAsync(hw + 3, d_total, sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipMemcpyAsync(hw + 4, flags + 1, sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    const uint64_t group_docs = hw[0], dense_docs = hw[1], too_long = hw[2], tot = hw[3], first_d = hw[4];
    if (too_long != kNone) {
        unsigned long long ends[2] = {0, 0};
        HIP_TRY(hipMemcpyAsync(ends, d_off + too_long, sizeof(ends), hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        return hist_doc_too_long(bp, doc0 + too_long, ends[1] - ends[0]);
    }
    if (bp.leftmost && pma->root_has_output() && first_d != kNone) return note_d(doc0 + first_d);
    if (tot * 8 > static_cast<unsigned long long>(OPT(max_result_bytes))) {
        set_error(std::to_string(tot) + " match records of 8 bytes exceed max_result_bytes");
        return DAAC_ERR_INVALID_AUTOMATON;   // (status 4 is this call's answer; the tuple lists answer 2 for theirs)
    }
    // 3. one record per match, then every document's rows at the front of its records
    DevBuf rec;
    HIP_TRY(rec.alloc(std::max<uint64_t>(tot, 1) * sizeof(unsigned long long), stream));
    a.rec = static_cast<unsigned long long *>(rec.p);
    h.rec = a.rec;
    if (tot) {
        if (!bp.chain) HIP_TRY(launch_batch_pieces(tier, da, chr, a, 3, bp.heads, static_cast<uint32_t>(t->num_cu), bp.threads, stream));
        else HIP_TRY(launch_batch_chain(da, chr, a, 3, bp.leftmost, static_cast<uint32_t>(t->num_cu), stream));
    }
    const uint64_t wave_docs = n - group_docs - dense_docs;
    if (wave_docs) HIP_TRY(launch_batch_hist_sort(h, true, n, static_cast<uint32_t>(t->num_cu), stream));
    HIP_TRY(launch_batch_hist_sort(h, false, group_docs, static_cast<uint32_t>(t->num_cu), stream));
    DevBuf scratch;
    if (dense_docs) {
        const uint64_t slots = pma->charwise ? pma->chost.outputs.size() : pma->host.outputs.size();
        const uint64_t per = std::min<uint64_t>({dense_docs, kHistDenseDocs, std::max<uint64_t>(1, kHistDenseScratch / (4 * std::max<uint64_t>(slots, 1)))});
        HIP_TRY(scratch.alloc(per * slots * sizeof(uint32_t), stream));
        for (uint64_t d0 = 0; d0 < dense_docs; d0 += per) {
            const uint32_t nd = static_cast<uint32_t>(std::min<uint64_t>(per, dense_docs - d0));
            HIP_TRY(hipMemsetAsync(scratch.p, 0, nd * slots * sizeof(uint32_t), stream));
            HIP_TRY(launch_batch_hist_dense(h, static_cast<uint32_t *>(scratch.p), slots, d0, nd, stream));
        }
    }
    // 4. rows per document -> the call's offsets, 5. the rows to their place
    HIP_TRY(launch_exclusive_scan(h.rowcnt, m, d_rows_total, scan_scratch, stream));
    unsigned long long nrows = 0;
    HIP_TRY(hipMemcpyAsync(&nrows, d_rows_total, sizeof(nrows), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    void *out = nullptr;
    unsigned long long *doffs = nullptr;
    HIP_TRY(dev_malloc(&out, std::max<uint64_t>(nrows, 1) * sizeof(daac_slot_count), stream));
    DevPtr out_guard = dev_guard(out, stream);
    HIP_TRY(dev_malloc(reinterpret_cast<void **>(&doffs), m * sizeof(unsigned long long), stream));
    DevPtr off_guard = dev_guard(doffs, stream);
    HIP_TRY(launch_batch_hist_copy(h.rec, roff, h.rowcnt, n, nrows, static_cast<unsigned long long *>(out), stream));
    HIP_TRY(hipMemcpyAsync(doffs, h.rowcnt, m * sizeof(unsigned long long), hipMemcpyDeviceToDevice, stream));
    HIP_TRY(hipStreamSynchronize(stream));   // (the scratch of this window is freed next)
    route.pieces += npieces;
    route.records += tot;
    route.wave_docs += wave_docs;
    route.group_docs += group_docs;
    route.dense_docs += dense_docs;
    (void)off_guard.release();
    *rows = out_guard.release();
    *doc_off = doffs;
    *total = nrows;
    return DAAC_OK;
}

void report_hist(const BatchPlan &bp, const HistRoute &r) {
    g_last_engine = bp.tier ? DAAC_ENGINE_TIERED : DAAC_ENGINE_DARRAY;
    g_last_kernel = "batch_hist pieces=" + std::to_string(r.pieces) + " records=" + std::to_string(r.records) + " wave_docs=" + std::to_string(r.wave_docs) +
                    " group_docs=" + std::to_string(r.group_docs) + " dense_docs=" + std::to_string(r.dense_docs);
}

}  // namespace

extern "C" {

daac_status daac_scan_count_batch(daac_pma *pma, int mode, int engine, const uint8_t *hay, const uint64_t *offsets, size_t n, int hay_is_device,
                                  void *stream_, uint64_t *counts, uint64_t *checksums, int out_is_device) {
    PmaScope scope_(pma);
    daac_status st = batch_precheck(pma, mode, hay, offsets, n, hay_is_device);
    if (st != DAAC_OK) return st;
    if (n && !counts) { set_error("counts is NULL"); return DAAC_ERR_INVALID_ARGUMENT; }
    BatchPlan bp;
    if ((st = batch_engine(pma, nullptr, mode, engine, bp)) != DAAC_OK) return st;
    if (n == 0) { report(bp, Route{}); return DAAC_OK; }
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    DeviceTables *t = nullptr;
    if ((st = get_tables(pma, &t)) != DAAC_OK) return st;
    if ((st = batch_engine(pma, t, mode, engine, bp)) != DAAC_OK) return st;
    unsigned long long *d_counts = reinterpret_cast<unsigned long long *>(counts), *d_sums = reinterpret_cast<unsigned long long *>(checksums);
    DevBuf outs;
    if (!out_is_device) {
        HIP_TRY(outs.alloc(2 * n * sizeof(unsigned long long), stream));
        d_counts = static_cast<unsigned long long *>(outs.p);
        d_sums = checksums ? d_counts + n : nullptr;
    }
    Route route;
    if (hay_is_device) {
        st = count_window(pma, t, bp, mode, engine, hay, reinterpret_cast<const unsigned long long *>(offsets), nullptr, n, stream, d_counts, d_sums, route);
    } else {
        st = for_windows(hay, offsets, n, stream, [&](const uint8_t *dh, const unsigned long long *d_off, const uint64_t *h_off, uint64_t i0, uint64_t m) {
            return count_window(pma, t, bp, mode, engine, dh, d_off, h_off, m, stream, d_counts + i0, d_sums ? d_sums + i0 : nullptr, route);
        });
    }
    if (st != DAAC_OK) return st;
    if (!out_is_device) {
        HIP_TRY(hipMemcpyAsync(counts, d_counts, n * sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
        if (checksums) HIP_TRY(hipMemcpyAsync(checksums, d_sums, n * sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
    }
    report(bp, route);
    return DAAC_OK;
}

daac_status daac_scan_batch_device16(daac_pma *pma, int mode, int engine, const uint8_t *hay, const uint64_t *offsets, size_t n, int hay_is_device,
                                     void *stream_, daac_match16 **dev_out, uint64_t **dev_doc_offsets, uint64_t *total) {
    PmaScope scope_(pma);
    daac_status st = batch_precheck(pma, mode, hay, offsets, n, hay_is_device);
    if (st != DAAC_OK) return st;
    if (!dev_out || !dev_doc_offsets || !total) { set_error("null argument"); return DAAC_ERR_INVALID_ARGUMENT; }
    *dev_out = nullptr;
    *dev_doc_offsets = nullptr;
    *total = 0;
    BatchPlan bp;
    if ((st = batch_engine(pma, nullptr, mode, engine, bp)) != DAAC_OK) return st;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (n == 0) {   // one offset, 0
        DevPtr g_z;
        if ((st = zero_word(stream, g_z)) != DAAC_OK) return st;
        HIP_TRY(hipStreamSynchronize(stream));
        *dev_doc_offsets = static_cast<uint64_t *>(g_z.release());
        report(bp, Route{});
        return DAAC_OK;
    }
    DeviceTables *t = nullptr;
    if ((st = get_tables(pma, &t)) != DAAC_OK) return st;
    if ((st = batch_engine(pma, t, mode, engine, bp)) != DAAC_OK) return st;
    Route route;
    void *list = nullptr;
    unsigned long long *doc_off = nullptr;
    uint64_t tot = 0;
    if (hay_is_device) {
        st = tuples_window(pma, t, bp, mode, engine, hay, reinterpret_cast<const unsigned long long *>(offsets), nullptr, n, stream, &list, &doc_off, &tot, route);
        if (st != DAAC_OK) return st;
    } else {
        st = windows_to_csr(hay, offsets, n, stream, 16, [&](const uint8_t *dh, const unsigned long long *d_off, const uint64_t *h_off, uint64_t, uint64_t m,
                                                            void **wl, unsigned long long **wo, uint64_t *wt) {
            return tuples_window(pma, t, bp, mode, engine, dh, d_off, h_off, m, stream, wl, wo, wt, route);
        }, &list, &doc_off, &tot);
        if (st != DAAC_OK) return st;
    }
    HIP_TRY(hipStreamSynchronize(stream));
    if (tot == 0) { dev_free(list, stream); list = nullptr; HIP_TRY(hipStreamSynchronize(stream)); }
    *dev_out = static_cast<daac_match16 *>(list);
    *dev_doc_offsets = reinterpret_cast<uint64_t *>(doc_off);
    *total = tot;
    report(bp, route);
    return DAAC_OK;
}

static_assert(sizeof(daac_slot_count) == sizeof(unsigned long long), "a row takes a record's place");

daac_status daac_scan_histogram_batch(daac_pma *pma, int mode, int engine, const uint8_t *hay, const uint64_t *offsets, size_t n, int hay_is_device,
                                      void *stream_, daac_slot_count **dev_rows, uint64_t **dev_doc_offsets, uint64_t *total) {
    PmaScope scope_(pma);
    daac_status st = batch_precheck(pma, mode, hay, offsets, n, hay_is_device);
    if (st != DAAC_OK) return st;
    if (!dev_rows || !dev_doc_offsets || !total) { set_error("null argument"); return DAAC_ERR_INVALID_ARGUMENT; }
    *dev_rows = nullptr;
    *dev_doc_offsets = nullptr;
    *total = 0;
    BatchPlan bp;
    if ((st = batch_engine(pma, nullptr, mode, engine, bp)) != DAAC_OK) return st;
    if (n && !hay_is_device) {   // the lengths the counts cannot serve, before a device is touched
        LongDoc over;
        (void)first_doc_over(hist_doc_limit(bp), offsets, n, nullptr, nullptr, over);
        if (over) return hist_doc_too_long(bp, over.doc, over.len);
    }
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (n == 0) {   // one offset, 0
        DevPtr g_z;
        if ((st = zero_word(stream, g_z)) != DAAC_OK) return st;
        HIP_TRY(hipStreamSynchronize(stream));
        *dev_doc_offsets = static_cast<uint64_t *>(g_z.release());
        report_hist(bp, HistRoute{});
        return DAAC_OK;
    }
    DeviceTables *t = nullptr;
    if ((st = get_tables(pma, &t)) != DAAC_OK) return st;
    if ((st = batch_engine(pma, t, mode, engine, bp)) != DAAC_OK) return st;
    HistRoute route;
    void *rows = nullptr;
    unsigned long long *doc_off = nullptr;
    uint64_t tot = 0;
    if (hay_is_device) {
        st = hist_window(pma, t, bp, hay, reinterpret_cast<const unsigned long long *>(offsets), n, 0, stream, &rows, &doc_off, &tot, route);
    } else {
        st = windows_to_csr(hay, offsets, n, stream, sizeof(daac_slot_count), [&](const uint8_t *dh, const unsigned long long *d_off, const uint64_t *, uint64_t i0,
                                                                                 uint64_t m, void **wl, unsigned long long **wo, uint64_t *wt) {
            return hist_window(pma, t, bp, dh, d_off, m, i0, stream, wl, wo, wt, route);
        }, &rows, &doc_off, &tot);
    }
    if (st != DAAC_OK) return st;
    HIP_TRY(hipStreamSynchronize(stream));
    if (tot == 0) { dev_free(rows, stream); rows = nullptr; HIP_TRY(hipStreamSynchronize(stream)); }
    *dev_rows = static_cast<daac_slot_count *>(rows);
    *dev_doc_offsets = reinterpret_cast<uint64_t *>(doc_off);
    *total = tot;
    report_hist(bp, route);
    return DAAC_OK;
}

}  // extern "C"
