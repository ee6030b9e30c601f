// C ABI (include/daachorse_amd.h), part 7: per-pattern match counts of an overlapping scan (daac_pma_outputs, daac_scan_histogram).
// The kernels are hist_kernels.hip; this file validates, cuts the range into launches of fewer than 2^32 bytes (host haystacks: staged
// window by window), folds every launch's 32-bit head counts into the u64 result and, for find_overlapping, propagates the head
// totals down the parent links once per call.
#include "api_internal.hpp"
#include "hist.hpp"

namespace {

constexpr uint64_t kHistLaunchBytes = 1ull << 31;   // device haystacks: bytes per launch (a 32-bit head counter takes one hit per position)
constexpr uint64_t kHistWindow = 256ull << 20;      // host haystacks: bytes staged to the device at a time
static_assert(kHistLaunchBytes < (1ull << 32) && kHistWindow < (1ull << 32), "a launch's range must stay below 2^32 bytes");

const std::vector<OutputRec> &outputs_of(const daac_pma *pma) { return pma->charwise ? pma->chost.outputs : pma->host.outputs; }

// Everything that is decided before a device is touched: statuses 1, 5 and 6.
daac_status hist_precheck(const daac_pma *pma, int mode, int engine, const uint8_t *hay, size_t len, size_t begin, const uint64_t *counts) {
    if (!pma || (len && !hay) || begin > len) { set_error("bad argument"); return DAAC_ERR_INVALID_ARGUMENT; }
    if (!counts && !outputs_of(pma).empty()) { set_error("counts is NULL"); return DAAC_ERR_INVALID_ARGUMENT; }
    if (mode == DAAC_FIND || mode == DAAC_LEFTMOST_FIND) {
        set_error("daac_scan_histogram serves DAAC_FIND_OVERLAPPING and DAAC_FIND_OVERLAPPING_NO_SUFFIX; find_iter / leftmost_find_iter are chains "
                  "through their own matches (their histogram belongs to the chain walkers' emit pass)");
        return DAAC_ERR_UNSUPPORTED;
    }
    const daac_status st = check_mode_kind(pma, mode);
    if (st != DAAC_OK) return st;
    if (engine != DAAC_ENGINE_AUTO && engine != DAAC_ENGINE_TIERED && engine != DAAC_ENGINE_DARRAY) {
        set_error(engine == DAAC_ENGINE_GRAM || engine == DAAC_ENGINE_PFX ? "the GRAM and PFX engines do not serve histograms (engine AUTO, TIERED or DARRAY)"
                                                                          : "unknown engine");
        return DAAC_ERR_UNSUPPORTED;
    }
    if (pma->charwise && engine == DAAC_ENGINE_TIERED) {
        set_error("charwise automata run on their double array only (engine AUTO or DARRAY)");
        return DAAC_ERR_UNSUPPORTED;
    }
    return DAAC_OK;
}

}  // namespace

extern "C" {

size_t daac_pma_outputs(const daac_pma *pma, uint32_t *out, size_t cap) {
    if (!pma) return 0;
    const std::vector<OutputRec> &o = outputs_of(pma);
    static_assert(sizeof(OutputRec) == 3 * sizeof(uint32_t), "{value, length, parent}");
    const size_t n = std::min(cap, o.size());
    if (out && n) std::memcpy(out, o.data(), n * sizeof(OutputRec));
    return o.size();
}

daac_status daac_scan_histogram(daac_pma *pma, int mode, int engine, const uint8_t *hay, size_t len, size_t begin, int hay_is_device, void *stream_,
                                uint64_t *counts, int counts_is_device) {
    PmaScope scope_(pma);
    daac_status st = hist_precheck(pma, mode, engine, hay, len, begin, counts);
    if (st != DAAC_OK) return st;
    const uint64_t n = outputs_of(pma).size();
    if (n == 0) {   // an automaton without patterns: nothing to count, nothing to write
        g_last_kernel = "hist eng=none lds_bins=0";
        return DAAC_OK;
    }
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    DeviceTables *t = nullptr;
    if ((st = get_tables(pma, &t)) != DAAC_OK) return st;

    // the launch shape of the segment scanners for the whole range (and make_plan's engine rules: TIERED where the tables are there)
    Plan pl;
    bool heads_only = false;
    if ((st = make_plan(pma, t, mode, engine, begin, len, pl, heads_only)) != DAAC_OK) return st;
    const TierDev *tier = pl.tier ? &t->tier : nullptr;
    const DArrayDev *da = (!pl.tier && !pma->charwise) ? &t->da : nullptr;
    const CharDev *chr = pma->charwise ? &t->chr : nullptr;
    const uint32_t *d_outputs = tier ? tier->outputs : da ? da->outputs : chr->outputs;

    HistArgs h{};
    h.n = static_cast<uint32_t>(n);
    h.off_bins = hist_engine_lds(tier, da);
    if (h.off_bins > kHistLdsLimit) { set_error("the engine's tables leave no LDS"); return DAAC_ERR_UNSUPPORTED; }
    h.lds_bins = static_cast<uint32_t>(std::min<uint64_t>({static_cast<uint64_t>(std::max<int64_t>(0, OPT(hist_lds_bins))), n, (kHistLdsLimit - h.off_bins) / 4u}));
    const uint32_t lds = std::max(16u, h.off_bins + 4u * h.lds_bins);
    uint32_t bpc = static_cast<uint32_t>(OPT(blocks_per_cu));
    if (bpc == 0) bpc = std::max(1u, std::min(2048u / pl.threads, kHistLdsLimit / lds));
    const uint64_t max_blocks = static_cast<uint64_t>(t->num_cu) * bpc;

    DevBuf heads_buf, counts_buf, snap_buf;
    HIP_TRY(heads_buf.alloc(n * sizeof(uint32_t), stream));
    h.heads = static_cast<uint32_t *>(heads_buf.p);
    HIP_TRY(hipMemsetAsync(h.heads, 0, n * sizeof(uint32_t), stream));
    unsigned long long *d_counts = reinterpret_cast<unsigned long long *>(counts);
    if (!counts_is_device) {
        HIP_TRY(counts_buf.alloc(n * sizeof(unsigned long long), stream));
        d_counts = static_cast<unsigned long long *>(counts_buf.p);
    }
    HIP_TRY(hipMemsetAsync(d_counts, 0, n * sizeof(unsigned long long), stream));

    g_last_engine = pl.tier ? DAAC_ENGINE_TIERED : DAAC_ENGINE_DARRAY;
    g_last_kernel = std::string("hist eng=") + (tier ? "tier" : da ? "darray" : "char") + " lds_bins=" + std::to_string(h.lds_bins);

    // one launch over [b, e) of the haystack whose byte 0 is at `base`, then its head counts into d_counts
    auto scan_piece = [&](const uint8_t *base, uint64_t b, uint64_t e) -> daac_status {
        assert(e - b < (1ull << 32));   // at most one hit per position and slot: a 32-bit head cannot wrap
        Plan pp;
        bool ho = false;
        const daac_status ps = make_plan(pma, t, mode, engine, b, e, pp, ho);
        if (ps != DAAC_OK) return ps;
        if (pp.a.nseg == 0 && b == 0) pp.a.nseg = 1;   // ROOT's list at end = 0
        if (pp.a.nseg == 0) return DAAC_OK;
        pp.a.hay = base;
        const uint32_t blocks = static_cast<uint32_t>(std::max<uint64_t>(1, std::min<uint64_t>(max_blocks, (pp.a.nseg + pp.threads - 1) / pp.threads)));
        HIP_TRY(launch_hist_scan(tier, da, chr, pp.a, h, blocks, pp.threads, stream));
        HIP_TRY(launch_hist_fold(h.heads, d_counts, n, stream));
        return DAAC_OK;
    };

    if (hay_is_device || len == 0) {
        uint64_t b = begin;
        do {
            const uint64_t e = std::min<uint64_t>(len, b + kHistLaunchBytes);
            if ((st = scan_piece(hay, b, e)) != DAAC_OK) return st;
            b = e;
        } while (b < len);
    } else {
        uint64_t b = begin;
        do {
            const uint64_t e = std::min<uint64_t>(len, b + kHistWindow);
            const uint64_t from = b > pl.a.halo ? b - pl.a.halo : 0;
            void *staged = nullptr;
            const uint8_t *base = nullptr;
            if ((st = stage_window(hay, from, e, stream, &staged, &base)) != DAAC_OK) return st;
            std::unique_ptr<void, void (*)(void *)> guard(staged, [](void *p) { if (p) (void)hipFree(p); });
            if ((st = scan_piece(base, b, e)) != DAAC_OK) return st;
            HIP_TRY(hipStreamSynchronize(stream));   // the window goes back before the next one is staged
            b = e;
        } while (b < len);
    }

    if (!heads_only) {   // find_overlapping: every hit reports its whole chain — each head total goes to every ancestor, once
        HIP_TRY(snap_buf.alloc(n * sizeof(unsigned long long), stream));
        HIP_TRY(hipMemcpyAsync(snap_buf.p, d_counts, n * sizeof(unsigned long long), hipMemcpyDeviceToDevice, stream));
        HIP_TRY(launch_hist_propagate(d_outputs, static_cast<const unsigned long long *>(snap_buf.p), d_counts, n, stream));
    }
    if (!counts_is_device) {
        HIP_TRY(hipMemcpyAsync(counts, d_counts, n * sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
    }
    return DAAC_OK;
}

}  // extern "C"
