// C ABI (include/daachorse_amd.h), part 14: a per-code-point rewrite of a text or a batch on the device (daac_normalizer_create,
// daac_normalize_batch, daac_normalize) and the way back from spans over the rewritten text to spans over the input (daac_spans_to_source).
// No automaton is involved: a normalizer is a list of rules over code points and a pool of replacement bytes.  This file validates its
// own arguments, builds the two-stage table on the host, uploads it per device on first use, marks the document starts (the splitter's
// pass), runs the count pass, sums the tile counts (one read-back), allocates the result and runs the write pass; the kernels are
// normalize_kernels.hip.  The batch arguments' rules, the staging of a host text, the validation of device offsets and the single haystack
// as a batch of one document are the batch front door's (api_internal.hpp, "api_batch.hip").
#include "api_internal.hpp"
#include "normalize.hpp"
#include "split.hpp"

struct daac_normalizer {
    std::vector<uint32_t> ascii;    // 128 entries
    std::vector<uint16_t> stage1;   // kNormStage1 block numbers
    std::vector<uint32_t> stage2;   // blocks of kNormBlock entries; block 0 is all copies
    std::vector<uint8_t> pool;
    size_t n_rules = 0;
    std::mutex mu;
    std::map<int, void *> dev;      // per device: ascii, stage2, stage1, pool in one block
};

namespace {

constexpr uint64_t kSrcLimit = 0xFFFFFFFFull;   // with src a document has fewer bytes than this

daac_status table_of(daac_normalizer *nz, daac::NormTable &out) {
    int device = 0;
    HIP_TRY(hipGetDevice(&device));
    std::lock_guard<std::mutex> g(nz->mu);
    const size_t b_ascii = nz->ascii.size() * sizeof(uint32_t), b2 = nz->stage2.size() * sizeof(uint32_t), b1 = nz->stage1.size() * sizeof(uint16_t);
    auto it = nz->dev.find(device);
    if (it == nz->dev.end()) {
        void *d = nullptr;
        HIP_TRY(hipMalloc(&d, b_ascii + b2 + b1 + nz->pool.size() + 16));
        std::unique_ptr<void, void (*)(void *)> guard(d, [](void *p) { (void)hipFree(p); });
        uint8_t *at = static_cast<uint8_t *>(d);
        HIP_TRY(hipMemcpy(at, nz->ascii.data(), b_ascii, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(at + b_ascii, nz->stage2.data(), b2, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(at + b_ascii + b2, nz->stage1.data(), b1, hipMemcpyHostToDevice));
        if (!nz->pool.empty()) HIP_TRY(hipMemcpy(at + b_ascii + b2 + b1, nz->pool.data(), nz->pool.size(), hipMemcpyHostToDevice));
        it = nz->dev.emplace(device, guard.release()).first;
    }
    const uint8_t *at = static_cast<const uint8_t *>(it->second);
    out.ascii = reinterpret_cast<const uint32_t *>(at);
    out.stage2 = reinterpret_cast<const uint32_t *>(at + b_ascii);
    out.stage1 = reinterpret_cast<const uint16_t *>(at + b_ascii + b2);
    out.pool = at + b_ascii + b2 + b1;
    return DAAC_OK;
}

daac_status too_long_for_src(uint64_t len) {
    set_error("a document of " + std::to_string(len) + " bytes: with src a document has fewer than 2^32 - 1");
    return DAAC_ERR_UNSUPPORTED;
}

std::string kernel_line(const daac_normalizer *nz, uint64_t n, uint64_t total, uint64_t out_len, bool src) {
    return "normalize rules=" + std::to_string(nz->n_rules) + " docs=" + std::to_string(n) + " bytes=" + std::to_string(total) + " out=" + std::to_string(out_len) +
           " src=" + (src ? "1" : "0");
}

// `text`: the byte at offsets[0] on the device; `d_off`: the n + 1 offsets on the device (n >= 1, checked); ends = {offsets[0], offsets[n]}.
daac_status normalize_device(daac_normalizer *nz, const uint8_t *text, const uint64_t ends[2], const unsigned long long *d_off, uint64_t n, hipStream_t stream,
                             bool want_src, uint8_t **dev_out, uint64_t **dev_out_offsets, uint32_t **dev_src, uint64_t *out_len) {
    const uint64_t total = ends[1] - ends[0];
    const uint64_t max_bytes = static_cast<uint64_t>(OPT(max_result_bytes));
    if (n + 1 > max_bytes / sizeof(uint64_t)) { set_error("out_offsets of " + std::to_string(n) + " documents exceeds max_result_bytes"); return DAAC_ERR_AUTOMATON_SCALE; }
    void *out_offsets = nullptr;
    HIP_TRY(dev_malloc(&out_offsets, (n + 1) * sizeof(uint64_t), stream));
    auto g_off = dev_guard(out_offsets, stream);
    if (total == 0) {   // documents, all of them empty: no byte
        void *out = nullptr, *src = nullptr;
        HIP_TRY(dev_malloc(&out, 0, stream));
        auto g_out = dev_guard(out, stream);
        if (want_src) HIP_TRY(dev_malloc(&src, 0, stream));
        auto g_src = dev_guard(src, stream);
        HIP_TRY(hipMemsetAsync(out_offsets, 0, (n + 1) * sizeof(uint64_t), stream));
        HIP_TRY(hipStreamSynchronize(stream));
        g_last_kernel = kernel_line(nz, n, 0, 0, want_src);
        *dev_out = static_cast<uint8_t *>(g_out.release());
        *dev_out_offsets = static_cast<uint64_t *>(g_off.release());
        if (want_src) *dev_src = static_cast<uint32_t *>(g_src.release());
        *out_len = 0;
        return DAAC_OK;
    }
    daac::NormArgs a{};
    daac_status st = table_of(nz, a.tab);
    if (st != DAAC_OK) return st;
    a.text = text;
    a.total = total;
    a.base = ends[0];
    a.doc_off = d_off;
    a.n_docs = n;
    a.tiles = (total + daac::kNormTile - 1) / daac::kNormTile;
    // the scratch: the tile counts, their sum, the sum's scratch, the marks, the longest document
    const uint64_t n_mark = a.tiles * (daac::kNormTile / 32) + 1, n_scan = exclusive_scan_scratch(a.tiles);
    DevBuf work;
    HIP_TRY(work.alloc((a.tiles + 2 + n_scan) * sizeof(unsigned long long) + n_mark * sizeof(uint32_t), stream));
    a.counts = static_cast<unsigned long long *>(work.p);
    unsigned long long *sum = a.counts + a.tiles, *longest = sum + 1, *scan_scratch = longest + 1;
    uint32_t *marks = reinterpret_cast<uint32_t *>(scan_scratch + n_scan);
    a.out_len = sum;
    a.marks = marks;
    HIP_TRY(hipMemsetAsync(longest, 0, sizeof(unsigned long long), stream));
    HIP_TRY(hipMemsetAsync(marks, 0, n_mark * sizeof(uint32_t), stream));
    daac::SplitArgs m{};   // the splitter's mark pass: it reads these fields and no other
    m.total = total;
    m.base = ends[0];
    m.doc_off = d_off;
    m.n_docs = n;
    m.marks = marks;
    HIP_TRY(daac::launch_split_marks(m, stream));
    if (want_src && total >= kSrcLimit) HIP_TRY(daac::launch_normalize_longest(d_off, n, longest, stream));
    HIP_TRY(daac::launch_normalize_count(a, stream));
    HIP_TRY(daac::launch_exclusive_scan(a.counts, a.tiles, sum, scan_scratch, stream));
    unsigned long long h[2] = {0, 0};   // the output's bytes, the longest document's
    HIP_TRY(hipMemcpyAsync(h, sum, sizeof(h), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    if (h[1] >= kSrcLimit) return too_long_for_src(h[1]);
    const uint64_t bytes = h[0];
    if (bytes > max_bytes || (want_src && bytes > max_bytes / 5)) {
        set_error("the output of " + std::to_string(bytes) + " bytes" + (want_src ? " with its src" : "") + " exceeds max_result_bytes");
        return DAAC_ERR_AUTOMATON_SCALE;
    }
    void *out = nullptr, *src = nullptr;
    HIP_TRY(dev_malloc(&out, bytes, stream));
    auto g_out = dev_guard(out, stream);
    if (want_src) HIP_TRY(dev_malloc(&src, bytes * sizeof(uint32_t), stream));
    auto g_src = dev_guard(src, stream);
    a.out = static_cast<uint8_t *>(out);
    a.src = static_cast<uint32_t *>(src);
    a.out_offsets = static_cast<unsigned long long *>(out_offsets);
    HIP_TRY(daac::launch_normalize_write(a, stream));
    HIP_TRY(hipStreamSynchronize(stream));   // the call's scratch is released next; the result is the caller's from here
    g_last_kernel = kernel_line(nz, n, total, bytes, want_src) + " tile=" + std::to_string(daac::kNormTile);
    *dev_out = static_cast<uint8_t *>(g_out.release());
    *dev_out_offsets = static_cast<uint64_t *>(g_off.release());
    if (want_src) *dev_src = static_cast<uint32_t *>(g_src.release());
    *out_len = bytes;
    return DAAC_OK;
}

}  // namespace

extern "C" {

daac_status daac_normalizer_create(const daac_norm_rule *rules, size_t n_rules, const uint8_t *pool, size_t pool_len, daac_normalizer **out) {
    if (!out) { set_error("null argument"); return DAAC_ERR_INVALID_ARGUMENT; }
    *out = nullptr;
    if (n_rules && !rules) { set_error("rules is NULL with n_rules = " + std::to_string(n_rules)); return DAAC_ERR_INVALID_ARGUMENT; }
    if (pool_len && !pool) { set_error("pool is NULL with pool_len = " + std::to_string(pool_len)); return DAAC_ERR_INVALID_ARGUMENT; }
    if (pool_len > daac::kNormMaxPool) { set_error("the pool has more than " + std::to_string(daac::kNormMaxPool) + " bytes"); return DAAC_ERR_INVALID_ARGUMENT; }
    for (size_t i = 0; i < n_rules; ++i) {
        const daac_norm_rule &r = rules[i];
        const std::string at = "rule " + std::to_string(i);
        if (r.last < r.first) { set_error(at + ": last < first"); return DAAC_ERR_INVALID_ARGUMENT; }
        if (r.last > 0x10FFFFu) { set_error(at + ": last is above U+10FFFF"); return DAAC_ERR_INVALID_ARGUMENT; }
        if (i && r.first <= rules[i - 1].last) { set_error(at + ": the rules are not sorted and disjoint"); return DAAC_ERR_INVALID_ARGUMENT; }
        if (r.kind < DAAC_NORM_DELETE || r.kind > DAAC_NORM_HANGUL) { set_error(at + ": kind is none of DAAC_NORM_DELETE, _REPLACE, _PAD and _HANGUL"); return DAAC_ERR_INVALID_ARGUMENT; }
        if (r.kind == DAAC_NORM_REPLACE) {
            if (r.len > daac::kNormMaxLen) { set_error(at + ": len is above " + std::to_string(daac::kNormMaxLen)); return DAAC_ERR_INVALID_ARGUMENT; }
            if (static_cast<uint64_t>(r.off) + r.len > pool_len) { set_error(at + ": off + len is beyond the pool"); return DAAC_ERR_INVALID_ARGUMENT; }
            if (r.first == r.last && r.first >= 0xD800u && r.first <= 0xDFFFu) { set_error(at + ": a surrogate has no UTF-8 sequence"); return DAAC_ERR_INVALID_ARGUMENT; }
        }
        if (r.kind == DAAC_NORM_HANGUL && (r.first < daac::kHangulFirst || r.last > daac::kHangulLast)) {
            set_error(at + ": DAAC_NORM_HANGUL outside U+AC00 .. U+D7A3");
            return DAAC_ERR_INVALID_ARGUMENT;
        }
    }
    auto entry_of = [](const daac_norm_rule &r) { return r.kind == DAAC_NORM_REPLACE ? r.kind | r.len << 3 | r.off << 11 : r.kind; };
    // the two-stage table: equal blocks of 256 code points are stored once
    std::unique_ptr<daac_normalizer> nz(new daac_normalizer);
    nz->n_rules = n_rules;
    nz->pool.assign(pool, pool + pool_len);
    nz->ascii.assign(128, 0);
    nz->stage1.assign(daac::kNormStage1, 0);
    nz->stage2.assign(daac::kNormBlock, 0);
    std::map<std::vector<uint32_t>, uint16_t> seen;
    seen.emplace(nz->stage2, 0);
    size_t r = 0;
    for (uint32_t hi = 0; hi < daac::kNormStage1; ++hi) {
        const uint32_t lo_cp = hi << 8, hi_cp = lo_cp + 255u;
        while (r < n_rules && rules[r].last < lo_cp) ++r;
        if (r == n_rules || rules[r].first > hi_cp) continue;   // all copies: block 0
        std::vector<uint32_t> blk(daac::kNormBlock, 0);
        for (size_t j = r; j < n_rules && rules[j].first <= hi_cp; ++j)
            for (uint32_t cp = std::max(rules[j].first, lo_cp); cp <= std::min(rules[j].last, hi_cp); ++cp) blk[cp & 255u] = entry_of(rules[j]);
        if (hi == 0) std::copy(blk.begin(), blk.begin() + 128, nz->ascii.begin());
        auto it = seen.find(blk);
        if (it == seen.end()) {
            it = seen.emplace(blk, static_cast<uint16_t>(seen.size())).first;   // (at most kNormStage1 blocks: 16 bits hold the number)
            nz->stage2.insert(nz->stage2.end(), blk.begin(), blk.end());
        }
        nz->stage1[hi] = it->second;
    }
    *out = nz.release();
    return DAAC_OK;
}

void daac_normalizer_free(daac_normalizer *nz) {
    if (!nz) return;
    for (auto &kv : nz->dev) (void)hipFree(kv.second);
    delete nz;
}

size_t daac_normalizer_table_bytes(const daac_normalizer *nz) {
    return nz ? nz->ascii.size() * sizeof(uint32_t) + nz->stage1.size() * sizeof(uint16_t) + nz->stage2.size() * sizeof(uint32_t) + nz->pool.size() : 0;
}

daac_status daac_normalize_batch(daac_normalizer *nz, const uint8_t *hay, const uint64_t *offsets, size_t n, int hay_is_device, void *stream_, int want_src,
                                 uint8_t **dev_out, uint64_t **dev_out_offsets, uint32_t **dev_src, uint64_t *out_len) {
    PmaScope scope_(nullptr);   // no handle: the process-wide options
    if (!nz || !dev_out || !dev_out_offsets || !out_len || (want_src && !dev_src)) { set_error("null argument"); return DAAC_ERR_INVALID_ARGUMENT; }
    daac_status st = check_batch_args(hay, offsets, n, hay_is_device);   // status 1 before a device is touched
    if (st != DAAC_OK) return st;
    *dev_out = nullptr;
    *dev_out_offsets = nullptr;
    if (dev_src) *dev_src = nullptr;
    *out_len = 0;
    LongDoc over;   // (device offsets: normalize_device's longest-document pass)
    if (want_src && !hay_is_device) (void)first_doc_over(kSrcLimit - 1, offsets, n, nullptr, nullptr, over);
    if (over) return too_long_for_src(over.len);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (n == 0) {   // no document: no byte and one offset, 0
        void *out = nullptr, *src = nullptr;
        HIP_TRY(dev_malloc(&out, 0, stream));
        auto g_out = dev_guard(out, stream);
        DevPtr g_oo;
        if ((st = zero_word(stream, g_oo)) != DAAC_OK) return st;
        if (want_src) HIP_TRY(dev_malloc(&src, 0, stream));
        auto g_src = dev_guard(src, stream);
        HIP_TRY(hipStreamSynchronize(stream));
        g_last_kernel = kernel_line(nz, 0, 0, 0, want_src != 0);
        *dev_out = static_cast<uint8_t *>(g_out.release());
        *dev_out_offsets = static_cast<uint64_t *>(g_oo.release());
        if (want_src) *dev_src = static_cast<uint32_t *>(g_src.release());
        return DAAC_OK;
    }
    StagedBatch b;   // the passes read what the offsets say: device offsets are validated first
    if ((st = stage_batch(hay, offsets, n, hay_is_device, stream, BatchCheck::kernel, b)) != DAAC_OK) return st;
    return normalize_device(nz, b.dev_hay + b.ends[0], b.ends, b.d_off, n, stream, want_src != 0, dev_out, dev_out_offsets, dev_src, out_len);
}

daac_status daac_normalize(daac_normalizer *nz, const uint8_t *hay, size_t len, int hay_is_device, void *stream_, int want_src, uint8_t **dev_out,
                           uint32_t **dev_src, uint64_t *out_len) {
    if (!nz || !dev_out || !out_len || (want_src && !dev_src)) { set_error("null argument"); return DAAC_ERR_INVALID_ARGUMENT; }
    if (len && !hay) { set_error("hay is NULL"); return DAAC_ERR_INVALID_ARGUMENT; }
    *dev_out = nullptr;
    if (dev_src) *dev_src = nullptr;
    *out_len = 0;
    if (want_src && len >= kSrcLimit) return too_long_for_src(len);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    PmaScope scope_(nullptr);
    StagedBatch b;
    daac_status st = stage_one(hay, len, hay_is_device, stream, b);
    if (st != DAAC_OK) return st;
    uint64_t *out_offsets = nullptr;
    st = normalize_device(nz, b.dev_hay, b.ends, b.d_off, 1, stream, want_src != 0, dev_out, &out_offsets, dev_src, out_len);
    dev_free(out_offsets, stream);
    return st;
}

daac_status daac_spans_to_source(uint64_t *dev_spans, const uint64_t *dev_tok_offsets, const uint64_t *dev_out_offsets, const uint32_t *dev_src, const uint8_t *hay,
                                 const uint64_t *offsets, size_t n, size_t n_tokens, int hay_is_device, void *stream_) {
    if (n_tokens && (!dev_spans || !dev_tok_offsets || !dev_out_offsets || !dev_src)) { set_error("null argument"); return DAAC_ERR_INVALID_ARGUMENT; }
    daac_status st = check_batch_args(hay, offsets, n, hay_is_device);
    if (st != DAAC_OK) return st;
    if (n_tokens && !n) { set_error("tokens without a document"); return DAAC_ERR_INVALID_ARGUMENT; }
    if (!n_tokens) return DAAC_OK;
    PmaScope scope_(nullptr);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    StagedBatch b;   // (device offsets are those the normalized batch was made from: validated then)
    if ((st = stage_batch(hay, offsets, n, hay_is_device, stream, BatchCheck::none, b)) != DAAC_OK) return st;
    HIP_TRY(daac::launch_spans_to_source(reinterpret_cast<unsigned long long *>(dev_spans), reinterpret_cast<const unsigned long long *>(dev_tok_offsets),
                                         reinterpret_cast<const unsigned long long *>(dev_out_offsets), dev_src, b.dev_hay, b.d_off, n, n_tokens, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    return DAAC_OK;
}

}  // extern "C"
