// C ABI (include/daachorse_amd.h), part 12: the pre-tokenizer split of a text or a batch into words on the device (daac_splitter_create,
// daac_split_batch, daac_split, daac_split_words_space) and the gather that turns offsets over words into offsets over documents (daac_offsets_compose).  No
// automaton is involved: a splitter is a rule and a class table.  This file validates its own arguments, builds the two-stage class table
// on the host, uploads it per device on first use, marks the document starts, runs the flag pass (behind the two scan passes where the
// rule has scans), sums the tile counts (one read-back), allocates the result and runs the write passes; the kernels are
// split_kernels.hip.  The batch arguments' rules, the staging of a host text, the validation of device offsets and the single haystack as
// a batch of one document are the batch front door's (api_internal.hpp, "api_batch.hip").
#include "api_internal.hpp"
#include "split.hpp"

struct daac_splitter {
    int rule = DAAC_SPLIT_GPT2;
    std::vector<uint16_t> stage1;   // kSplitStage1 block numbers
    std::vector<uint8_t> stage2;    // blocks of kSplitBlockBytes (DAAC_SPLIT_O200K: kSplitBlockBytes4, four bits a code point); block 0 is all O
    std::mutex mu;
    std::map<int, void *> dev;      // per device: stage1, then stage2 at byte 2 * kSplitStage1
};

namespace {

daac_status table_of(daac_splitter *sp, daac::SplitTable &out) {
    int device = 0;
    HIP_TRY(hipGetDevice(&device));
    std::lock_guard<std::mutex> g(sp->mu);
    auto it = sp->dev.find(device);
    if (it == sp->dev.end()) {
        void *d = nullptr;
        const size_t b1 = sp->stage1.size() * sizeof(uint16_t);
        HIP_TRY(hipMalloc(&d, b1 + sp->stage2.size()));
        std::unique_ptr<void, void (*)(void *)> guard(d, [](void *p) { (void)hipFree(p); });
        HIP_TRY(hipMemcpy(d, sp->stage1.data(), b1, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(static_cast<uint8_t *>(d) + b1, sp->stage2.data(), sp->stage2.size(), hipMemcpyHostToDevice));
        it = sp->dev.emplace(device, guard.release()).first;
    }
    out.stage1 = static_cast<const uint16_t *>(it->second);
    out.stage2 = static_cast<const uint8_t *>(it->second) + sp->stage1.size() * sizeof(uint16_t);
    return DAAC_OK;
}

const char *rule_name(int rule) { return rule == DAAC_SPLIT_GPT2 ? "gpt2" : rule == DAAC_SPLIT_CL100K ? "cl100k" : rule == DAAC_SPLIT_LLAMA3 ? "llama3" : rule == DAAC_SPLIT_BERT ? "bert" : rule == DAAC_SPLIT_O200K ? "o200k" : "whitespace"; }
bool rule_scans(int rule) { return rule == DAAC_SPLIT_CL100K || rule == DAAC_SPLIT_LLAMA3; }

daac_status too_many_words(uint64_t words) {
    set_error("the list of " + std::to_string(words) + " words exceeds max_result_bytes");
    return DAAC_ERR_AUTOMATON_SCALE;
}

// `text`: the byte at offsets[0] on the device; `d_off`: the n + 1 offsets on the device (n >= 1, checked); ends = {offsets[0], offsets[n]}.
daac_status split_device(daac_splitter *sp, const uint8_t *text, const uint64_t ends[2], const unsigned long long *d_off, uint64_t n, hipStream_t stream,
                         uint64_t **dev_word_offsets, uint64_t **dev_doc_words, uint64_t *n_words) {
    const uint64_t total = ends[1] - ends[0];
    if (n + 1 > static_cast<uint64_t>(OPT(max_result_bytes)) / sizeof(uint64_t)) { set_error("doc_words of " + std::to_string(n) + " documents exceeds max_result_bytes"); return DAAC_ERR_AUTOMATON_SCALE; }
    void *doc_words = nullptr;
    HIP_TRY(dev_malloc(&doc_words, (n + 1) * sizeof(uint64_t), stream));
    auto g_docs = dev_guard(doc_words, stream);
    if (total == 0) {   // documents, all of them empty: no word
        void *wo = nullptr;
        HIP_TRY(dev_malloc(&wo, sizeof(uint64_t), stream));
        auto g_wo = dev_guard(wo, stream);
        HIP_TRY(hipMemsetAsync(doc_words, 0, (n + 1) * sizeof(uint64_t), stream));
        HIP_TRY(hipMemcpyAsync(wo, &ends[0], sizeof(uint64_t), hipMemcpyHostToDevice, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        g_last_kernel = std::string("split rule=") + rule_name(sp->rule) + " docs=" + std::to_string(n) + " bytes=0 words=0";
        *dev_word_offsets = static_cast<uint64_t *>(g_wo.release());
        *dev_doc_words = static_cast<uint64_t *>(g_docs.release());
        *n_words = 0;
        return DAAC_OK;
    }
    daac::SplitArgs a{};
    daac_status st = table_of(sp, a.tab);
    if (st != DAAC_OK) return st;
    a.text = text;
    a.total = total;
    a.base = ends[0];
    a.doc_off = d_off;
    a.n_docs = n;
    a.rule = sp->rule;
    a.tiles = (total + daac::kSplitTile - 1) / daac::kSplitTile;
    // the scratch: the tile counts, their sum, the sum's scratch, the masks, the marks; for a rule with scans three words a tile more, for
    // DAAC_SPLIT_O200K a 64-bit map a tile on top of them (in front of the masks: aligned)
    const uint64_t n_mask = a.tiles * (daac::kSplitTile / 64), n_mark = a.tiles * (daac::kSplitTile / 32) + 1, n_scan = exclusive_scan_scratch(a.tiles);
    const bool o200k = sp->rule == DAAC_SPLIT_O200K;
    const uint64_t n_carry = rule_scans(sp->rule) || o200k ? 3 * a.tiles : 0, n_map = o200k ? a.tiles : 0;
    DevBuf work;
    HIP_TRY(work.alloc((a.tiles + 1 + n_scan + n_map + n_mask) * sizeof(unsigned long long) + (n_mark + n_carry) * sizeof(uint32_t), stream));
    a.counts = static_cast<unsigned long long *>(work.p);
    unsigned long long *sum = a.counts + a.tiles, *scan_scratch = sum + 1;
    a.n_words = sum;
    a.masks = scan_scratch + n_scan + n_map;
    a.marks = reinterpret_cast<uint32_t *>(a.masks + n_mask);
    HIP_TRY(hipMemsetAsync(a.marks, 0, n_mark * sizeof(uint32_t), stream));
    HIP_TRY(daac::launch_split_marks(a, stream));
    if (n_carry) {
        a.tile_sum = a.marks + n_mark;
        a.carry_f = a.tile_sum + a.tiles;
        a.carry_b = a.carry_f + a.tiles;
        if (o200k) HIP_TRY(daac::launch_split_flags_o200k(daac::SplitO200kArgs{a, scan_scratch + n_scan}, stream));
        else HIP_TRY(daac::launch_split_flags_scanned(a, stream));
    } else {
        HIP_TRY(daac::launch_split_flags(a, stream));
    }
    HIP_TRY(daac::launch_exclusive_scan(a.counts, a.tiles, sum, scan_scratch, stream));
    unsigned long long words = 0;
    HIP_TRY(hipMemcpyAsync(&words, sum, sizeof(words), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    if (words > total) { set_error("the word count does not fit the text"); return DAAC_ERR_DEVICE; }   // (never seen: a word has a byte)
    if (words + 1 > static_cast<uint64_t>(OPT(max_result_bytes)) / sizeof(uint64_t)) return too_many_words(words);
    void *wo = nullptr;
    HIP_TRY(dev_malloc(&wo, (words + 1) * sizeof(uint64_t), stream));
    auto g_wo = dev_guard(wo, stream);
    a.word_offsets = static_cast<unsigned long long *>(wo);
    a.doc_words = static_cast<unsigned long long *>(doc_words);
    HIP_TRY(daac::launch_split_scatter(a, stream));
    HIP_TRY(hipStreamSynchronize(stream));   // the call's scratch is released next; the result is the caller's from here
    g_last_kernel = std::string("split rule=") + rule_name(sp->rule) + " docs=" + std::to_string(n) + " bytes=" + std::to_string(total) + " words=" + std::to_string(words) +
                    " tile=" + std::to_string(daac::kSplitTile);
    *dev_word_offsets = static_cast<uint64_t *>(g_wo.release());
    *dev_doc_words = static_cast<uint64_t *>(g_docs.release());
    *n_words = words;
    return DAAC_OK;
}

}  // namespace

extern "C" {

daac_status daac_splitter_create(int rule, const daac_char_range *ranges, size_t n_ranges, daac_splitter **out) {
    if (!out) { set_error("null argument"); return DAAC_ERR_INVALID_ARGUMENT; }
    *out = nullptr;
    if (rule != DAAC_SPLIT_WHITESPACE && rule != DAAC_SPLIT_GPT2 && rule != DAAC_SPLIT_CL100K && rule != DAAC_SPLIT_LLAMA3 && rule != DAAC_SPLIT_BERT &&
        rule != DAAC_SPLIT_O200K) {
        set_error("rule is none of DAAC_SPLIT_WHITESPACE, DAAC_SPLIT_GPT2, DAAC_SPLIT_CL100K, DAAC_SPLIT_LLAMA3, DAAC_SPLIT_BERT and DAAC_SPLIT_O200K");
        return DAAC_ERR_INVALID_ARGUMENT;
    }
    if (n_ranges && !ranges) { set_error("ranges is NULL with n_ranges = " + std::to_string(n_ranges)); return DAAC_ERR_INVALID_ARGUMENT; }
    for (size_t i = 0; i < n_ranges; ++i) {
        const daac_char_range &r = ranges[i];
        const std::string at = "range " + std::to_string(i);
        if (r.last < r.first) { set_error(at + ": last < first"); return DAAC_ERR_INVALID_ARGUMENT; }
        if (r.first < 0x80u) { set_error(at + ": first is below U+0080 (the ASCII classes are fixed)"); return DAAC_ERR_INVALID_ARGUMENT; }
        if (r.last > 0x10FFFFu) { set_error(at + ": last is above U+10FFFF"); return DAAC_ERR_INVALID_ARGUMENT; }
        if (r.cls < 1u || r.cls > (rule == DAAC_SPLIT_O200K ? 6u : 3u)) {
            set_error(at + (rule == DAAC_SPLIT_O200K ? ": cls is not 1 (caseless L), 2 (N), 3 (S), 4 (upper), 5 (lower) or 6 (mark)" : ": cls is not 1 (L), 2 (N) or 3 (S)"));
            return DAAC_ERR_INVALID_ARGUMENT;
        }
        if (i && r.first <= ranges[i - 1].last) { set_error(at + ": the ranges are not sorted and disjoint"); return DAAC_ERR_INVALID_ARGUMENT; }
    }
    // the two-stage table: equal blocks of 256 code points are stored once; two bits a code point, four under DAAC_SPLIT_O200K
    const uint32_t bits = rule == DAAC_SPLIT_O200K ? 4u : 2u, per_byte = 8u / bits, block_bytes = 256u / per_byte;
    std::unique_ptr<daac_splitter> sp(new daac_splitter);
    sp->rule = rule;
    sp->stage1.assign(daac::kSplitStage1, 0);
    sp->stage2.assign(block_bytes, 0);
    std::map<std::vector<uint8_t>, uint16_t> seen;
    seen.emplace(sp->stage2, 0);
    size_t r = 0;
    for (uint32_t hi = 0; hi < daac::kSplitStage1; ++hi) {
        const uint32_t lo_cp = hi << 8, hi_cp = lo_cp + 255u;
        while (r < n_ranges && ranges[r].last < lo_cp) ++r;
        if (r == n_ranges || ranges[r].first > hi_cp) continue;   // all O: block 0
        std::vector<uint8_t> blk(block_bytes, 0);
        for (size_t j = r; j < n_ranges && ranges[j].first <= hi_cp; ++j)
            for (uint32_t cp = std::max(ranges[j].first, lo_cp); cp <= std::min(ranges[j].last, hi_cp); ++cp)
                blk[(cp & 255u) / per_byte] = static_cast<uint8_t>(blk[(cp & 255u) / per_byte] | ranges[j].cls << (bits * (cp % per_byte)));
        auto it = seen.find(blk);
        if (it == seen.end()) {
            it = seen.emplace(blk, static_cast<uint16_t>(seen.size())).first;   // (at most kSplitStage1 blocks: 16 bits hold the number)
            sp->stage2.insert(sp->stage2.end(), blk.begin(), blk.end());
        }
        sp->stage1[hi] = it->second;
    }
    *out = sp.release();
    return DAAC_OK;
}

void daac_splitter_free(daac_splitter *sp) {
    if (!sp) return;
    for (auto &kv : sp->dev) (void)hipFree(kv.second);
    delete sp;
}

daac_status daac_split_batch(daac_splitter *sp, const uint8_t *hay, const uint64_t *offsets, size_t n, int hay_is_device, void *stream_,
                             uint64_t **dev_word_offsets, uint64_t **dev_doc_words, uint64_t *n_words) {
    PmaScope scope_(nullptr);   // no handle: the process-wide options
    if (!sp || !dev_word_offsets || !dev_doc_words || !n_words) { set_error("null argument"); return DAAC_ERR_INVALID_ARGUMENT; }
    daac_status st = check_batch_args(hay, offsets, n, hay_is_device);   // status 1 before a device is touched
    if (st != DAAC_OK) return st;
    *dev_word_offsets = nullptr;
    *dev_doc_words = nullptr;
    *n_words = 0;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (n == 0) {   // no document: one word offset and one doc_words entry, both 0
        DevPtr g_wo, g_dw;
        if ((st = zero_word(stream, g_wo)) != DAAC_OK || (st = zero_word(stream, g_dw)) != DAAC_OK) return st;
        HIP_TRY(hipStreamSynchronize(stream));
        g_last_kernel = std::string("split rule=") + rule_name(sp->rule) + " docs=0 bytes=0 words=0";
        *dev_word_offsets = static_cast<uint64_t *>(g_wo.release());
        *dev_doc_words = static_cast<uint64_t *>(g_dw.release());
        return DAAC_OK;
    }
    StagedBatch b;   // the flag pass reads what the offsets say: device offsets are validated first
    if ((st = stage_batch(hay, offsets, n, hay_is_device, stream, BatchCheck::kernel, b)) != DAAC_OK) return st;
    return split_device(sp, b.dev_hay + b.ends[0], b.ends, b.d_off, n, stream, dev_word_offsets, dev_doc_words, n_words);
}

daac_status daac_split(daac_splitter *sp, const uint8_t *hay, size_t len, int hay_is_device, void *stream_, uint64_t **dev_word_offsets, uint64_t *n_words) {
    if (!sp || !dev_word_offsets || !n_words) { set_error("null argument"); return DAAC_ERR_INVALID_ARGUMENT; }
    if (len && !hay) { set_error("hay is NULL"); return DAAC_ERR_INVALID_ARGUMENT; }
    *dev_word_offsets = nullptr;
    *n_words = 0;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    PmaScope scope_(nullptr);
    StagedBatch b;
    daac_status st = stage_one(hay, len, hay_is_device, stream, b);
    if (st != DAAC_OK) return st;
    uint64_t *doc_words = nullptr;
    st = split_device(sp, b.dev_hay, b.ends, b.d_off, 1, stream, dev_word_offsets, &doc_words, n_words);
    dev_free(doc_words, stream);
    return st;
}

daac_status daac_split_words_space(daac_splitter *sp, const uint8_t *hay, const uint64_t *dev_word_offsets, size_t n_words, int hay_is_device, void *stream_,
                                   uint8_t **dev_flags) {
    if (!sp || !dev_flags || (n_words && (!hay || !dev_word_offsets))) { set_error("null argument"); return DAAC_ERR_INVALID_ARGUMENT; }
    *dev_flags = nullptr;
    if (n_words == 0) return DAAC_OK;
    PmaScope scope_(nullptr);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (n_words > static_cast<uint64_t>(OPT(max_result_bytes))) { set_error("the flags of " + std::to_string(n_words) + " words exceed max_result_bytes"); return DAAC_ERR_AUTOMATON_SCALE; }
    daac::SplitTable tab{};
    daac_status st = table_of(sp, tab);
    if (st != DAAC_OK) return st;
    void *staged = nullptr;
    const uint8_t *dev_hay = hay;
    uint64_t ends[2] = {0, ~0ull};   // what the words lie in: a device haystack is the caller's word for it
    if (!hay_is_device) {   // the words' bytes go to the device once: the first and the last offset say which
        HIP_TRY(hipMemcpyAsync(&ends[0], dev_word_offsets, sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipMemcpyAsync(&ends[1], dev_word_offsets + n_words, sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        if (ends[1] < ends[0]) { set_error("word offsets decrease"); return DAAC_ERR_INVALID_ARGUMENT; }
        if ((st = stage_window(hay, ends[0], ends[1], stream, &staged, &dev_hay)) != DAAC_OK) return st;
    }
    std::unique_ptr<void, void (*)(void *)> g1(staged, [](void *p) { if (p) (void)hipFree(p); });
    void *flags = nullptr;
    HIP_TRY(dev_malloc(&flags, n_words, stream));
    DevPtr g = dev_guard(flags, stream);
    HIP_TRY(daac::launch_split_words_space(tab, dev_hay, reinterpret_cast<const unsigned long long *>(dev_word_offsets), n_words, ends[0], ends[1],
                                           static_cast<uint8_t *>(flags), stream, sp->rule == DAAC_SPLIT_O200K));
    HIP_TRY(hipStreamSynchronize(stream));
    *dev_flags = static_cast<uint8_t *>(g.release());
    return DAAC_OK;
}

daac_status daac_offsets_compose(const uint64_t *dev_inner, const uint64_t *dev_outer, size_t n_outer, void *stream_, uint64_t **dev_out) {
    if (!dev_out || (n_outer && (!dev_inner || !dev_outer))) { set_error("null argument"); return DAAC_ERR_INVALID_ARGUMENT; }
    *dev_out = nullptr;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    void *out = nullptr;
    HIP_TRY(dev_malloc(&out, n_outer * sizeof(uint64_t), stream));
    DevPtr g = dev_guard(out, stream);
    HIP_TRY(daac::launch_offsets_compose(reinterpret_cast<const unsigned long long *>(dev_inner), reinterpret_cast<const unsigned long long *>(dev_outer), n_outer,
                                         static_cast<unsigned long long *>(out), stream));
    HIP_TRY(hipStreamSynchronize(stream));
    *dev_out = static_cast<uint64_t *>(g.release());
    return DAAC_OK;
}

daac_status daac_spans_rebase(uint64_t *dev_spans, const uint64_t *dev_tok_offsets, const uint64_t *dev_word_offsets, const uint64_t *dev_doc_words,
                              const uint64_t *dev_doc_offsets, size_t n_words, size_t n_docs, void *stream_) {
    if (n_words && n_docs && (!dev_spans || !dev_tok_offsets || !dev_word_offsets || !dev_doc_words || !dev_doc_offsets)) { set_error("null argument"); return DAAC_ERR_INVALID_ARGUMENT; }
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    HIP_TRY(daac::launch_spans_rebase(reinterpret_cast<unsigned long long *>(dev_spans), reinterpret_cast<const unsigned long long *>(dev_tok_offsets),
                                      reinterpret_cast<const unsigned long long *>(dev_word_offsets), reinterpret_cast<const unsigned long long *>(dev_doc_words),
                                      reinterpret_cast<const unsigned long long *>(dev_doc_offsets), n_words, n_docs, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    return DAAC_OK;
}

}  // extern "C"
