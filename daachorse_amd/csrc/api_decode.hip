// C ABI (include/daachorse_amd.h), part 17: token ids back to text (daac_decoder_create, daac_decoder_free, daac_tokens_decode).  No
// automaton is involved: a decoder is a table of images over the ids and a pool of their bytes, uploaded per device on first use as
// daac_normalizer's table is.  This file validates its arguments in the header's order, runs the sizing and header passes and the
// exclusive sum, reads the four totals back once (read_totals: the token calls' back door, "api_tokens.hip"), applies the errors and the
// limit, allocates the text and runs the copy pass; the kernels are decode_kernels.hip.
#include "api_internal.hpp"
#include "decode.hpp"

struct daac_decoder {
    std::vector<daac::DecodePiece> pieces;
    std::vector<uint8_t> flags;
    std::vector<uint8_t> pool;
    std::mutex mu;
    struct OnDevice { void *block; int num_cu; };
    std::map<int, OnDevice> dev;   // per device: pieces, flags, pool in one block
};

namespace {

daac_status decode_refuse(const std::string &msg) {
    set_error(msg);
    return DAAC_ERR_INVALID_ARGUMENT;
}

daac_status table_of(daac_decoder *dec, daac::DecodeArgs &a, uint32_t *num_cu) {
    int device = 0;
    HIP_TRY(hipGetDevice(&device));
    std::lock_guard<std::mutex> g(dec->mu);
    const size_t b_pieces = dec->pieces.size() * sizeof(daac::DecodePiece), b_flags = (dec->flags.size() + 15) & ~size_t(15);
    auto it = dec->dev.find(device);
    if (it == dec->dev.end()) {
        void *d = nullptr;
        HIP_TRY(hipMalloc(&d, b_pieces + b_flags + dec->pool.size() + 16));
        std::unique_ptr<void, void (*)(void *)> guard(d, [](void *p) { (void)hipFree(p); });
        uint8_t *at = static_cast<uint8_t *>(d);
        if (b_pieces) HIP_TRY(hipMemcpy(at, dec->pieces.data(), b_pieces, hipMemcpyHostToDevice));
        if (!dec->flags.empty()) HIP_TRY(hipMemcpy(at + b_pieces, dec->flags.data(), dec->flags.size(), hipMemcpyHostToDevice));
        if (!dec->pool.empty()) HIP_TRY(hipMemcpy(at + b_pieces + b_flags, dec->pool.data(), dec->pool.size(), hipMemcpyHostToDevice));
        int cus = 0;
        HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device));
        it = dec->dev.emplace(device, daac_decoder::OnDevice{guard.release(), cus}).first;
    }
    const uint8_t *at = static_cast<const uint8_t *>(it->second.block);
    a.pieces = reinterpret_cast<const daac::DecodePiece *>(at);
    a.flags = at + b_pieces;
    a.pool = at + b_pieces + b_flags;
    a.pool_bytes = dec->pool.size();
    a.n_ids = dec->pieces.size();
    *num_cu = static_cast<uint32_t>(std::max(1, it->second.num_cu));
    return DAAC_OK;
}

}  // namespace

extern "C" {

daac_status daac_decoder_create(const uint8_t *pool, uint64_t pool_bytes, const daac_decode_piece *pieces, const uint8_t *flags, uint64_t n_ids, daac_decoder **out) {
    if (!out) return decode_refuse("null argument");
    *out = nullptr;
    if (pool_bytes && !pool) return decode_refuse("pool is NULL with pool_bytes = " + std::to_string(pool_bytes));
    if (n_ids && (!pieces || !flags)) return decode_refuse("pieces or flags is NULL with n_ids = " + std::to_string(n_ids));
    if (pool_bytes >= (1ull << 32)) return decode_refuse("the pool has " + std::to_string(pool_bytes) + " bytes: below 4 GiB");
    if (n_ids > (1ull << 32)) return decode_refuse("n_ids is " + std::to_string(n_ids) + ": an id has 32 bits");
    for (uint64_t i = 0; i < n_ids; ++i) {
        const daac_decode_piece &p = pieces[i];
        if (flags[i] & ~(DAAC_DECODE_SPECIAL | DAAC_DECODE_ABSENT)) return decode_refuse("id " + std::to_string(i) + ": flags other than DAAC_DECODE_SPECIAL and DAAC_DECODE_ABSENT");
        if (static_cast<uint64_t>(p.off) + p.len > pool_bytes || static_cast<uint64_t>(p.first_off) + p.first_len > pool_bytes)
            return decode_refuse("id " + std::to_string(i) + ": an image leaves the pool");
    }
    std::unique_ptr<daac_decoder> dec(new daac_decoder);
    dec->pool.assign(pool, pool + pool_bytes);
    dec->flags.assign(flags, flags + n_ids);
    dec->pieces.resize(n_ids);
    for (uint64_t i = 0; i < n_ids; ++i) dec->pieces[i] = daac::DecodePiece{pieces[i].off, pieces[i].len, pieces[i].first_off, pieces[i].first_len};
    *out = dec.release();
    return DAAC_OK;
}

void daac_decoder_free(daac_decoder *dec) {
    if (!dec) return;
    for (auto &kv : dec->dev) (void)hipFree(kv.second.block);
    delete dec;
}

daac_status daac_tokens_decode(daac_decoder *dec, const void *dev_ids, uint32_t id_width, const uint64_t *dev_offsets, uint64_t n_tokens, size_t n, uint64_t row_length,
                               int skip_special, int unknown_skip, void *stream_, uint8_t **dev_out, uint64_t **dev_out_offsets, uint64_t **dev_token_starts,
                               uint64_t *out_bytes) {
    PmaScope scope_(nullptr);   // no handle of an automaton: the process-wide options
    const bool csr = dev_offsets != nullptr;
    // ---- before a device is touched, in the header's order
    if (!dec || !dev_out || !dev_out_offsets || !out_bytes || (csr && n_tokens && !dev_ids) || (!csr && n && row_length && !dev_ids)) return decode_refuse("null argument");
    if (id_width != 4 && id_width != 8) return decode_refuse("id_width is " + std::to_string(id_width) + ": 4 (int32 / uint32) or 8 (int64)");
    if (csr && id_width != 4) return decode_refuse("id_width is 8: a CSR token list holds 4-byte ids");
    if (!csr && n && !row_length) return decode_refuse("neither token offsets nor a row_length: " + std::to_string(n) + " documents need one of them");
    const uint64_t max_bytes = static_cast<uint64_t>(OPT(max_result_bytes));
    if (n >= max_bytes / sizeof(uint64_t)) { set_error("out_offsets (n + 1 entries) of " + std::to_string(n) + " documents exceeds max_result_bytes"); return DAAC_ERR_AUTOMATON_SCALE; }
    if (!csr && n && n > (max_bytes / sizeof(uint64_t)) / row_length) {
        set_error("a plane of " + std::to_string(n) + " rows of " + std::to_string(row_length) + " exceeds max_result_bytes");
        return DAAC_ERR_AUTOMATON_SCALE;
    }
    const uint64_t T = csr ? n_tokens : static_cast<uint64_t>(n) * row_length;
    if (dev_token_starts && T >= max_bytes / sizeof(uint64_t)) { set_error("token_starts of " + std::to_string(T) + " tokens exceeds max_result_bytes"); return DAAC_ERR_AUTOMATON_SCALE; }
    *dev_out = nullptr;
    *dev_out_offsets = nullptr;
    if (dev_token_starts) *dev_token_starts = nullptr;
    *out_bytes = 0;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    daac_status st;
    const std::string head = "decode docs=" + std::to_string(n);
    if (n == 0) {   // no document: no byte and one offset, 0
        DevPtr g_oo;
        if ((st = zero_word(stream, g_oo)) != DAAC_OK) return st;
        HIP_TRY(hipStreamSynchronize(stream));
        *dev_out_offsets = static_cast<uint64_t *>(g_oo.release());
        g_last_kernel = head + " tokens=0 kept=0 bytes=0";
        return DAAC_OK;
    }
    daac::DecodeArgs a{};
    uint32_t num_cu = 1;
    if ((st = table_of(dec, a, &num_cu)) != DAAC_OK) return st;
    a.ids = dev_ids;
    a.width = id_width;
    a.off = reinterpret_cast<const unsigned long long *>(dev_offsets);
    a.row_len = csr ? 0 : row_length;
    a.n_tokens = T;
    a.n_docs = n;
    a.skip_special = skip_special ? 1 : 0;
    a.unknown_skip = unknown_skip ? 1 : 0;
    // the results that exist whatever the text's size, and the scratch: the three folded words and the sum's total, the sum's scratch,
    // the starts unless they are a result, the marks
    void *oo = nullptr, *ts = nullptr;
    HIP_TRY(dev_malloc(&oo, (n + 1) * sizeof(uint64_t), stream));
    DevPtr g_oo = dev_guard(oo, stream);
    if (dev_token_starts) HIP_TRY(dev_malloc(&ts, (T + 1) * sizeof(uint64_t), stream));
    DevPtr g_ts = dev_guard(ts, stream);
    const uint64_t n_scan = exclusive_scan_scratch(T + 1);
    DevBuf work;
    HIP_TRY(work.alloc((daac::kDecodeFoldWords + 1 + n_scan + (ts ? 0 : T + 1)) * sizeof(unsigned long long) + T, stream));
    a.fold = static_cast<unsigned long long *>(work.p);
    unsigned long long *sum = a.fold + daac::kDecodeFoldWords, *scan_scratch = sum + 1;
    a.start = ts ? static_cast<unsigned long long *>(ts) : scan_scratch + n_scan;
    a.mark = reinterpret_cast<uint8_t *>(scan_scratch + n_scan + (ts ? 0 : T + 1));
    a.out_offsets = static_cast<unsigned long long *>(oo);
    HIP_TRY(hipMemsetAsync(a.fold, 0, (daac::kDecodeFoldWords + 1) * sizeof(unsigned long long), stream));
    HIP_TRY(daac::launch_decode_size(a, stream));
    HIP_TRY(daac::launch_decode_header(a, stream));
    HIP_TRY(daac::launch_exclusive_scan(a.start, T + 1, sum, scan_scratch, stream));
    unsigned long long h[daac::kDecodeFoldWords + 1] = {0, 0, 0, 0};
    if ((st = read_totals(a.fold, daac::kDecodeFoldWords + 1, stream, h)) != DAAC_OK) return st;
    if (h[0]) return decode_refuse("document " + std::to_string(~h[0]) + ": its token offsets decrease or leave the token list");
    if (h[1] && !a.unknown_skip) {   // the lowest token without an entry: its document by the offsets, which are in order
        const uint64_t i = ~h[1];
        uint64_t d = 0;
        if (!csr) {
            d = i / row_length;
        } else {   // the last document that begins at or before the token (the documents in front of it that are empty share its offset)
            std::vector<uint64_t> off(n + 1);
            HIP_TRY(hipMemcpyAsync(off.data(), dev_offsets, (n + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
            HIP_TRY(hipStreamSynchronize(stream));
            d = static_cast<uint64_t>(std::upper_bound(off.begin(), off.end(), i) - off.begin()) - 1;
        }
        const uint64_t first = csr ? 0 : d * row_length;
        return decode_refuse("document " + std::to_string(d) + ", token " + std::to_string(i) + (csr ? "" : " (column " + std::to_string(i - first) + ")") +
                             ": its id has no entry in the decoder (unknown_skip leaves such tokens out)");
    }
    const uint64_t kept = h[2], bytes = h[3];
    if (bytes > max_bytes) {
        set_error("the text of " + std::to_string(bytes) + " bytes exceeds max_result_bytes");
        return DAAC_ERR_AUTOMATON_SCALE;
    }
    HIP_TRY(daac::launch_decode_doc_offsets(a, stream));
    void *out = nullptr;
    HIP_TRY(dev_malloc(&out, bytes, stream));   // (no byte: a granule, so that the result is a batch to point at)
    DevPtr g_out = dev_guard(out, stream);
    a.out = static_cast<uint8_t *>(out);
    a.out_len = bytes;
    a.tiles = (bytes + daac::kDecodeTile - 1) / daac::kDecodeTile;
    DevBuf tiles;
    if (a.tiles) {
        HIP_TRY(tiles.alloc((a.tiles + 1) * sizeof(long long), stream));
        a.tile_lo = static_cast<long long *>(tiles.p);
        HIP_TRY(daac::launch_decode_copy(a, num_cu, stream));
    }
    HIP_TRY(hipStreamSynchronize(stream));   // the call's scratch is released next; the result is the caller's from here
    g_last_kernel = head + " tokens=" + std::to_string(T) + " kept=" + std::to_string(kept) + " bytes=" + std::to_string(bytes);
    *dev_out = static_cast<uint8_t *>(g_out.release());
    *dev_out_offsets = static_cast<uint64_t *>(g_oo.release());
    if (dev_token_starts) *dev_token_starts = static_cast<uint64_t *>(g_ts.release());
    *out_bytes = bytes;
    return DAAC_OK;
}

}  // extern "C"
