// C ABI (include/daachorse_amd.h), part 16: model inputs — a token result wrapped in a template, truncated and padded into the planes a
// model reads (daac_tokens_pack).  The kernels are pack_kernels.hip and, for the CSR form's row offsets, the exclusive sum of
// scan_kernels.hip.  This file validates its arguments in the header's order, runs the header pass, reads the four totals back once
// (read_totals: the token calls' back door, "api_tokens.hip"), sizes and allocates the planes and runs the slot pass.
#include "api_internal.hpp"
#include "pack.hpp"

namespace {

daac_status pack_refuse(const std::string &msg) {
    set_error(msg);
    return DAAC_ERR_INVALID_ARGUMENT;
}

// a template's rules; *n_added: its special pieces
daac_status check_template(const char *name, const daac_pack_piece *pieces, uint32_t n, bool pair, uint32_t *n_added) {
    if (n > DAAC_PACK_MAX_PIECES) return pack_refuse(std::string("the ") + name + " template has " + std::to_string(n) + " pieces: at most " + std::to_string(DAAC_PACK_MAX_PIECES));
    uint32_t count[3] = {0, 0, 0};
    for (uint32_t i = 0; i < n; ++i) {
        if (pieces[i].kind > DAAC_PACK_B) return pack_refuse(std::string("the ") + name + " template: piece " + std::to_string(i) + " has no such kind");
        ++count[pieces[i].kind];
    }
    if (count[DAAC_PACK_A] != 1) return pack_refuse(std::string("the ") + name + " template holds sequence A " + std::to_string(count[DAAC_PACK_A]) + " times: exactly once");
    if (count[DAAC_PACK_B] != (pair ? 1u : 0u)) return pack_refuse(std::string("the ") + name + " template holds sequence B " + std::to_string(count[DAAC_PACK_B]) + " times: " + (pair ? "exactly once" : "never"));
    *n_added = count[DAAC_PACK_SPECIAL];
    return DAAC_OK;
}

struct PackOuts {   // the caller's out-pointers
    void **input_ids, **type_ids, **attention, **special;
    uint64_t **offsets, **row_offsets;
    uint64_t *row_length, *n_slots;
    void clear() const {
        *input_ids = nullptr;
        if (type_ids) *type_ids = nullptr;
        if (attention) *attention = nullptr;
        if (special) *special = nullptr;
        if (offsets) *offsets = nullptr;
        if (row_offsets) *row_offsets = nullptr;
        *row_length = 0;
        *n_slots = 0;
    }
};

}  // namespace

extern "C" {

daac_status daac_tokens_pack(const daac_pack_params *params, const uint32_t *dev_a_ids, const uint64_t *dev_a_spans, const uint64_t *dev_a_offsets,
                             uint64_t a_tokens, const uint32_t *dev_b_ids, const uint64_t *dev_b_spans, const uint64_t *dev_b_offsets, uint64_t b_tokens,
                             size_t n, void *stream_, void **dev_input_ids, void **dev_token_type_ids, void **dev_attention_mask,
                             void **dev_special_tokens_mask, uint64_t **dev_offsets, uint64_t **dev_row_offsets, uint64_t *row_length, uint64_t *n_slots) {
    PmaScope scope_(nullptr);   // no handle: the process-wide options
    const PackOuts o{dev_input_ids, dev_token_type_ids, dev_attention_mask, dev_special_tokens_mask, dev_offsets, dev_row_offsets, row_length, n_slots};
    const bool pair = dev_b_offsets != nullptr;
    // ---- before a device is touched, in the header's order
    if (!params || !dev_input_ids || !row_length || !n_slots || (n && !dev_a_offsets) || (a_tokens && !dev_a_ids) || (pair && b_tokens && !dev_b_ids)) return pack_refuse("null argument");
    const daac_pack_params &p = *params;
    if (p.struct_size != sizeof(daac_pack_params)) return pack_refuse("daac_pack_params.struct_size is " + std::to_string(p.struct_size) + ", not " + std::to_string(sizeof(daac_pack_params)));
    uint32_t added_single = 0, added_pair = 0;
    daac_status st = check_template("single", p.single, p.n_single, false, &added_single);
    if (st != DAAC_OK) return st;
    if (pair && !p.n_pair) return pack_refuse("a pair batch without a pair template");
    if (p.n_pair && (st = check_template("pair", p.pair, p.n_pair, true, &added_pair)) != DAAC_OK) return st;
    if (p.width != 4 && p.width != 8) return pack_refuse("width is " + std::to_string(p.width) + ": 4 (int32) or 8 (int64)");
    if (p.truncate && p.strategy > DAAC_TRUNC_ONLY_SECOND) return pack_refuse("no such truncation strategy");
    if (p.padding > DAAC_PAD_FIXED) return pack_refuse("no such padding");
    if (p.padding != DAAC_PAD_NONE && p.pad_multiple == 0) return pack_refuse("pad_multiple is 0: 1 for none");
    if (p.truncate && p.strategy == DAAC_TRUNC_ONLY_SECOND && !pair) return pack_refuse("only_second truncates sequence B: the batch has none");
    const uint32_t n_added = pair ? added_pair : added_single;
    if (p.truncate && p.max_length < n_added) return pack_refuse("max_length " + std::to_string(p.max_length) + " is below the template's " + std::to_string(n_added) + " special tokens");
    const bool csr = p.padding == DAAC_PAD_NONE;
    if (csr && !dev_row_offsets) return pack_refuse("null argument: the result without padding has row offsets");
    if (dev_offsets && ((a_tokens && !dev_a_spans) || (pair && b_tokens && !dev_b_spans))) return pack_refuse("offsets are wanted, but a sequence with tokens has no spans");
    o.clear();
    const uint64_t max_bytes = static_cast<uint64_t>(OPT(max_result_bytes));
    if (csr && n >= max_bytes / sizeof(uint64_t)) { set_error("row_offsets (n + 1 entries) of " + std::to_string(n) + " documents exceeds max_result_bytes"); return DAAC_ERR_AUTOMATON_SCALE; }
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const std::string head = "pack docs=" + std::to_string(n) + " pair=" + std::to_string(pair ? 1 : 0);
    if (n == 0) {   // no document: no plane, L = 0, and the CSR form's one offset
        DevPtr g_ro;
        if (csr) {
            if ((st = zero_word(stream, g_ro)) != DAAC_OK) return st;
            HIP_TRY(hipStreamSynchronize(stream));
            *dev_row_offsets = static_cast<uint64_t *>(g_ro.release());
        }
        g_last_kernel = head + " row=0 tokens=0 dropped=0";
        return DAAC_OK;
    }
    daac::PackArgs a{};
    a.a_ids = dev_a_ids;
    a.a_spans = dev_offsets ? reinterpret_cast<const unsigned long long *>(dev_a_spans) : nullptr;
    a.a_off = reinterpret_cast<const unsigned long long *>(dev_a_offsets);
    a.a_tokens = a_tokens;
    a.b_ids = dev_b_ids;
    a.b_spans = dev_offsets ? reinterpret_cast<const unsigned long long *>(dev_b_spans) : nullptr;
    a.b_off = reinterpret_cast<const unsigned long long *>(dev_b_offsets);
    a.b_tokens = pair ? b_tokens : 0;
    a.n_docs = n;
    a.n_pieces = pair ? p.n_pair : p.n_single;
    for (uint32_t i = 0; i < a.n_pieces; ++i) {
        const daac_pack_piece &q = (pair ? p.pair : p.single)[i];
        a.pieces[i] = daac::PackPiece{q.kind, q.id, q.type_id};
    }
    a.n_added = n_added;
    a.truncate = p.truncate ? 1 : 0;
    a.strategy = p.strategy;
    a.trunc_left = p.truncate && p.truncate_left ? 1 : 0;
    a.budget = p.truncate ? p.max_length - n_added : 0;
    a.pad_left = !csr && p.pad_left ? 1 : 0;
    a.pad_id = p.pad_id;
    a.pad_type_id = p.pad_type_id;
    a.width = p.width;
    a.csr = csr ? 1 : 0;
    // the scratch: the row headers, the four totals and, for the CSR form, the sum's total and its scratch
    const uint64_t m = n + 1;
    DevBuf work;
    HIP_TRY(work.alloc((daac::kPackHdrWords * n + daac::kPackFoldWords + 1 + (csr ? exclusive_scan_scratch(m) : 0)) * sizeof(unsigned long long), stream));
    a.hdr = static_cast<unsigned long long *>(work.p);
    a.fold = a.hdr + daac::kPackHdrWords * n;
    unsigned long long *sum = a.fold + daac::kPackFoldWords, *scan_scratch = sum + 1;
    void *ro = nullptr;
    if (csr) HIP_TRY(dev_malloc(&ro, m * sizeof(uint64_t), stream));
    DevPtr g_ro = dev_guard(ro, stream);
    a.row_len = static_cast<unsigned long long *>(ro);
    HIP_TRY(hipMemsetAsync(a.fold, 0, (daac::kPackFoldWords + 1) * sizeof(unsigned long long), stream));
    HIP_TRY(daac::launch_pack_header(a, stream));
    if (csr) HIP_TRY(daac::launch_exclusive_scan(a.row_len, m, sum, scan_scratch, stream));
    unsigned long long h[daac::kPackFoldWords] = {0, 0, 0, 0};
    if ((st = read_totals(a.fold, daac::kPackFoldWords, stream, h)) != DAAC_OK) return st;
    if (h[1]) {   // the first document in error
        const unsigned long long code = ~h[1];
        const std::string doc = "document " + std::to_string(code / 2) + ": ";
        if (code % 2 == daac::kPackOffsetsBroken) return pack_refuse(doc + "its token offsets decrease or leave the token list");
        return pack_refuse(doc + (p.strategy == DAAC_TRUNC_ONLY_FIRST ? "only_first" : "only_second") + " cannot take " + "the tokens above max_length from a sequence this short");
    }
    const uint64_t longest = h[0], R = h[2], dropped = h[3];
    uint64_t L = longest;
    if (!csr) {
        if (p.padding == DAAC_PAD_FIXED && p.pad_length > L) L = p.pad_length;
        const uint64_t rem = L % p.pad_multiple;
        if (rem) {
            if (L > UINT64_MAX - (p.pad_multiple - rem)) { set_error("the padded row length exceeds max_result_bytes"); return DAAC_ERR_AUTOMATON_SCALE; }
            L += p.pad_multiple - rem;
        }
    }
    const uint64_t per_slot = static_cast<uint64_t>(p.width) * (1 + (dev_token_type_ids ? 1 : 0) + (dev_attention_mask && !csr ? 1 : 0) + (dev_special_tokens_mask ? 1 : 0)) +
                              (dev_offsets ? 2 * sizeof(uint64_t) : 0);
    if (csr ? R > max_bytes / per_slot : (L != 0 && n > max_bytes / per_slot / L)) {
        set_error("the result of " + std::to_string(n) + " rows of " + std::to_string(csr ? longest : L) + " exceeds max_result_bytes");
        return DAAC_ERR_AUTOMATON_SCALE;
    }
    a.L = L;
    a.slots = csr ? R : n * L;
    a.row_offsets = a.row_len;
    void *pl[4] = {nullptr, nullptr, nullptr, nullptr}, *off = nullptr;
    void **const want[4] = {dev_input_ids, dev_token_type_ids, csr ? nullptr : dev_attention_mask, dev_special_tokens_mask};
    DevPtr g_pl[4], g_off;
    for (int i = 0; i < 4; ++i) {
        if (want[i] && a.slots) HIP_TRY(dev_malloc(&pl[i], a.slots * p.width, stream));
        g_pl[i] = dev_guard(pl[i], stream);
    }
    if (dev_offsets && a.slots) HIP_TRY(dev_malloc(&off, a.slots * 2 * sizeof(uint64_t), stream));
    g_off = dev_guard(off, stream);
    a.input_ids = pl[0];
    a.type_ids = pl[1];
    a.attention = pl[2];
    a.special = pl[3];
    a.offsets = static_cast<unsigned long long *>(off);
    if (a.slots) HIP_TRY(daac::launch_pack_slots(a, stream));
    HIP_TRY(hipStreamSynchronize(stream));   // the call's scratch is released next; the result is the caller's from here
    g_last_kernel = head + " row=" + std::to_string(L) + " tokens=" + std::to_string(R - n * n_added) + " dropped=" + std::to_string(dropped);
    for (int i = 0; i < 4; ++i)
        if (want[i]) *want[i] = g_pl[i].release();
    if (dev_offsets) *dev_offsets = static_cast<uint64_t *>(g_off.release());
    if (csr) *dev_row_offsets = static_cast<uint64_t *>(g_ro.release());
    *row_length = L;
    *n_slots = a.slots;
    return DAAC_OK;
}

}  // extern "C"
