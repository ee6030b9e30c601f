// tokens_pack on the device (daac_tokens_pack): what api_pack.hip and pack_kernels.hip share, and the per-lane bodies of the kernels.
//
// The definition (include/daachorse_amd.h has it in full).  Sequence A is a CSR token result of n documents (ids, optional spans,
// n + 1 token offsets), sequence B an optional second one of the same n: the batch is all singles or all pairs.  A template is a list
// of at most kPackMaxPieces pieces {kind: special | A | B, id, type_id}; n_added is the number of its special pieces.  Truncation runs
// before the template, on budget = max_length - n_added; a row is the template walked in order over what the sequences keep; padding
// makes the rows one length L (dense planes [n, L]), no padding leaves them as they are (flat planes [R] and n + 1 row offsets).
//
// Two kernels.  The header pass runs one lane per document: what A and B keep, where their first kept token lies, and whether the
// document cannot be truncated as asked; it folds the longest row, the first document in error, the slots and the dropped tokens into
// four words.  The slot pass runs one lane per output slot over the flat n * L (or R) index space: the slot finds its row (a division,
// or a binary search in the row offsets), its column's source — padding, a template piece, a token of A or B — and stores that slot
// of every plane.  The 64 lanes of a wave store 64 consecutive elements of every plane, rows shorter than a wave share it, positions
// are 64-bit, and every word is written by the one lane that owns it: no atomics and no LDS in the slot pass.
//
// The per-lane bodies below are plain C++: with DAAC_PACK_HOST defined this file compiles without HIP and a host program runs them
// document by document and slot by slot (tests/native/pack_check.cpp).
#pragma once

#include <cstdint>

#ifndef DAAC_PACK_HOST
#include <hip/hip_runtime.h>
#define PACK_FN static __host__ __device__ __forceinline__
#else
#define PACK_FN static inline
#endif

namespace daac {

// the launch shape of both passes: lanes of a workgroup, and the workgroups of a pass, which stride over the documents / the slots
// (256 CUs x 8 workgroups: a memory-bound pass gains nothing from more, and 64 consecutive slots stay one wave's)
constexpr uint32_t kPackLanes = 256;
constexpr uint32_t kPackMaxBlocks = 2048;
constexpr uint32_t kPackMaxPieces = 16;   // DAAC_PACK_MAX_PIECES

enum : uint32_t { kPackSpecial = 0, kPackA = 1, kPackB = 2 };                         // daac_pack_piece_kind
enum : uint32_t { kPackLongestFirst = 0, kPackOnlyFirst = 1, kPackOnlySecond = 2 };   // daac_pack_strategy
enum : uint32_t { kPackOffsetsBroken = 0, kPackTooShort = 1 };                        // why a document is in error
constexpr uint32_t kPackHdrWords = 4;    // a row header: {A's first kept token, A's kept tokens, B's first, B's kept}
constexpr uint32_t kPackFoldWords = 4;   // {longest row, ~(2 * first document in error + why), slots of all rows, tokens dropped}: max, max, sum, sum

struct PackPiece {   // daac_pack_piece
    uint32_t kind, id, type_id;
};

struct PackArgs {
    const uint32_t *a_ids;
    const unsigned long long *a_spans;   // NULL: no offsets plane
    const unsigned long long *a_off;     // n_docs + 1
    uint64_t a_tokens;                   // the tokens a_ids (and a_spans) hold: a document's offsets stay inside them or it is in error
    const uint32_t *b_ids;
    const unsigned long long *b_spans;
    const unsigned long long *b_off;     // NULL: singles
    uint64_t b_tokens;
    uint64_t n_docs;
    PackPiece pieces[kPackMaxPieces];    // the template in use
    uint32_t n_pieces, n_added;
    uint32_t truncate, strategy, trunc_left;   // truncate 0: every token is kept
    uint64_t budget;                           // max_length - n_added
    uint32_t pad_left, pad_id, pad_type_id;
    uint32_t width;                            // bytes of a plane's element: 4 or 8
    // the header pass
    unsigned long long *hdr;             // kPackHdrWords * n_docs
    unsigned long long *row_len;         // CSR form: n_docs + 1, the rows' lengths with a closing 0 (their exclusive sum: row_offsets); else NULL
    unsigned long long *fold;            // kPackFoldWords, cleared
    // the slot pass
    uint32_t csr;                        // 1: flat planes over row_offsets, 0: dense planes of row length L
    uint64_t L;
    uint64_t slots;                      // n_docs * L, or R
    const unsigned long long *row_offsets;
    void *input_ids, *type_ids, *attention, *special;   // planes of `width`-byte elements; all but input_ids may be NULL
    unsigned long long *offsets;                        // pairs, or NULL
};

struct PackRow {   // what the header lane learns of its document
    uint64_t a_first, a_keep, b_first, b_keep;
    uint64_t row_len, dropped;
    uint32_t error, why;
};

PACK_FN uint64_t pack_min(uint64_t x, uint64_t y) { return x < y ? x : y; }
PACK_FN uint64_t pack_max(uint64_t x, uint64_t y) { return x > y ? x : y; }

// what two sequences of n1 and n2 tokens keep under `budget`; false: the strategy cannot take what is asked from its one sequence
PACK_FN bool pack_truncate(uint64_t n1, uint64_t n2, bool pair, uint64_t budget, uint32_t strategy, uint64_t &k1, uint64_t &k2) {
    k1 = n1;
    k2 = n2;
    if (budget == 0) { k1 = k2 = 0; return true; }
    if (!pair) { k1 = pack_min(n1, budget); return true; }
    if (n1 <= budget && n2 <= budget - n1) return true;
    const uint64_t need = n1 - (budget - pack_min(n2, budget)) + (n2 - pack_min(n2, budget));   // n1 + n2 - budget, without the sum's overflow
    if (strategy == kPackLongestFirst) {
        uint64_t a = pack_min(n1, n2), b;
        b = a > budget ? a : pack_max(a, budget - a);
        if (a > budget || b > budget - a) { a = budget / 2; b = a + budget % 2; }
        k1 = n1 > n2 ? b : a;
        k2 = n1 > n2 ? a : b;
        return true;
    }
    if (strategy == kPackOnlyFirst) {
        if (n1 <= need) { k1 = k2 = 0; return false; }
        k1 = n1 - need;
        return true;
    }
    if (n2 <= need) { k1 = k2 = 0; return false; }
    k2 = n2 - need;
    return true;
}

// one sequence's tokens of document d; false: its offsets decrease or leave the token list
PACK_FN bool pack_doc_tokens(const unsigned long long *off, uint64_t tokens, uint64_t d, uint64_t &first, uint64_t &n) {
    const uint64_t t0 = off[d], t1 = off[d + 1];
    first = t0;
    n = 0;
    if (t1 < t0 || t1 > tokens) return false;
    n = t1 - t0;
    return true;
}

// document d of n_docs: its header, written to a.hdr (and its row's length to a.row_len)
PACK_FN PackRow pack_header_lane(const PackArgs &a, uint64_t d) {
    PackRow r{};
    uint64_t n1 = 0, n2 = 0;
    bool ok = pack_doc_tokens(a.a_off, a.a_tokens, d, r.a_first, n1);
    if (a.b_off) ok = pack_doc_tokens(a.b_off, a.b_tokens, d, r.b_first, n2) && ok;
    if (!ok) {
        r.error = 1;
        r.why = kPackOffsetsBroken;
        n1 = n2 = 0;
    }
    r.a_keep = n1;
    r.b_keep = n2;
    if (ok && a.truncate && !pack_truncate(n1, n2, a.b_off != nullptr, a.budget, a.strategy, r.a_keep, r.b_keep)) {
        r.error = 1;
        r.why = kPackTooShort;
    }
    if (a.trunc_left) {   // the last tokens are the ones kept
        r.a_first += n1 - r.a_keep;
        r.b_first += n2 - r.b_keep;
    }
    r.dropped = (n1 - r.a_keep) + (n2 - r.b_keep);
    r.row_len = r.a_keep + r.b_keep + a.n_added;
    unsigned long long *h = a.hdr + kPackHdrWords * d;
    h[0] = r.a_first;
    h[1] = r.a_keep;
    h[2] = r.b_first;
    h[3] = r.b_keep;
    if (a.row_len) a.row_len[d] = r.row_len;
    return r;
}

// the largest i in [0, n) with off[i] <= x, for non-decreasing off with off[0] <= x
PACK_FN uint64_t pack_row_of(const unsigned long long *off, uint64_t n, uint64_t x) {
    uint64_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (off[mid] <= x) lo = mid; else hi = mid;
    }
    return lo;
}

enum : uint32_t { kSlotPad = 0, kSlotSpecial = 1, kSlotA = 2, kSlotB = 3 };
struct PackSlot {
    uint32_t source;   // kSlot*
    uint32_t id, type_id;
    uint64_t token;    // kSlotA / kSlotB: the token's index in its sequence's list
};

// column `col` of a row with header h, in a row of L columns (CSR form: L = the row's own length)
PACK_FN PackSlot pack_slot(const PackArgs &a, const unsigned long long *h, uint64_t col, uint64_t L) {
    PackSlot s{kSlotPad, a.pad_id, a.pad_type_id, 0};
    const uint64_t a_keep = h[1], b_keep = h[3], row_len = a_keep + b_keep + a.n_added;
    uint64_t c = col;
    if (a.pad_left) {
        const uint64_t pad = L > row_len ? L - row_len : 0;
        if (c < pad) return s;
        c -= pad;
    }
    if (c >= row_len) return s;
    for (uint32_t p = 0; p < a.n_pieces && p < kPackMaxPieces; ++p) {
        const PackPiece pc = a.pieces[p];
        const uint64_t len = pc.kind == kPackSpecial ? 1 : pc.kind == kPackA ? a_keep : b_keep;
        if (c < len) {
            s.source = pc.kind == kPackSpecial ? kSlotSpecial : pc.kind == kPackA ? kSlotA : kSlotB;
            s.type_id = pc.type_id;
            s.id = pc.id;
            s.token = (pc.kind == kPackA ? h[0] : h[2]) + c;
            return s;
        }
        c -= len;
    }
    return s;   // (never reached: the pieces' lengths sum to row_len)
}

PACK_FN void pack_store(void *plane, uint32_t width, uint64_t x, uint32_t v) {
    if (!plane) return;
    if (width == 8) static_cast<uint64_t *>(plane)[x] = v;
    else static_cast<uint32_t *>(plane)[x] = v;
}

// slot x of a.slots: that slot of every plane
PACK_FN void pack_slot_lane(const PackArgs &a, uint64_t x) {
    uint64_t row, col, L = a.L;
    if (a.csr) {
        row = pack_row_of(a.row_offsets, a.n_docs, x);
        col = x - a.row_offsets[row];
        L = a.row_offsets[row + 1] - a.row_offsets[row];
    } else if (((x | L) >> 32) == 0) {   // the common case on 32-bit division
        row = static_cast<uint32_t>(x) / static_cast<uint32_t>(L);
        col = static_cast<uint32_t>(x) % static_cast<uint32_t>(L);
    } else {
        row = x / L;
        col = x % L;
    }
    const PackSlot s = pack_slot(a, a.hdr + kPackHdrWords * row, col, L);
    uint32_t id = s.id;
    if (s.source == kSlotA) id = a.a_ids[s.token];
    if (s.source == kSlotB) id = a.b_ids[s.token];
    pack_store(a.input_ids, a.width, x, id);
    pack_store(a.type_ids, a.width, x, s.type_id);
    pack_store(a.attention, a.width, x, s.source != kSlotPad);
    pack_store(a.special, a.width, x, s.source == kSlotPad || s.source == kSlotSpecial);
    if (a.offsets) {
        const unsigned long long *sp = s.source == kSlotA ? a.a_spans : s.source == kSlotB ? a.b_spans : nullptr;
        a.offsets[2 * x] = sp ? sp[2 * s.token] : 0;
        a.offsets[2 * x + 1] = sp ? sp[2 * s.token + 1] : 0;
    }
}

#ifndef DAAC_PACK_HOST
// hdr (and row_len with its closing 0) for the n_docs documents; the four words of a.fold, which the caller has cleared
hipError_t launch_pack_header(const PackArgs &a, hipStream_t stream);
// every plane's a.slots elements
hipError_t launch_pack_slots(const PackArgs &a, hipStream_t stream);
#endif

}  // namespace daac
