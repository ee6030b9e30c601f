// tokens_decode on the device (daac_tokens_decode): what api_decode.hip and decode_kernels.hip share, and the per-lane bodies of the kernels.
//
// The definition (include/daachorse_amd.h has it in full).  A decoder is a table over the ids 0 .. n_ids - 1: an image rest[id], an image
// first[id] and flags (special, absent), the images' bytes in one pool.  A document's token is kept unless it is special and
// skip_special is set, or its id has no entry and unknown_skip is set; the document's text is first[k_0] + rest[k_1] + rest[k_2] + ...
// over its kept tokens.  The tokens come as a CSR list (u32 ids, n + 1 u64 token offsets) or as a dense [n, L] plane of 4- or 8-byte
// elements, where an 8-byte element outside [0, 2^32) is an id without an entry.
//
// The passes.  sizing: one lane per token writes the length of the token's rest image (0 when it is not kept, or lies in no document)
// and a mark of 0, and folds the lowest flat index of a token without an entry and the number of kept tokens.  header: one lane per
// document checks the document's token range, walks to its first kept token, and overrides that token's length with the first image's
// and its mark with 1 — one store a document into what the sizing pass has written, which is why it runs behind it.  An exclusive sum of
// the lengths gives every token's start in the output; out_offsets[d] is the start of document d's first token.  tiles: one lane per
// output tile, the last token that begins at or before the tile's first byte.  copy: output-parallel, a workgroup a tile, a lane 16
// bytes and one aligned 16-byte store; output byte q belongs to the LARGEST i with start[i] <= q, which steps over empty images by
// itself.  Positions are 64-bit; every output byte and every scratch word but the three folded ones is written by the one lane that
// owns it.
//
// The per-lane bodies below are plain C++: with DAAC_DECODE_HOST defined this file compiles without HIP and a host program runs them
// document by document, token by token and lane by lane (tests/native/decode_check.cpp).
#pragma once

#include <cstdint>
#include <cstring>

#ifndef DAAC_DECODE_HOST
#include <hip/hip_runtime.h>
#define DECODE_FN static __host__ __device__ __forceinline__
#else
#define DECODE_FN static inline
#endif

namespace daac {

constexpr uint32_t kDecodeLanes = 256;                // lanes of a copy workgroup, 16 output bytes each: a wave's 64 stores cover 1 KiB without a gap
constexpr uint32_t kDecodeTile = kDecodeLanes * 16;   // output bytes a workgroup writes per turn: 4 KiB, 32 full 128-byte lines, and one search per tile
constexpr uint32_t kDecodeStage = 4096;               // token starts of a tile staged in LDS as 16-bit offsets into the tile (8 KB, so eight workgroups a
                                                      // CU keep theirs): a tile of 1-byte images fits; only one with empty images besides searches HBM
static_assert(kDecodeTile <= 0xFFFFu, "a staged start is a 16-bit offset of 1 .. kDecodeTile");
constexpr uint32_t kDecodeSizeLanes = 256;           // the launch shape of the passes with one lane per token / document / tile, as pack's
constexpr uint32_t kDecodeMaxBlocks = 2048;

enum : uint32_t { kDecodeSpecial = 1, kDecodeAbsent = 2 };   // DAAC_DECODE_SPECIAL, DAAC_DECODE_ABSENT
enum : uint32_t { kTokKept = 0, kTokSkipped = 1, kTokUnknown = 2 };
constexpr uint32_t kDecodeFoldWords = 3;   // {~first document in error, ~lowest flat index of a token without an entry, kept tokens}: max, max, sum

struct DecodePiece {   // daac_decode_piece: rest = pool[off, off + len), first = pool[first_off, first_off + first_len)
    uint32_t off, len, first_off, first_len;
};

struct DecodeArgs {
    const void *ids;                  // n_tokens elements of `width` bytes
    uint32_t width;                   // 4 or 8
    const unsigned long long *off;    // CSR: n_docs + 1 token offsets; NULL: dense rows of row_len tokens
    uint64_t row_len;
    uint64_t n_tokens;                // CSR: the tokens `ids` holds; dense: n_docs * row_len
    uint64_t n_docs;
    uint32_t skip_special, unknown_skip;
    // the decoder's table
    const DecodePiece *pieces;
    const uint8_t *flags;
    const uint8_t *pool;
    uint64_t pool_bytes;
    uint64_t n_ids;
    // the sizing and header passes
    unsigned long long *start;        // n_tokens + 1: the images' lengths with a closing 0, then (their exclusive sum) the tokens' starts and the total
    uint8_t *mark;                    // n_tokens: 1 = the token takes its first image
    unsigned long long *fold;         // kDecodeFoldWords, cleared
    unsigned long long *out_offsets;  // n_docs + 1
    // the copy pass
    uint8_t *out;                     // 16-byte aligned
    uint64_t out_len;
    long long *tile_lo;               // tiles + 1: the last token that begins at or before the tile's first byte; entry `tiles`: n_tokens - 1
    uint64_t tiles;
};

DECODE_FN uint64_t decode_min(uint64_t x, uint64_t y) { return x < y ? x : y; }

// token i: kept, skipped or without an entry; id: its id where it has an entry
DECODE_FN uint32_t decode_class(const DecodeArgs &a, uint64_t i, uint32_t &id) {
    id = 0;
    if (a.width == 8) {
        const uint64_t v = static_cast<const uint64_t *>(a.ids)[i];
        if (v >> 32) return kTokUnknown;   // negative, or 2^32 and above
        id = static_cast<uint32_t>(v);
    } else {
        id = static_cast<const uint32_t *>(a.ids)[i];
    }
    if (id >= a.n_ids) return kTokUnknown;
    const uint32_t f = a.flags[id];
    if (f & kDecodeAbsent) return kTokUnknown;
    return (f & kDecodeSpecial) && a.skip_special ? kTokSkipped : kTokKept;
}

// the tokens [lo, hi) that lie in a document at all, whatever the offsets say: inside the token list and not decreasing
DECODE_FN void decode_span(const DecodeArgs &a, uint64_t &lo, uint64_t &hi) {
    lo = 0;
    hi = a.n_tokens;
    if (a.off && a.n_docs) {
        lo = decode_min(a.off[0], a.n_tokens);
        hi = decode_min(a.off[a.n_docs], a.n_tokens);
        if (hi < lo) hi = lo;
    }
}

// document d's tokens [t0, t1); false: its offsets decrease or leave the token list
DECODE_FN bool decode_doc_tokens(const DecodeArgs &a, uint64_t d, uint64_t &t0, uint64_t &t1) {
    if (!a.off) {
        t0 = d * a.row_len;
        t1 = t0 + a.row_len;
        return true;
    }
    t0 = a.off[d];
    t1 = a.off[d + 1];
    if (t1 < t0 || t1 > a.n_tokens) { t0 = t1 = 0; return false; }
    return true;
}

struct DecodeSized {
    uint32_t kept, unknown;
};

// token i of n_tokens, of which [lo, hi) lie in documents: its rest image's length to a.start, its mark cleared
DECODE_FN DecodeSized decode_size_lane(const DecodeArgs &a, uint64_t i, uint64_t lo, uint64_t hi) {
    DecodeSized r{0, 0};
    uint64_t len = 0;
    if (i >= lo && i < hi) {
        uint32_t id;
        const uint32_t c = decode_class(a, i, id);
        if (c == kTokKept) { len = a.pieces[id].len; r.kept = 1; }
        r.unknown = c == kTokUnknown;
    }
    a.start[i] = len;
    a.mark[i] = 0;
    return r;
}

// document d: true if its token range is in order; its first kept token takes its first image (behind the sizing pass, before the sum)
DECODE_FN bool decode_header_lane(const DecodeArgs &a, uint64_t d) {
    uint64_t t0, t1;
    if (!decode_doc_tokens(a, d, t0, t1)) return false;
    for (uint64_t i = t0; i < t1; ++i) {
        uint32_t id;
        if (decode_class(a, i, id) != kTokKept) continue;
        a.start[i] = a.pieces[id].first_len;
        a.mark[i] = 1;
        break;
    }
    return true;
}

// out_offsets[d], d <= n_docs, behind the sum: the start of the document's first token (the closing entry: the total)
DECODE_FN void decode_doc_offset_lane(const DecodeArgs &a, uint64_t d) {
    uint64_t t = a.n_tokens;
    if (!a.off) t = d * a.row_len;
    else t = decode_min(a.off[d], a.n_tokens);   // (a batch in error is refused before this pass; the bound holds whatever the offsets say)
    a.out_offsets[d] = a.start[t];
}

// tile t of a.tiles + 1: the largest i in [0, n_tokens) with start[i] <= t * kDecodeTile (n_tokens >= 1 and start[0] = 0)
DECODE_FN void decode_tile_lane(const DecodeArgs &a, uint64_t t) {
    const uint64_t q = t * kDecodeTile;
    uint64_t lo = 0, hi = a.n_tokens;
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (a.start[mid] <= q) lo = mid; else hi = mid;
    }
    a.tile_lo[t] = static_cast<long long>(lo);
}

// The tile's tokens after k_lo are numbered j = 0 .. m - 1 (token k_lo + 1 + j); they begin inside the tile, at tile_begin + s_rel[j]
// when staged.  -> the first j in [lo, m] whose token begins beyond q.
template <bool STAGED>
DECODE_FN uint64_t decode_toks_up_to(const uint16_t *s_rel, const unsigned long long *after, uint64_t tile_begin, uint64_t lo, uint64_t m, uint64_t q) {
    uint64_t hi = m;
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        const uint64_t p = STAGED ? tile_begin + s_rel[mid] : after[mid];
        if (p <= q) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// lane `lane` of the workgroup that owns the tile at tile_begin: output bytes [tile_begin + 16 * lane, + 16), as far as the output goes
template <bool STAGED>
DECODE_FN void decode_copy_lane(const DecodeArgs &a, const uint16_t *s_rel, uint64_t tile_begin, long long k_lo, uint64_t m, uint32_t lane) {
    const uint64_t q0 = tile_begin + static_cast<uint64_t>(lane) * 16;
    if (q0 >= a.out_len) return;
    const unsigned long long *after = a.start + (k_lo + 1);
    uint64_t j = decode_toks_up_to<STAGED>(s_rel, after, tile_begin, 0, m, q0);   // the lane's first byte lies in token k_lo + j
    // the token in hand: it begins at output position o with len bytes of the pool from `at`; the next begins at `next`
    uint64_t o = 0, next = 0;
    uint32_t len = 0, at = 0;
    auto fetch = [&]() {
        const uint64_t s = static_cast<uint64_t>(k_lo) + j;
        o = a.start[s];
        len = 0;
        at = 0;
        uint32_t id;
        if (decode_class(a, s, id) == kTokKept) {   // (a token that owns a byte is a kept one: the check keeps a bad list out of the table)
            const DecodePiece pc = a.pieces[id];
            const bool f = a.mark[s] != 0;
            at = f ? pc.first_off : pc.off;
            len = f ? pc.first_len : pc.len;
        }
        next = j < m ? (STAGED ? tile_begin + s_rel[j] : after[j]) : ~0ull;
    };
    fetch();
    const uint64_t left = a.out_len - q0;
    const uint32_t n = left < 16 ? static_cast<uint32_t>(left) : 16u;
    if (n == 16 && q0 + 16 <= next) {   // 16 bytes of one image: long pieces
        const uint64_t p = static_cast<uint64_t>(at) + (q0 - o);
        if (q0 - o + 16 <= len && p + 16 <= a.pool_bytes) {
#ifndef DAAC_DECODE_HOST
            uint4 v;
            __builtin_memcpy(&v, a.pool + p, 16);   // (any alignment)
            *reinterpret_cast<uint4 *>(a.out + q0) = v;
#else
            memcpy(a.out + q0, a.pool + p, 16);
#endif
            return;
        }
    }
    uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
    for (uint32_t x = 0; x < 4; ++x) {
#pragma unroll
        for (uint32_t y = 0; y < 4; ++y) {
            const uint32_t b = 4 * x + y;
            if (b < n) {
                const uint64_t q = q0 + b;
                if (q >= next) {   // one step first; a binary search when more tokens begin at or before q
                    ++j;
                    if (j < m && (STAGED ? tile_begin + s_rel[j] : after[j]) <= q) j = decode_toks_up_to<STAGED>(s_rel, after, tile_begin, j + 1, m, q);
                    fetch();
                }
                const uint64_t d = q - o, p = static_cast<uint64_t>(at) + d;
                uint32_t c = 0;   // (both checks hold by construction; a read outside the pool must not happen whatever the lists say)
                if (d < len && p < a.pool_bytes) c = a.pool[p];
                w[x] |= c << (8 * y);
            }
        }
    }
    if (n == 16) {
#ifndef DAAC_DECODE_HOST
        *reinterpret_cast<uint4 *>(a.out + q0) = make_uint4(w[0], w[1], w[2], w[3]);
#else
        memcpy(a.out + q0, w, 16);
#endif
    } else {   // the result's last granule
#pragma unroll
        for (uint32_t x = 0; x < 4; ++x) {
#pragma unroll
            for (uint32_t y = 0; y < 4; ++y)
                if (4 * x + y < n) a.out[q0 + 4 * x + y] = static_cast<uint8_t>(w[x] >> (8 * y));
        }
    }
}

// the tokens after k_lo that begin in (tile_begin, tile_begin + kDecodeTile]: what a workgroup stages when there are at most kDecodeStage
DECODE_FN uint64_t decode_tile_tokens(const DecodeArgs &a, uint64_t t, long long &k_lo) {
    k_lo = a.tile_lo[t];
    return static_cast<uint64_t>(a.tile_lo[t + 1] - k_lo);
}

#ifndef DAAC_DECODE_HOST
// a.start (lengths, closing 0) and a.mark for the n_tokens tokens; words 1 and 2 of a.fold, which the caller has cleared
hipError_t launch_decode_size(const DecodeArgs &a, hipStream_t stream);
// the documents' token ranges checked, their first kept tokens' lengths and marks overridden; word 0 of a.fold
hipError_t launch_decode_header(const DecodeArgs &a, hipStream_t stream);
// behind the sum: a.out_offsets
hipError_t launch_decode_doc_offsets(const DecodeArgs &a, hipStream_t stream);
// tile_lo (one lane per tile: a binary search in the starts), then the copy itself
hipError_t launch_decode_copy(const DecodeArgs &a, uint32_t num_cu, hipStream_t stream);
#endif

}  // namespace daac
