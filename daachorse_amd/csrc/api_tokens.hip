// The back door of the calls that return a token list (daac_tokenize, daac_tokenize_bpe, daac_tokenize_unigram, daac_tokenize_wordpiece,
// each with its _batch, and daac_tokens_splice): the one read-back of the totals, the two limits, the result buffers and their hand-over
// to the caller; and what the three lattice tokenizers (bpe, unigram, wordpiece) share in front of that: the overlapping scan that is
// their piece lattice and the carve of their scratch.  Declared in api_internal.hpp ("api_tokens.hip"), where the templates that run
// these steps in order are; DESIGN.md, "The token calls' back door".  No kernel is launched here.
#include "api_internal.hpp"

namespace daac {
namespace api {

daac_status read_totals(const unsigned long long *dev, unsigned count, hipStream_t stream, unsigned long long *out) {
    unsigned long long *pin = reinterpret_cast<unsigned long long *>(pinned_words());   // (64 bytes: count <= 8)
    unsigned long long *h = pin ? pin : out;
    HIP_TRY(hipMemcpyAsync(h, dev, count * sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    if (pin) std::copy(pin, pin + count, out);
    return DAAC_OK;
}

daac_status alloc_tok_offsets(uint64_t n_docs, hipStream_t stream, TokenBufs &r) {
    void *p = nullptr;
    HIP_TRY(dev_malloc(&p, (n_docs + 1) * sizeof(uint64_t), stream));
    r.tok_offsets = dev_guard(p, stream);
    return DAAC_OK;
}

daac_status token_buffers(uint64_t total, uint64_t fit, bool want_spans, bool offsets, uint64_t n_docs, hipStream_t stream, TokenBufs &r) {
    if (total > fit) { set_error("the token count does not fit the text"); return DAAC_ERR_DEVICE; }   // (never seen: every token has a byte)
    const uint64_t per_token = sizeof(uint32_t) + (want_spans ? 2 * sizeof(uint64_t) : 0);
    if (total > static_cast<uint64_t>(OPT(max_result_bytes)) / per_token) {
        set_error("the result of " + std::to_string(total) + " tokens exceeds max_result_bytes");
        return DAAC_ERR_AUTOMATON_SCALE;
    }
    void *ids = nullptr, *spans = nullptr;
    if (total) HIP_TRY(dev_malloc(&ids, total * sizeof(uint32_t), stream));
    r.ids = dev_guard(ids, stream);
    if (total && want_spans) HIP_TRY(dev_malloc(&spans, total * 2 * sizeof(uint64_t), stream));
    r.spans = dev_guard(spans, stream);
    return offsets ? alloc_tok_offsets(n_docs, stream, r) : DAAC_OK;
}

void hand_over(TokenBufs &r, const TokenOuts &o, uint64_t total, uint64_t matches) {
    *o.dev_ids = static_cast<uint32_t *>(r.ids.release());
    if (o.dev_spans) *o.dev_spans = static_cast<uint64_t *>(r.spans.release());
    if (o.dev_tok_offsets) *o.dev_tok_offsets = static_cast<uint64_t *>(r.tok_offsets.release());
    *o.n_tokens = total;
    *o.n_matches = matches;
}

daac_status lattice_scan(const LatticeIn &in, TupleList &tl, uint64_t *k) {
    return daac_scan_batch_device16(in.pma, DAAC_FIND_OVERLAPPING, in.engine, in.dev_hay, reinterpret_cast<const uint64_t *>(in.d_off), in.n, 1, in.stream,
                                    reinterpret_cast<daac_match16 **>(&tl.list), &tl.doc_first, k);
}

daac_status carve_lattice(size_t front_bytes, size_t behind_bytes, uint64_t m, hipStream_t stream, LatticeScratch &s) {
    assert(front_bytes % sizeof(unsigned long long) == 0);
    const uint64_t words = 2 + m + exclusive_scan_scratch(m);
    HIP_TRY(s.buf.alloc(front_bytes + words * sizeof(unsigned long long) + behind_bytes, stream));
    s.front = s.buf.p;
    s.hdr = reinterpret_cast<unsigned long long *>(static_cast<char *>(s.buf.p) + front_bytes);
    s.own_off = s.hdr + 2;
    s.scan = s.own_off + m;
    s.behind = s.hdr + words;
    return DAAC_OK;
}

daac_status no_document(daac_pma *pma, int mode, int engine, const uint8_t *hay, const uint64_t *offsets, int hay_is_device, hipStream_t stream, const char *line,
                        const TokenOuts &o) {
    TupleList tl(stream);
    uint64_t k = 0;
    daac_status st = daac_scan_batch_device16(pma, mode, engine, hay, offsets, 0, hay_is_device, stream, reinterpret_cast<daac_match16 **>(&tl.list), &tl.doc_first, &k);
    if (st != DAAC_OK) return st;
    *o.dev_tok_offsets = tl.doc_first;
    tl.doc_first = nullptr;
    g_last_kernel = std::string(line) + g_last_kernel;
    return DAAC_OK;
}

}  // namespace api
}  // namespace daac
