// daachorse_amd.hpp — header-only C++17 façade over the C ABI (include/daachorse_amd.h).
//
// The reference is a Rust crate; no Rust toolchain exists in this image, so the host side that a
// crate user would touch is mirrored here in C++ with the crate's names, argument meaning and
// error behaviour (reference src/bytewise.rs, src/bytewise/builder.rs, src/bytewise/iter.rs and their
// src/charwise* twins):
//
//     auto pma = daachorse::DoubleArrayAhoCorasick::new_({"bcd", "ab", "a"}).value();
//     for (auto it = pma.find_overlapping_iter("abcd"); auto m = it.next();)
//         use(m->start(), m->end(), m->value());
//
//   * construction / deserialisation return Result<T> (a value or a DaachorseError), like the
//     crate's `Result<_, DaachorseError>` (src/errors.rs:10-22, 140);
//   * calling a query of the wrong MatchKind PANICS in the crate (bytewise.rs:194-197, 299-302,
//     551-554): here it throws daachorse::PanicError carrying the crate's message;
//   * iterators are lazy (`next()`), borrow the automaton, and keep the haystack alive.
// Every scan runs on the MI355X; there is no CPU scan path behind this header.
#pragma once

#include <algorithm>
#include <cstdint>
#include <memory>
#include <optional>
#include <stdexcept>
#include <string>
#include <string_view>
#include <utility>
#include <variant>
#include <vector>

#include "daachorse_amd.h"

namespace daachorse {

enum class MatchKind : uint8_t { Standard = 0, LeftmostLongest = 1, LeftmostFirst = 2 };  // src/lib.rs:324-346

struct DaachorseError {  // src/errors.rs:10-22
    enum Kind { InvalidArgument = 1, AutomatonScale = 2, InvalidConversion = 3, InvalidAutomaton = 4, Unsupported = 6, Device = 7 } kind;
    std::string message;
};

struct PanicError : std::runtime_error {  // the crate's assert!/panic! paths
    using std::runtime_error::runtime_error;
};

template <class T>
class Result {
public:
    Result(T v) : v_(std::move(v)) {}
    Result(DaachorseError e) : v_(std::move(e)) {}
    bool is_ok() const { return v_.index() == 0; }
    bool is_err() const { return !is_ok(); }
    T &value() {
        if (is_err()) throw PanicError("called `Result::unwrap()` on an `Err` value: " + std::get<1>(v_).message);
        return std::get<0>(v_);
    }
    T unwrap() { return std::move(value()); }
    const DaachorseError &error() const { return std::get<1>(v_); }

private:
    std::variant<T, DaachorseError> v_;
};

class Match {  // src/lib.rs:286-320
public:
    Match(uint64_t s, uint64_t e, uint32_t v) : s_(s), e_(e), v_(v) {}
    uint64_t start() const { return s_; }
    uint64_t end() const { return e_; }
    uint32_t value() const { return v_; }
    bool operator==(const Match &o) const { return s_ == o.s_ && e_ == o.e_ && v_ == o.v_; }

private:
    uint64_t s_, e_;
    uint32_t v_;
};

namespace detail {
inline DaachorseError make_error(daac_status st) {
    const char *m = daac_last_error();
    return DaachorseError{static_cast<DaachorseError::Kind>(st), m ? m : ""};
}
struct PmaDeleter { void operator()(daac_pma *p) const { daac_pma_free(p); } };
struct IterDeleter { void operator()(daac_iter *p) const { daac_iter_close(p); } };
}  // namespace detail

// Iterator<Item = Match<u32>>: FindIterator / FindOverlappingIterator / FindOverlappingNoSuffixIterator /
// LeftmostFindIterator of src/bytewise/iter.rs, one type here because the device engine sits behind them.
class MatchIterator {
public:
    // one 8-byte read from the run at hand (the compact iterator: {value, end relative to the run's base | length << end_bits}: half the
    // bytes over PCIe); a library call per window of the haystack (daac_iter_next_batch8), not per match.  Dictionaries with patterns of
    // several KB have no compact form: 16-byte runs then.
    std::optional<Match> next() {
        if (run_n_ == 0) {
            const int r = compact_ ? daac_iter_next_batch8(it_.get(), &run8_, &run_n_, &base_, &end_bits_) : daac_iter_next_batch(it_.get(), &run16_, &run_n_);
            if (r == 0) return std::nullopt;
            if (r < 0) throw PanicError(std::string("device scan failed: ") + daac_last_error());
        }
        --run_n_;
        if (!compact_) {
            const daac_match16 t = *run16_++;
            return Match(t.end - t.length, t.end, t.value);
        }
        const daac_match8 t = *run8_++;
        const uint64_t end = base_ + (t.end_len & ((1u << end_bits_) - 1u));
        return Match(end - (t.end_len >> end_bits_), end, t.value);
    }
    std::vector<Match> collect() {
        std::vector<Match> out;
        while (auto m = next()) out.push_back(*m);
        return out;
    }

private:
    template <class F>
    friend class BasicAhoCorasick;
    MatchIterator(daac_iter *it, std::unique_ptr<std::string> hay, bool compact) : hay_(std::move(hay)), it_(it), compact_(compact) {}
    std::unique_ptr<std::string> hay_;  // the haystack lives (at a stable address) as long as the iterator (the crate's `P`)
    std::unique_ptr<daac_iter, detail::IterDeleter> it_;
    bool compact_ = true;
    const daac_match8 *run8_ = nullptr;    // what is left of the last run (a view of the iterator's window buffer)
    const daac_match16 *run16_ = nullptr;
    size_t run_n_ = 0;
    uint64_t base_ = 0;
    uint32_t end_bits_ = 32;
};

// FindStepper / FindOverlappingStepper (src/bytewise/iter.rs:344-475, src/charwise/iter.rs:403-534), fed a chunk
// at a time: feed() returns the matches decided so far, positions counted from the first byte ever fed.
class Stepper {
public:
    std::vector<Match> feed(std::string_view chunk) {
        daac_matches *m = nullptr;
        const daac_status st = daac_stream_feed(s_.get(), reinterpret_cast<const uint8_t *>(chunk.data()), chunk.size(), 0, &m);
        if (st != DAAC_OK) throw PanicError(std::string("device scan failed: ") + daac_last_error());
        std::vector<Match> out;
        const daac_match *p = daac_matches_data(m);
        for (size_t i = 0, n = daac_matches_count(m); i < n; ++i) out.emplace_back(p[i].start, p[i].end, p[i].value);
        daac_matches_free(m);
        return out;
    }

private:
    template <class F>
    friend class BasicAhoCorasick;
    struct Closer { void operator()(daac_stream *s) const { daac_stream_close(s); } };
    explicit Stepper(daac_stream *s) : s_(s) {}
    std::unique_ptr<daac_stream, Closer> s_;
};

namespace detail {
// Which pair of C entry points builds / parses the automaton behind a handle (the scans are shared).
struct Bytewise {  // src/bytewise.rs, src/bytewise/builder.rs
    static daac_status parse(const uint8_t *b, size_t n, daac_pma **h, size_t *used) { return daac_bytewise_from_serialized(b, n, h, used); }
    static daac_status build(const uint8_t *b, const uint64_t *o, const uint32_t *v, size_t n, uint8_t k, uint32_t f, daac_pma **h) {
        return daac_bytewise_build(b, o, v, n, k, f, h);
    }
};
struct Charwise {  // src/charwise.rs, src/charwise/builder.rs
    static daac_status parse(const uint8_t *b, size_t n, daac_pma **h, size_t *used) { return daac_charwise_from_serialized(b, n, h, used); }
    static daac_status build(const uint8_t *b, const uint64_t *o, const uint32_t *v, size_t n, uint8_t k, uint32_t f, daac_pma **h) {
        return daac_charwise_build(b, o, v, n, k, f, h);
    }
};
}  // namespace detail

template <class Flavor>
class BasicBuilder;

// DoubleArrayAhoCorasick<u32> (src/bytewise.rs:54-68) and CharwiseDoubleArrayAhoCorasick<u32>
// (src/charwise.rs:59-65): the same surface; charwise haystacks and patterns are UTF-8, positions are bytes.
template <class Flavor>
class BasicAhoCorasick {
public:
    // bytewise.rs:103-110 / 154-161, charwise.rs:87-94 / 139-146 (`new` is a keyword in C++)
    static Result<BasicAhoCorasick> new_(const std::vector<std::string> &patterns) { return BasicBuilder<Flavor>().build(patterns); }
    static Result<BasicAhoCorasick> with_values(const std::vector<std::pair<std::string, uint32_t>> &patvals) {
        return BasicBuilder<Flavor>().build_with_values(patvals);
    }

    // bytewise.rs:868-964, charwise.rs:896-952: (automaton, bytes consumed)
    static Result<std::pair<BasicAhoCorasick, size_t>> deserialize(std::string_view source) {
        daac_pma *h = nullptr;
        size_t consumed = 0;
        const daac_status st = Flavor::parse(reinterpret_cast<const uint8_t *>(source.data()), source.size(), &h, &consumed);
        if (st != DAAC_OK) return detail::make_error(st);
        return std::make_pair(BasicAhoCorasick(h), consumed);
    }
    std::string serialize() const {  // bytewise.rs:801-820, charwise.rs:831-848
        uint8_t *buf = nullptr;
        size_t len = 0;
        if (daac_pma_serialize(h_.get(), &buf, &len) != DAAC_OK) throw PanicError(daac_last_error());
        std::string out(reinterpret_cast<char *>(buf), len);
        daac_free(buf);
        return out;
    }

    MatchIterator find_iter(std::string haystack) const { return open(DAAC_FIND, std::move(haystack), "Error: match_kind must be standard."); }
    MatchIterator find_overlapping_iter(std::string haystack) const {
        return open(DAAC_FIND_OVERLAPPING, std::move(haystack), "Error: match_kind must be standard.");
    }
    MatchIterator find_overlapping_no_suffix_iter(std::string haystack) const {
        return open(DAAC_FIND_OVERLAPPING_NO_SUFFIX, std::move(haystack), "Error: match_kind must be standard.");
    }
    MatchIterator leftmost_find_iter(std::string haystack) const {
        return open(DAAC_LEFTMOST_FIND, std::move(haystack), "Error: match_kind must be leftmost.");
    }

    // `pma.find_overlapping_iter(h).count()` and its three siblings without materialising a match (Iterator::count on the
    // iterators of src/bytewise/iter.rs / src/charwise/iter.rs): one device pass, nothing but the number comes back.
    size_t find_iter_count(std::string_view haystack) const { return count(DAAC_FIND, haystack, "Error: match_kind must be standard."); }
    size_t find_overlapping_iter_count(std::string_view haystack) const {
        return count(DAAC_FIND_OVERLAPPING, haystack, "Error: match_kind must be standard.");
    }
    size_t find_overlapping_no_suffix_iter_count(std::string_view haystack) const {
        return count(DAAC_FIND_OVERLAPPING_NO_SUFFIX, haystack, "Error: match_kind must be standard.");
    }
    size_t leftmost_find_iter_count(std::string_view haystack) const {
        return count(DAAC_LEFTMOST_FIND, haystack, "Error: match_kind must be leftmost.");
    }

    // The whole match list of find_overlapping_iter, in the iterator's order, left in device memory for a consumer that
    // runs on the GPU (daac_scan_device); `haystack_dev` is a device pointer.  to_host() copies a slice back.
    class DeviceMatches {
    public:
        DeviceMatches(DeviceMatches &&o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr; o.n_ = 0; }
        DeviceMatches(const DeviceMatches &) = delete;
        ~DeviceMatches() { daac_device_free(p_); }
        const daac_match *data() const { return p_; }  // device pointer
        size_t size() const { return n_; }
        std::vector<Match> to_host(size_t first, size_t n) const {
            if (first > n_ || n > n_ - first) throw std::out_of_range("DeviceMatches::to_host");
            std::vector<daac_match> raw(n);
            if (n && daac_device_to_host(raw.data(), p_ + first, n * sizeof(daac_match)) != DAAC_OK) throw PanicError(daac_last_error());
            std::vector<Match> out;
            out.reserve(n);
            for (const auto &m : raw) out.emplace_back(m.start, m.end, m.value);
            return out;
        }

    private:
        friend class BasicAhoCorasick;
        DeviceMatches(daac_match *p, size_t n) : p_(p), n_(n) {}
        daac_match *p_;
        size_t n_;
    };
    DeviceMatches find_overlapping_device(const uint8_t *haystack_dev, size_t len, void *stream = nullptr) const {
        return scan_device(haystack_dev, len, 1, stream);
    }
    DeviceMatches find_overlapping_device(std::string_view host_haystack) const {  // the haystack is copied over first
        return scan_device(reinterpret_cast<const uint8_t *>(host_haystack.data()), host_haystack.size(), 0, nullptr);
    }

    // replace_all over find_iter (Standard) / leftmost_find_iter (the leftmost kinds), spliced on the device (daac_replace_all[_batch]):
    // one replacement for every match, or one per value (automata built without values: per pattern index).  A batch replaces every
    // document as a haystack of its own.
    std::string replace_all(std::string_view haystack, const std::vector<std::string> &replacements) const {
        const Replacements r(replacements);
        uint8_t *p = nullptr;
        uint64_t n = 0, k = 0;
        replace_check(daac_replace_all(h_.get(), replace_mode(), DAAC_ENGINE_AUTO, reinterpret_cast<const uint8_t *>(haystack.data()), haystack.size(), 0, nullptr,
                                       r.blob(), r.offs.data(), replacements.size(), &p, &n, &k));
        return replace_fetch(p, n);
    }
    std::vector<std::string> replace_all_batch(const std::vector<std::string> &docs, const std::vector<std::string> &replacements) const {
        const Replacements r(replacements), d(docs);
        uint8_t *p = nullptr;
        uint64_t *po = nullptr, n = 0, k = 0;
        replace_check(daac_replace_all_batch(h_.get(), replace_mode(), DAAC_ENGINE_AUTO, d.blob(), d.offs.data(), docs.size(), 0, nullptr, r.blob(), r.offs.data(),
                                             replacements.size(), &p, &po, &n, &k));
        std::vector<uint64_t> o(docs.size() + 1);
        const daac_status st = daac_device_to_host(o.data(), po, o.size() * sizeof(uint64_t));
        daac_device_free(po);
        if (st != DAAC_OK) { daac_device_free(p); throw PanicError(daac_last_error()); }
        const std::string all = replace_fetch(p, n);
        std::vector<std::string> out;
        for (size_t i = 0; i < docs.size(); ++i) out.push_back(all.substr(o[i], o[i + 1] - o[i]));
        return out;
    }

    // tokenize over find_iter (Standard) / leftmost_find_iter (the leftmost kinds) on the device (daac_tokenize[_batch]): the matches'
    // values and what `gap` makes of the text between them, as one id list.  A batch tokenizes every document as a haystack of its own
    // and returns the ids of all documents with n + 1 offsets into them.
    std::vector<uint32_t> tokenize(std::string_view haystack, daac_gap gap = DAAC_GAP_UNK, uint32_t gap_id = 0) const {
        uint32_t *p = nullptr;
        uint64_t n = 0, k = 0;
        tokenize_check(daac_tokenize(h_.get(), replace_mode(), DAAC_ENGINE_AUTO, reinterpret_cast<const uint8_t *>(haystack.data()), haystack.size(), 0, nullptr,
                                     gap, gap_id, &p, nullptr, &n, &k));
        return tokenize_fetch(p, n);
    }
    std::pair<std::vector<uint32_t>, std::vector<uint64_t>> tokenize_batch(const std::vector<std::string> &docs, daac_gap gap = DAAC_GAP_UNK,
                                                                            uint32_t gap_id = 0) const {
        const Replacements d(docs);
        uint32_t *p = nullptr;
        uint64_t *po = nullptr, n = 0, k = 0;
        tokenize_check(daac_tokenize_batch(h_.get(), replace_mode(), DAAC_ENGINE_AUTO, d.blob(), d.offs.data(), docs.size(), 0, nullptr, gap, gap_id, &p, nullptr,
                                           &po, &n, &k));
        std::vector<uint64_t> o(docs.size() + 1);
        const daac_status st = daac_device_to_host(o.data(), po, o.size() * sizeof(uint64_t));
        daac_device_free(po);
        if (st != DAAC_OK) { daac_device_free(p); throw PanicError(daac_last_error()); }
        return {tokenize_fetch(p, n), std::move(o)};
    }

    // The segmentation whose pieces' scores sum highest (daac_tokenize_unigram[_batch]; Standard automata): a Viterbi pass over the
    // overlapping matches with `scores[value]` per match and `unk_score` per unknown piece (a byte, or a UTF-8 code point).  `score`
    // receives the path's score.  A batch segments every document on its own and returns all ids with n + 1 offsets into them.
    std::vector<uint32_t> tokenize_unigram(std::string_view haystack, const std::vector<float> &scores, float unk_score, daac_gap gap = DAAC_GAP_CHARS,
                                           uint32_t gap_id = 0, float *score = nullptr) const {
        uint32_t *p = nullptr;
        uint64_t n = 0, k = 0;
        tokenize_check(daac_tokenize_unigram(h_.get(), DAAC_ENGINE_AUTO, reinterpret_cast<const uint8_t *>(haystack.data()), haystack.size(), 0, nullptr,
                                             scores.data(), scores.size(), unk_score, gap, gap_id, &p, nullptr, &n, &k, score));
        return tokenize_fetch(p, n);
    }
    std::pair<std::vector<uint32_t>, std::vector<uint64_t>> tokenize_unigram_batch(const std::vector<std::string> &docs, const std::vector<float> &scores,
                                                                                    float unk_score, daac_gap gap = DAAC_GAP_CHARS, uint32_t gap_id = 0) const {
        const Replacements d(docs);
        uint32_t *p = nullptr;
        uint64_t *po = nullptr, n = 0, k = 0;
        tokenize_check(daac_tokenize_unigram_batch(h_.get(), DAAC_ENGINE_AUTO, d.blob(), d.offs.data(), docs.size(), 0, nullptr, scores.data(), scores.size(),
                                                   unk_score, gap, gap_id, &p, nullptr, &po, nullptr, &n, &k));
        std::vector<uint64_t> o(docs.size() + 1);
        const daac_status st = daac_device_to_host(o.data(), po, o.size() * sizeof(uint64_t));
        daac_device_free(po);
        if (st != DAAC_OK) { daac_device_free(p); throw PanicError(daac_last_error()); }
        return {tokenize_fetch(p, n), std::move(o)};
    }

    // Byte-pair merging in rank order (daac_tokenize_bpe[_batch]; Standard automata): what tiktoken's byte_pair_merge gives for one piece
    // of pre-split text.  `ranks[value]` is a piece's rank (empty: its value); a part the vocabulary lacks becomes a byte or a UTF-8 code
    // point (`gap`).  A document above the handle's option bpe_doc_max is refused.  A batch merges every document on its own and returns
    // all ids with n + 1 offsets into them.
    std::vector<uint32_t> tokenize_bpe(std::string_view haystack, const std::vector<uint32_t> &ranks = {}, daac_gap gap = DAAC_GAP_BYTES,
                                       uint32_t gap_id = 0) const {
        uint32_t *p = nullptr;
        uint64_t n = 0, k = 0;
        tokenize_check(daac_tokenize_bpe(h_.get(), DAAC_ENGINE_AUTO, reinterpret_cast<const uint8_t *>(haystack.data()), haystack.size(), 0, nullptr,
                                         ranks.empty() ? nullptr : ranks.data(), ranks.size(), gap, gap_id, &p, nullptr, &n, &k));
        return tokenize_fetch(p, n);
    }
    std::pair<std::vector<uint32_t>, std::vector<uint64_t>> tokenize_bpe_batch(const std::vector<std::string> &docs, const std::vector<uint32_t> &ranks = {},
                                                                                daac_gap gap = DAAC_GAP_BYTES, uint32_t gap_id = 0) const {
        const Replacements d(docs);
        uint32_t *p = nullptr;
        uint64_t *po = nullptr, n = 0, k = 0;
        tokenize_check(daac_tokenize_bpe_batch(h_.get(), DAAC_ENGINE_AUTO, d.blob(), d.offs.data(), docs.size(), 0, nullptr,
                                               ranks.empty() ? nullptr : ranks.data(), ranks.size(), gap, gap_id, &p, nullptr, &po, &n, &k));
        std::vector<uint64_t> o(docs.size() + 1);
        const daac_status st = daac_device_to_host(o.data(), po, o.size() * sizeof(uint64_t));
        daac_device_free(po);
        if (st != DAAC_OK) { daac_device_free(p); throw PanicError(daac_last_error()); }
        return {tokenize_fetch(p, n), std::move(o)};
    }

    // BERT's WordPiece (daac_tokenize_wordpiece[_batch]; Standard automata): greedy longest-match-first over the initial pieces
    // (`first_ids[value]`) and the continuation pieces (`cont_ids[value]`; 0xFFFFFFFF: no such piece) of one word of pre-split text.  A
    // word with a position no piece covers, or of more than `max_chars` characters, is the one token `unk_id`.  A batch segments every
    // word on its own and returns all ids with n + 1 offsets into them.
    std::vector<uint32_t> tokenize_wordpiece(std::string_view word, const std::vector<uint32_t> &first_ids, const std::vector<uint32_t> &cont_ids, uint32_t unk_id,
                                             uint32_t max_chars = 100) const {
        uint32_t *p = nullptr;
        uint64_t n = 0, k = 0;
        tokenize_check(daac_tokenize_wordpiece(h_.get(), DAAC_ENGINE_AUTO, reinterpret_cast<const uint8_t *>(word.data()), word.size(), 0, nullptr, first_ids.data(),
                                               cont_ids.data(), std::min(first_ids.size(), cont_ids.size()), unk_id, max_chars, &p, nullptr, &n, &k));
        return tokenize_fetch(p, n);
    }
    std::pair<std::vector<uint32_t>, std::vector<uint64_t>> tokenize_wordpiece_batch(const std::vector<std::string> &words, const std::vector<uint32_t> &first_ids,
                                                                                      const std::vector<uint32_t> &cont_ids, uint32_t unk_id,
                                                                                      uint32_t max_chars = 100) const {
        const Replacements d(words);
        uint32_t *p = nullptr;
        uint64_t *po = nullptr, n = 0, k = 0;
        tokenize_check(daac_tokenize_wordpiece_batch(h_.get(), DAAC_ENGINE_AUTO, d.blob(), d.offs.data(), words.size(), 0, nullptr, first_ids.data(), cont_ids.data(),
                                                     std::min(first_ids.size(), cont_ids.size()), unk_id, max_chars, nullptr, &p, nullptr, &po, &n, &k));
        std::vector<uint64_t> o(words.size() + 1);
        const daac_status st = daac_device_to_host(o.data(), po, o.size() * sizeof(uint64_t));
        daac_device_free(po);
        if (st != DAAC_OK) { daac_device_free(p); throw PanicError(daac_last_error()); }
        return {tokenize_fetch(p, n), std::move(o)};
    }

    // bytewise.rs:238-251, 353-375 / charwise.rs: steppers for text that arrives in pieces
    Stepper find_stepper() const { return open_stepper(DAAC_FIND); }
    Stepper find_overlapping_stepper() const { return open_stepper(DAAC_FIND_OVERLAPPING); }

    MatchKind match_kind() const { return static_cast<MatchKind>(info().match_kind); }
    size_t num_states() const { return info().num_states; }
    size_t heap_bytes() const { return info().heap_bytes; }
    daac_pma *raw() const { return h_.get(); }

private:
    friend class BasicBuilder<Flavor>;
    explicit BasicAhoCorasick(daac_pma *h) : h_(h) {}
    daac_info info() const {
        daac_info i;
        i.struct_size = static_cast<uint32_t>(sizeof(i));
        daac_pma_info(h_.get(), &i);
        return i;
    }
    size_t count(int mode, std::string_view hay, const char *panic_msg) const {
        uint64_t n = 0;
        const daac_status st = daac_scan_count_only_range(h_.get(), mode, DAAC_ENGINE_AUTO, reinterpret_cast<const uint8_t *>(hay.data()),
                                                          hay.size(), 0, 0, nullptr, &n, nullptr);
        if (st == DAAC_ERR_MATCH_KIND) throw PanicError(panic_msg);
        if (st != DAAC_OK) throw PanicError(std::string("device scan failed: ") + daac_last_error());
        return n;
    }
    DeviceMatches scan_device(const uint8_t *hay, size_t len, int on_device, void *stream) const {
        daac_match *p = nullptr;
        uint64_t n = 0;
        const daac_status st = daac_scan_device(h_.get(), DAAC_FIND_OVERLAPPING, DAAC_ENGINE_AUTO, hay, len, on_device, stream, &p, &n);
        if (st == DAAC_ERR_MATCH_KIND) throw PanicError("Error: match_kind must be standard.");
        if (st != DAAC_OK) throw PanicError(std::string("device scan failed: ") + daac_last_error());
        return DeviceMatches(p, n);
    }
    struct Replacements {   // strings as one blob + n + 1 offsets
        std::string bytes;
        std::vector<uint64_t> offs{0};
        explicit Replacements(const std::vector<std::string> &v) { for (const auto &s : v) { bytes += s; offs.push_back(bytes.size()); } }
        const uint8_t *blob() const { return reinterpret_cast<const uint8_t *>(bytes.data()); }
    };
    int replace_mode() const { return match_kind() == MatchKind::Standard ? DAAC_FIND : DAAC_LEFTMOST_FIND; }
    static void replace_check(daac_status st) {
        if (st != DAAC_OK) throw PanicError(std::string("replace_all failed: ") + daac_last_error());
    }
    static std::string replace_fetch(uint8_t *p, uint64_t n) {   // the device result to the host, and released
        std::string out(n, '\0');
        const daac_status st = daac_device_to_host(out.data(), p, n);
        daac_device_free(p);
        if (st != DAAC_OK) throw PanicError(daac_last_error());
        return out;
    }
    static void tokenize_check(daac_status st) {
        if (st != DAAC_OK) throw PanicError(std::string("tokenize failed: ") + daac_last_error());
    }
    static std::vector<uint32_t> tokenize_fetch(uint32_t *p, uint64_t n) {   // the device result to the host, and released
        std::vector<uint32_t> out(n);
        const daac_status st = daac_device_to_host(out.data(), p, n * sizeof(uint32_t));
        daac_device_free(p);
        if (st != DAAC_OK) throw PanicError(daac_last_error());
        return out;
    }
    Stepper open_stepper(int mode) const {
        daac_stream *st = nullptr;
        const daac_status rc = daac_stream_open(h_.get(), mode, DAAC_ENGINE_AUTO, nullptr, &st);
        if (rc == DAAC_ERR_MATCH_KIND) throw PanicError("Error: match_kind must be standard.");
        if (rc != DAAC_OK) throw PanicError(std::string("device scan failed: ") + daac_last_error());
        return Stepper(st);
    }
    MatchIterator open(int mode, std::string hay, const char *panic_msg) const {
        auto keep = std::make_unique<std::string>(std::move(hay));
        daac_iter *it = nullptr;
        bool compact = true;
        daac_status st = daac_iter_open_compact(h_.get(), mode, DAAC_ENGINE_AUTO, reinterpret_cast<const uint8_t *>(keep->data()), keep->size(),
                                                0, nullptr, &it);
        if (st == DAAC_ERR_UNSUPPORTED) {   // (patterns of several KB: the 16-byte runs)
            compact = false;
            st = daac_iter_open(h_.get(), mode, DAAC_ENGINE_AUTO, reinterpret_cast<const uint8_t *>(keep->data()), keep->size(), 0, nullptr, &it);
        }
        if (st == DAAC_ERR_MATCH_KIND) throw PanicError(panic_msg);
        if (st != DAAC_OK) throw PanicError(std::string("device scan failed: ") + daac_last_error());
        return MatchIterator(it, std::move(keep), compact);
    }
    std::unique_ptr<daac_pma, detail::PmaDeleter> h_;
};

template <class Flavor>
class BasicBuilder {  // src/bytewise/builder.rs:21-244, src/charwise/builder.rs:20-239
public:
    BasicBuilder &match_kind(MatchKind k) { kind_ = k; return *this; }
    BasicBuilder &num_free_blocks(uint32_t n) {
        if (n < 1) throw PanicError("assertion failed: n >= 1");  // builder.rs:113 / :131
        nfb_ = n;
        return *this;
    }
    Result<BasicAhoCorasick<Flavor>> build(const std::vector<std::string> &patterns) const { return run(patterns, nullptr); }
    Result<BasicAhoCorasick<Flavor>> build_with_values(const std::vector<std::pair<std::string, uint32_t>> &patvals) const {
        std::vector<std::string> pats;
        std::vector<uint32_t> vals;
        for (const auto &pv : patvals) { pats.push_back(pv.first); vals.push_back(pv.second); }
        return run(pats, &vals);
    }

private:
    Result<BasicAhoCorasick<Flavor>> run(const std::vector<std::string> &pats, const std::vector<uint32_t> *vals) const {
        std::string blob;
        std::vector<uint64_t> offs{0};
        for (const auto &p : pats) { blob += p; offs.push_back(blob.size()); }
        daac_pma *h = nullptr;
        const daac_status st = Flavor::build(reinterpret_cast<const uint8_t *>(blob.data()), offs.data(), vals ? vals->data() : nullptr,
                                             pats.size(), static_cast<uint8_t>(kind_), nfb_, &h);
        if (st != DAAC_OK) return detail::make_error(st);
        return BasicAhoCorasick<Flavor>(h);
    }
    MatchKind kind_ = MatchKind::Standard;
    uint32_t nfb_ = 16;
};

using DoubleArrayAhoCorasick = BasicAhoCorasick<detail::Bytewise>;
using DoubleArrayAhoCorasickBuilder = BasicBuilder<detail::Bytewise>;
using CharwiseDoubleArrayAhoCorasick = BasicAhoCorasick<detail::Charwise>;
using CharwiseDoubleArrayAhoCorasickBuilder = BasicBuilder<detail::Charwise>;

// daac_tokens_pack over a batch of singles in device memory (template, truncation and padding: the header has the definition): the
// planes stay on the device and are the caller's, released with daac_device_free.  -> {row length, slots}
struct PackedPlanes {
    void *input_ids = nullptr, *token_type_ids = nullptr, *attention_mask = nullptr, *special_tokens_mask = nullptr;
    uint64_t *offsets = nullptr, *row_offsets = nullptr;
    uint64_t row_length = 0, slots = 0;
};
inline PackedPlanes tokens_pack(const daac_pack_params &params, const uint32_t *dev_ids, const uint64_t *dev_spans, const uint64_t *dev_offsets, uint64_t n_tokens,
                                size_t n, void *stream = nullptr) {
    PackedPlanes r;
    const daac_status st = daac_tokens_pack(&params, dev_ids, dev_spans, dev_offsets, n_tokens, nullptr, nullptr, nullptr, 0, n, stream, &r.input_ids, &r.token_type_ids,
                                            params.padding == DAAC_PAD_NONE ? nullptr : &r.attention_mask, &r.special_tokens_mask, dev_spans ? &r.offsets : nullptr,
                                            params.padding == DAAC_PAD_NONE ? &r.row_offsets : nullptr, &r.row_length, &r.slots);
    if (st != DAAC_OK) throw PanicError(std::string("tokens_pack failed: ") + daac_last_error());
    return r;
}

// daac_decoder: token ids back to text (the header has the definition).  The table is given as it is uploaded: the images' bytes in one
// pool, per id where its rest and first image lie, and a flag byte.  The text stays on the device and is the caller's, released with
// daac_device_free.
struct DecodedText {
    uint8_t *text = nullptr;
    uint64_t *offsets = nullptr, *token_starts = nullptr;
    uint64_t bytes = 0;
};
class Decoder {
public:
    Decoder(const std::string &pool, const std::vector<daac_decode_piece> &pieces, const std::vector<uint8_t> &flags) {
        if (pieces.size() != flags.size()) throw PanicError("Decoder: one flag byte per piece");
        const daac_status st = daac_decoder_create(reinterpret_cast<const uint8_t *>(pool.data()), pool.size(), pieces.data(), flags.data(), pieces.size(), &h_);
        if (st != DAAC_OK) throw PanicError(std::string("decoder_create failed: ") + daac_last_error());
    }
    ~Decoder() { daac_decoder_free(h_); }
    Decoder(const Decoder &) = delete;
    Decoder &operator=(const Decoder &) = delete;
    // a CSR token result in device memory: n_tokens u32 ids and n + 1 u64 token offsets
    DecodedText decode(const uint32_t *dev_ids, const uint64_t *dev_offsets, uint64_t n_tokens, size_t n, bool skip_special = true, bool unknown_skip = false,
                       bool token_starts = false, void *stream = nullptr) const {
        return run(dev_ids, 4, dev_offsets, n_tokens, n, 0, skip_special, unknown_skip, token_starts, stream);
    }
    // an [n, row_length] plane of id_width-byte ids (4 or 8) in device memory
    DecodedText decode_plane(const void *dev_ids, uint32_t id_width, size_t n, uint64_t row_length, bool skip_special = true, bool unknown_skip = false,
                             bool token_starts = false, void *stream = nullptr) const {
        return run(dev_ids, id_width, nullptr, 0, n, row_length, skip_special, unknown_skip, token_starts, stream);
    }

private:
    DecodedText run(const void *dev_ids, uint32_t id_width, const uint64_t *dev_offsets, uint64_t n_tokens, size_t n, uint64_t row_length, bool skip_special,
                    bool unknown_skip, bool token_starts, void *stream) const {
        DecodedText r;
        const daac_status st = daac_tokens_decode(h_, dev_ids, id_width, dev_offsets, n_tokens, n, row_length, skip_special, unknown_skip, stream, &r.text, &r.offsets,
                                                  token_starts ? &r.token_starts : nullptr, &r.bytes);
        if (st != DAAC_OK) throw PanicError(std::string("tokens_decode failed: ") + daac_last_error());
        return r;
    }
    daac_decoder *h_ = nullptr;
};

}  // namespace daachorse
