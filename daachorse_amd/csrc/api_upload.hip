// C ABI (include/daachorse_amd.h), part 1: handles — construction, serialisation, the upload of the re-packed automaton and of every
// engine's tables to a device, daac_pma_info / _explain / _trim.  No CPU scan fallback lives here.
#include "api_internal.hpp"

namespace daac {
namespace api {

// --------------------------------------------------------------------------------------- upload
// The tables themselves are the layout layer's (upload_layout.hpp): here the device, the options it reads and the hand-over to the handle.
daac_status upload_locked(daac_pma *pma, int device, DeviceTables **out) {
    auto it = pma->dev.find(device);
    if (it != pma->dev.end()) { *out = it->second.get(); return DAAC_OK; }
    int prev = 0;
    HIP_TRY(hipGetDevice(&prev));
    HIP_TRY(hipSetDevice(device));
    struct DeviceGuard {  // the caller's current device comes back on every return path, errors included
        int prev;
        ~DeviceGuard() { (void)hipSetDevice(prev); }
    } device_guard{prev};
    std::unique_ptr<DeviceTables> t(new DeviceTables);
    t->device = device;
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    t->num_cu = prop.multiProcessorCount;

    UploadOptions o;   // every option the layout depends on
    o.lds_budget = OPT(lds_budget); o.dense_depth = OPT(dense_depth); o.rows_share_pct = OPT(rows_share_pct);
    o.gram_lds_budget = OPT(gram_lds_budget); o.gram_rank_in_lds = OPT(gram_rank_in_lds);
    o.gram4_mph = OPT(gram4_mph); o.gram2_rfull = OPT(gram2_rfull); o.gram2_dpp = OPT(gram2_dpp);
    o.left3 = OPT(left3); o.pfx = OPT(pfx);
    o.char_map_lds = OPT(char_map_lds); o.char_row_lds = OPT(char_row_lds);
    // (*t twice: the EngineTables the layout fills, and the sink its arrays leave through)
    const daac_status st = pma->charwise ? layout::charwise_handle(pma->chost, o, *t, *t) : layout::bytewise_handle(pma->host, o, *t, *t);
    if (st != DAAC_OK) return st;
    HIP_TRY(hipDeviceSynchronize());
    *out = t.get();
    pma->dev[device] = std::move(t);
    return DAAC_OK;
}

daac_status get_tables(daac_pma *pma, DeviceTables **out) {
    int device = 0;
    HIP_TRY(hipGetDevice(&device));
    std::lock_guard<std::mutex> g(pma->mu);
    return upload_locked(pma, device, out);
}

}  // namespace api
}  // namespace daac

// ============================================================================== exported C ABI
extern "C" {

const char *daac_last_error(void) { return last_error_cstr(); }
int daac_last_engine(void) { return g_last_engine; }
const char *daac_last_kernel(void) { return g_last_kernel.c_str(); }
void daac_free(void *p) { std::free(p); }

daac_status daac_bytewise_from_serialized(const uint8_t *blob, size_t len, daac_pma **out, size_t *consumed) {
    if (!blob || !out) { set_error("null argument"); return DAAC_ERR_INVALID_ARGUMENT; }
    std::unique_ptr<daac_pma> p(new daac_pma);
    const daac_status st = HostPma::deserialize(blob, len, p->host, consumed);
    if (st != DAAC_OK) return st;
    *out = p.release();
    return DAAC_OK;
}

daac_status daac_bytewise_from_parts(const uint32_t *states, size_t n_states, const uint32_t *lstates, const uint32_t *fails,
                                     size_t n_lstates, const uint32_t *outputs, size_t n_outputs, uint8_t match_kind,
                                     uint32_t num_states, daac_pma **out) {
    if (!out || match_kind > 2) { set_error("bad argument"); return DAAC_ERR_INVALID_ARGUMENT; }
    if ((n_states && !states) || (n_lstates && (!lstates || !fails)) || (n_outputs && !outputs)) {
        set_error("null array with a non-zero count (`fails` must hold n_lstates entries)");
        return DAAC_ERR_INVALID_ARGUMENT;
    }
    std::unique_ptr<daac_pma> p(new daac_pma);
    HostPma &h = p->host;
    h.match_kind = match_kind;
    h.num_states = num_states;
    h.states.resize(n_states);
    if (n_states) std::memcpy(h.states.data(), states, n_states * sizeof(StateRec));
    h.lstates.resize(n_lstates);
    h.fails.resize(n_lstates);
    if (n_lstates) {
        std::memcpy(h.lstates.data(), lstates, n_lstates * sizeof(LStateRec));
        std::memcpy(h.fails.data(), fails, n_lstates * sizeof(uint32_t));
    }
    h.outputs.resize(n_outputs);
    if (n_outputs) std::memcpy(h.outputs.data(), outputs, n_outputs * sizeof(OutputRec));
    if (h.is_standard()) h.build_root_table();
    const daac_status st = h.validate();
    if (st != DAAC_OK) return st;
    *out = p.release();
    return DAAC_OK;
}

daac_status daac_bytewise_build(const uint8_t *blob, const uint64_t *offsets, const uint32_t *values, size_t n, uint8_t match_kind,
                                uint32_t num_free_blocks, daac_pma **out) {
    if (!out || (n && (!blob || !offsets))) { set_error("null argument"); return DAAC_ERR_INVALID_ARGUMENT; }
    try {
        std::unique_ptr<daac_pma> p(new daac_pma);
        const daac_status st = build_bytewise(blob, offsets, values, n, match_kind, num_free_blocks, p->host);
        if (st != DAAC_OK) return st;
        *out = p.release();
        return DAAC_OK;
    } catch (const std::bad_alloc &) {
        set_error("out of memory while building the automaton");
        return DAAC_ERR_AUTOMATON_SCALE;
    }
}

daac_status daac_charwise_from_serialized(const uint8_t *blob, size_t len, daac_pma **out, size_t *consumed) {
    if (!blob || !out) { set_error("null argument"); return DAAC_ERR_INVALID_ARGUMENT; }
    std::unique_ptr<daac_pma> p(new daac_pma);
    p->charwise = true;
    const daac_status st = HostCharPma::deserialize(blob, len, p->chost, consumed);
    if (st != DAAC_OK) return st;
    *out = p.release();
    return DAAC_OK;
}

daac_status daac_charwise_build(const uint8_t *blob, const uint64_t *offsets, const uint32_t *values, size_t n, uint8_t match_kind,
                                uint32_t num_free_blocks, daac_pma **out) {
    if (!out || (n && (!blob || !offsets))) { set_error("null argument"); return DAAC_ERR_INVALID_ARGUMENT; }
    try {
        std::unique_ptr<daac_pma> p(new daac_pma);
        p->charwise = true;
        const daac_status st = build_charwise(blob, offsets, values, n, match_kind, num_free_blocks, p->chost);
        if (st != DAAC_OK) return st;
        *out = p.release();
        return DAAC_OK;
    } catch (const std::bad_alloc &) {
        set_error("out of memory while building the automaton");
        return DAAC_ERR_AUTOMATON_SCALE;
    }
}

daac_status daac_pma_serialize(const daac_pma *pma, uint8_t **buf, size_t *len) {
    if (!pma || !buf || !len) { set_error("null argument"); return DAAC_ERR_INVALID_ARGUMENT; }
    std::vector<uint8_t> v;
    if (pma->charwise) pma->chost.serialize(v); else pma->host.serialize(v);
    uint8_t *b = static_cast<uint8_t *>(std::malloc(v.size() ? v.size() : 1));
    if (!b) { set_error("out of memory"); return DAAC_ERR_AUTOMATON_SCALE; }
    std::memcpy(b, v.data(), v.size());
    *buf = b;
    *len = v.size();
    return DAAC_OK;
}

uint32_t daac_abi_version(void) { return DAAC_ABI_VERSION; }

// the engine plan of a handle: what scan_count_impl / scan_range_device / make_plan decide for engine AUTO, said up front
static void fill_plan(const daac_pma *pma, const DeviceTables *t, daac_info &f) {
    auto set = [&](int req, int engine, int kernel, int why) {
        f.plan_engine[req] = static_cast<uint8_t>(engine); f.plan_kernel[req] = static_cast<uint8_t>(kernel); f.plan_reason[req] = static_cast<uint8_t>(why);
    };
    for (int r = 0; r < DAAC_REQ_N; ++r) set(r, DAAC_ENGINE_AUTO, DAAC_KERNEL_NONE, t ? DAAC_WHY_FASTEST : DAAC_WHY_NOT_UPLOADED);
    if (!t) return;   // (a charwise handle has no table set beside its double array)
    const bool standard = pma->is_standard();
    // the restart iterator of the handle's kind: find3 / left3, else the chain walkers over the double array (bytewise, "" in the set: the sync-point scanners)
    const int find_req = standard ? DAAC_REQ_FIND : DAAC_REQ_LEFTMOST_FIND;
    if (select_ready(pma, t, !standard) && select_text_ok(t, !standard)) set(find_req, DAAC_ENGINE_GRAM, DAAC_KERNEL_SELECT, DAAC_WHY_FASTEST);
    else set(find_req, DAAC_ENGINE_DARRAY, !pma->charwise && pma->root_has_output() ? DAAC_KERNEL_SEGMENT : DAAC_KERNEL_CHAIN, DAAC_WHY_CHAIN);
    if (!standard) return;
    // why the byte-class tables were declined, as far as it is known
    const int why_no_gram = pma->charwise ? DAAC_WHY_CHARWISE : pma->root_has_output() ? DAAC_WHY_EMPTY_PATTERN
                            : t->n_distinct_bytes > 61 ? DAAC_WHY_ALPHABET : t->n_distinct_bytes != 0 ? DAAC_WHY_LDS : DAAC_WHY_TRIE_SHAPE;
    // count / count + checksum: what scan_count_impl will run (the same resolver)
    for (const bool cs : {false, true}) {
        const CountPlan cp = resolve_count(pma, t, DAAC_FIND_OVERLAPPING, DAAC_ENGINE_AUTO, cs, 0);
        const std::pair<int, int> ids = count_ids(t, cp);   // (GRAM tables there, their checksum half without room: LDS)
        set(cs ? DAAC_REQ_OVERLAPPING_CHECKSUM : DAAC_REQ_OVERLAPPING_COUNT, ids.first, ids.second,
            ids.first == DAAC_ENGINE_GRAM ? DAAC_WHY_FASTEST : (cs && (t->gram2_ok || t->gramw_ok)) ? DAAC_WHY_LDS : why_no_gram);
    }
    const int seg_engine = t->tier_ok ? DAAC_ENGINE_TIERED : DAAC_ENGINE_DARRAY;
    if (emit3_ready(t, false) && emit3_text_ok(t)) set(DAAC_REQ_OVERLAPPING_TUPLES, DAAC_ENGINE_GRAM, DAAC_KERNEL_GRAM_EMIT, DAAC_WHY_FASTEST);
    else if (emit3_ready(t, true) && emit3_text_ok(t)) set(DAAC_REQ_OVERLAPPING_TUPLES, DAAC_ENGINE_PFX, DAAC_KERNEL_PFX, why_no_gram);
    else set(DAAC_REQ_OVERLAPPING_TUPLES, seg_engine, DAAC_KERNEL_SEGMENT, t->gram2_ok ? DAAC_WHY_DUPLICATES : why_no_gram);
    set(DAAC_REQ_NO_SUFFIX, seg_engine, DAAC_KERNEL_SEGMENT, pma->charwise ? DAAC_WHY_CHARWISE : DAAC_WHY_FASTEST);
}

daac_status daac_pma_info(const daac_pma *pma, daac_info *info) {
    PmaScope scope_(pma);
    if (!pma || !info) { set_error("null argument"); return DAAC_ERR_INVALID_ARGUMENT; }
    const uint32_t cap = info->struct_size;
    if (cap < 8 || cap > (1u << 16)) {
        set_error("daac_info.struct_size must hold sizeof(daac_info) of the caller (ABI version " + std::to_string(DAAC_ABI_VERSION) + ")");
        return DAAC_ERR_INVALID_ARGUMENT;
    }
    daac_info full;
    daac_info *f = &full;
    std::memset(f, 0, sizeof(*f));
    f->struct_size = static_cast<uint32_t>(sizeof(daac_info));
    if (pma->charwise) {
        const HostCharPma &c = pma->chost;
        f->match_kind = c.match_kind;
        f->num_states = c.num_states;
        f->states_len = c.states.size();
        f->outputs_len = c.outputs.size();
        f->heap_bytes = c.heap_bytes();
        f->max_pattern_len = c.max_pattern_len();
        f->charwise = 1;
        f->alphabet_size = c.alphabet_size;
    } else {
        const HostPma &h = pma->host;
        f->match_kind = h.match_kind;
        f->num_states = h.num_states;
        f->states_len = h.states_len();
        f->outputs_len = h.outputs.size();
        f->heap_bytes = h.heap_bytes();
        f->max_pattern_len = h.max_pattern_len();
    }
    {
        std::lock_guard<std::mutex> g(const_cast<daac_pma *>(pma)->mu);
        const DeviceTables *t = pma->dev.empty() ? nullptr : pma->dev.begin()->second.get();
        if (t && !pma->charwise) {
            f->tiered_available = t->tier_ok;
            if (t->tier_ok) {
                f->num_classes = t->tier.C;
                f->tier_dense_states = t->tier.NA;
                f->tier_lds_states = t->tier.NB;
                f->tier_lds_bytes = t->tier.off_cls + 256u;   // (the tables alone: a launch asks for at least 1 KiB, for its reduction scratch)
            }
            f->gram_available = t->gram_ok || t->gram2_ok;
            if (t->gram_ok) {
                f->gram_k = t->gram.K;
                f->gram_lds_bytes = t->gram.lds_bytes;
            }
            if (t->gramw_ok) { f->gram_available = 1; f->gram_k = 2; f->gram_lds_bytes = t->gramw.lds_count; f->num_classes = t->gramw.C; f->gram_wide = 1; }
            f->gram2_available = t->gram2_ok;
            if (t->gram2_ok) {
                f->gram2_k = t->gram2.K;
                f->gram2_exact = t->gram2.exact_ok;
                f->gram2_lds_count = t->gram2.lds_count;
                f->gram2_lds_exact = t->gram2.lds_exact;
                if (!t->gram_ok) { f->gram_k = t->gram2.K; f->gram_lds_bytes = t->gram2.lds_count; }
            }
            f->pfx_available = t->pfx_ok;
            if (t->pfx_ok) { f->pfx_key_bytes = t->pfx.G; f->pfx_lds_bytes = t->pfx.lds_bytes; }
        }
        fill_plan(pma, t, *f);
    }
    std::memcpy(info, f, std::min<size_t>(cap, sizeof(daac_info)));
    info->struct_size = static_cast<uint32_t>(std::min<size_t>(cap, sizeof(daac_info)));
    return DAAC_OK;
}

size_t daac_pma_explain(const daac_pma *pma, char *buf, size_t cap) {
    if (!pma) return 0;
    daac_info f;
    f.struct_size = static_cast<uint32_t>(sizeof(f));
    if (daac_pma_info(pma, &f) != DAAC_OK) return 0;
    static const char *req[] = {"find_overlapping_iter(h).count()", "find_overlapping count + checksum", "find_overlapping tuples", "find_iter",
                                "leftmost_find_iter", "find_overlapping_no_suffix_iter"};
    static const char *eng[] = {"auto", "tiered", "darray", "gram", "pfx"};
    static const char *ker[] = {"- (the crate panics: wrong MatchKind)", "gram4 count kernel (one LDS lookup per byte)", "gram count + checksum kernel",
                                "gram wide-alphabet kernel (31-62 byte classes)", "gram tuple emitter", "pfx (hashed prefix filter + start-anchored walks, any alphabet)",
                                "segment scanners (one lane per segment)", "micro-step walker over the double array", "chain walkers (speculate / reconcile / emit)",
                                "selection over the tuple emitter's detection (find3 / left3: no state chain)"};
    static const char *why[] = {"", "not uploaded yet", "more distinct pattern bytes than the byte-class tables take", "tables do not fit the LDS",
                                "\"\" is a pattern", "duplicate patterns the tables cannot encode", "the iterator is a chain through its own matches",
                                "charwise automaton", "trie shape / table limits"};
    std::string s;
    for (int r = 0; r < DAAC_REQ_N; ++r) {
        s += req[r];
        s += ": ";
        if (f.plan_reason[r] == DAAC_WHY_NOT_UPLOADED) { s += "not uploaded yet (daac_pma_upload decides the plan)\n"; continue; }
        if (f.plan_kernel[r] == DAAC_KERNEL_NONE) { s += ker[0]; s += "\n"; continue; }
        s += "engine "; s += eng[f.plan_engine[r] < sizeof(eng) / sizeof(*eng) ? f.plan_engine[r] : 0];
        s += ", "; s += ker[f.plan_kernel[r] < sizeof(ker) / sizeof(*ker) ? f.plan_kernel[r] : 0];
        if (f.plan_reason[r] != DAAC_WHY_FASTEST) { s += "  [not the fastest family: "; s += why[f.plan_reason[r] < sizeof(why) / sizeof(*why) ? f.plan_reason[r] : 0]; s += "]"; }
        s += "\n";
    }
    if (buf && cap) {
        const size_t n = std::min(cap - 1, s.size());
        std::memcpy(buf, s.data(), n);
        buf[n] = 0;
    }
    return s.size() + 1;
}

// Gives back what the handle keeps between calls beside its tables: the emitter's / selection kernels' workspace on every device it was
// uploaded to (option workspace_keep bounds it while it is kept).  A workspace a scan is using right now stays.
daac_status daac_pma_trim(daac_pma *pma) {
    if (!pma) { set_error("null argument"); return DAAC_ERR_INVALID_ARGUMENT; }
    std::lock_guard<std::mutex> g(pma->mu);
    int prev = 0;
    const bool have_prev = hipGetDevice(&prev) == hipSuccess;
    for (auto &kv : pma->dev) {
        DeviceTables *t = kv.second.get();
        if (!t || t->ws_busy.exchange(true)) continue;
        if (t->ws_p && hipSetDevice(kv.first) == hipSuccess) { (void)hipFree(t->ws_p); t->ws_p = nullptr; t->ws_bytes = 0; }
        t->ws_want.store(0);
        t->ws_busy.store(false);
    }
    if (have_prev) (void)hipSetDevice(prev);
    return DAAC_OK;
}

void daac_pma_free(daac_pma *pma) { delete pma; }

daac_status daac_pma_upload(daac_pma *pma, int device) {
    PmaScope scope_(pma);
    if (!pma) { set_error("null argument"); return DAAC_ERR_INVALID_ARGUMENT; }
    std::lock_guard<std::mutex> g(pma->mu);
    DeviceTables *t = nullptr;
    return upload_locked(pma, device, &t);
}

}  // extern "C"
