// CPU-emulated build of the libaae_hip host+kernel sources (TEST INFRASTRUCTURE ONLY;
// see hip_emu.h).  Exports the same C ABI operating on host pointers.
#include "hip_emu.h"

#include "../../augmentedautoencoder_amd/csrc/aae_hip_impl.h"

// (tests/test_options.py) the eight ScanSettings fields of a codebook handle (col_stride <= 1) or of its upright copy for col_stride
extern "C" int aae_emu_codebook_scan_settings(const aae_codebook* cb, int col_stride, int* out8) {
    const aae_host::ScanSettings* s = col_stride <= 1 ? cb : nullptr;
    for (const auto& c : cb->upright_copies)
        if (c.first == col_stride) s = c.second;
    if (!s) return AAE_ERR_INVALID;
    const int v[8] = {s->scan_mode, s->scan_ticket, s->topk_prune, s->scan_walk, s->scan_fused_norm, s->scan_rh4, s->scan_resident_fin, s->scan_topk_stream};
    memcpy(out8, v, sizeof(v));
    return AAE_OK;
}

// (tests/test_multi_plans.py, tests/golden/make_multi_plans.cpp) what the grouped query's planner decides for a frame, as one JSON object: per distinct
// encoder handle (in the order of `items`) whether layers[li].wino[0] is set; with_plan: the item list after expand_items and every field of its MultiPlan that
// a launch depends on.  Plans the way multi_impl does (prepares nothing).  Returns the text's length; writes it, 0-terminated, where it fits into `cap` bytes.
extern "C" size_t aae_emu_multi_plan_dump(const aae_multi_item* items_in, int n_items_in, int scan_only, int with_plan, char* out, size_t cap) {
    using namespace aae_host;
    std::string s;
    auto put = [&s](const char* fmt, auto... v) { char b[512]; snprintf(b, sizeof(b), fmt, v...); s += b; };
    auto list = [&](const char* name, const auto& v, auto&& one) {
        put("\"%s\": [", name);
        for (size_t k = 0; k < v.size(); ++k) { if (k) s += ", "; one(v[k]); }
        s += "]";
    };
    auto ints = [&](const auto& v) { s += "["; for (size_t k = 0; k < v.size(); ++k) put(k ? ", %d" : "%d", (int)v[k]); s += "]"; };
    auto wavek = [&](const WaveKPlan& w) {
        if (!w.use) { s += "null"; return; }
        put("[%d, %d, %d, %d, %d, %zu]", wavek_shape_key(w), w.gsplits, w.num_mt, w.num_nt, w.tail_tiles, w.partial_bytes);
    };
    std::vector<const aae_encoder*> encs;
    auto enc_id = [&encs](const aae_encoder* e) { return e ? (int)(std::find(encs.begin(), encs.end(), e) - encs.begin()) : -1; };
    for (int i = 0; i < n_items_in; ++i)
        if (items_in[i].enc && enc_id(items_in[i].enc) == (int)encs.size()) encs.push_back(items_in[i].enc);
    s += "{";
    list("prepared", encs, [&](const aae_encoder* e) {
        s += "[";
        for (size_t li = 0; li < e->layers.size(); ++li) put(li ? ", %d" : "%d", e->layers[li].wino[0] ? 1 : 0);
        s += "]";
    });
    if (with_plan) {
        std::vector<aae_multi_item> expanded;
        const bool split = expand_items(items_in, n_items_in, scan_only != 0, expanded);
        const aae_multi_item* items = split ? expanded.data() : items_in;
        const int n_items = split ? (int)expanded.size() : n_items_in;
        MultiPlan mp;
        const int rc = plan_multi(items, n_items, scan_only != 0, mp);
        put(", \"split\": %d, \"rc\": %d, ", split ? 1 : 0, rc);
        int at = 0;
        list("items", mp.items, [&](const MultiItemPlan& p) {
            const aae_multi_item& it = items[at++];
            put("{\"enc\": %d, \"n\": %d, \"col_stride\": %d, \"grouped\": %d, \"mid\": %d, \"row0\": %d, \"enc_off\": %zu, \"enc_bytes\": %zu, \"cb_off\": %zu, \"cb_bytes\": %zu, ",
                enc_id(it.enc), it.n, it.col_stride, (int)p.grouped, (int)p.mid, p.row0, p.enc_off, p.enc_bytes, p.cb_off, p.cb_bytes);
            list("plans", p.plans, wavek);
            s += ", ";
            list("rem_plans", p.rem_plans, wavek);
            s += "}";
        });
        s += ", "; list("groups", mp.groups, ints);
        s += ", "; list("mid_groups", mp.mid_groups, ints);
        s += ", "; list("group_wino", mp.group_wino, ints);
        s += ", "; list("mid_wino", mp.mid_wino, ints);
        s += ", "; list("mid_rem", mp.mid_rem, ints);
        put(", \"seq\": [%zu, %zu, %zu, %zu], \"total\": %zu", mp.seq_enc_off, mp.seq_enc_bytes, mp.seq_cb_off, mp.seq_cb_bytes, mp.total);
    }
    s += "}";
    if (out && s.size() < cap) memcpy(out, s.c_str(), s.size() + 1);
    return s.size();
}
