// Records tests/golden/option_rules.json: what aae_encoder_set_option and aae_codebook_set_scan_mode answered, and stored, in the
// commit BEFORE the option and scan-mode tables of csrc/aae_options.h existed (47d26f01c60db62700ad28d3a561405a636be0be: the strcmp
// ladder and the nested ternaries of aae_abi_impl.h).  It includes that commit's host sources through the CPU emulator, the way
// tests/emu/aae_emu_lib.cpp does, calls the real entry points and reads the handles' fields.  From the root of a checkout of that
// commit, with this file copied in:
//
//   clang++ -DAAE_EXPERIMENTS -O1 -std=c++17 -ffp-contract=off -Wno-pass-failed -Wno-psabi tests/golden/make_option_rules.cpp tests/emu/hip_emu.cpp -o rules_experiments
//   clang++                   -O1 -std=c++17 -ffp-contract=off -Wno-pass-failed -Wno-psabi tests/golden/make_option_rules.cpp tests/emu/hip_emu.cpp -o rules_product
//   (echo '{"parent": "47d26f01c60db62700ad28d3a561405a636be0be",'; ./rules_experiments; echo ','; ./rules_product; echo '}') > tests/golden/option_rules.json
//
// Every probe starts from the defaults: the option fields of ONE default-config encoder (128 x 128 x 3, filters 128 256 512 512,
// 5 x 5 stride 2, latent 128) are put back to their values after creation in front of each call.  Probe values per option:
// INT_MIN, -1, 0, 1, 2, INT_MAX, the default and its two neighbours, and every bound or allowed value of the rule with its two
// neighbours.  "stored" is the option's field after the call (null for "wavek_timeline", whose state is a buffer pointer).
#include <limits.h>

#include <set>

#include "../emu/hip_emu.h"

#include "../../augmentedautoencoder_amd/csrc/aae_hip_impl.h"

namespace {

struct Probe {
    const char* name;
    int aae_encoder::*field;
    std::vector<int> bounds;      // of the rule in aae_encoder_set_option
};

#define O(name, ...) {#name, &aae_encoder::name, {__VA_ARGS__}}
const Probe kOptions[] = {
    O(splitk_min_base_blocks), O(splitk_target_blocks), O(reduce_small), O(igemm_stagger), O(x3h_dma), O(x3h_wide256), O(x3h_min_tiles, 0),
    O(x3h_wide256_min_blocks, 1), O(x3h_wide_min_blocks, 0), O(igemm_dma), O(igemm_breg), O(dense_gemv), O(dense_gemv_max_batch), O(wavek_tail_split),
    O(planner_cost_min_batch, 1), O(planner_cost_batch3), O(wavek_eff64x32_pct, 30, 100), O(wavek_g_boost, 1, 4), O(wavek_force_tail_tiles, 0),
    O(wavek_force_tail_g, 2), O(gemv_ticket), O(wavek), O(wavek_dense), O(wavek_ablate), O(wavek_balance), O(planner_cost_model), O(ticket_prep),
    O(multi_group_plan), O(multi_xcd_affine), O(multi_force_depth), O(multi_force_shape), O(multi_force_g), O(detect_chain),
    O(detect_chain_blocks, 1, 1024), O(compact_workspace), O(chain_timeline, 0), {"wavek_timeline", nullptr, {}}, O(wavek_max_tiles, 0, 8192),
    O(wavek_narrow_max_tiles, 0), O(wavek_target_blocks, 0, 512), O(wavek_tiny_max_tiles, 0), O(wavek_waves, 4, 8), O(wavek_pingpong), O(wavek_spread, 0, 3),
    O(wavek_tiny_waves, 4, 8), O(wavek_depth, 2, 3), O(igemm_breg_wide), O(igemm_breg_wide_min_blocks), O(igemm_breg_min_blocks), O(first_vec4),
    O(first_group_split_max_tiles, 0), O(first_target_blocks, 1), O(first_max_tiles_per_block, 1), O(x3h_act_shift, -8, 12), O(winograd, 0, 2),
    O(winograd_wide), O(winograd_stage32), O(winograd_static_halo), O(winograd_min_batch, 1), O(winograd_min_fill_pct, 1, 100), O(winograd_min_blocks, 0),
    O(multi_mid_group), O(multi_split_items), O(multi_group_winograd), O(multi_mid_scan), O(multi_mid_ragged), O(winograd_xcd_cols, -1, 8), O(precision, 0, 2),
};
#undef O

aae_encoder* default_encoder() {
    aae_encoder_desc d = {};
    d.in_h = d.in_w = 128; d.in_c = 3; d.num_layers = 4; d.kernel_size = 5; d.latent_size = 128;
    const int filters[4] = {128, 256, 512, 512};
    for (int i = 0; i < 4; ++i) { d.num_filters[i] = filters[i]; d.strides[i] = 2; }
    std::vector<float> w((size_t)25 * 512 * 512);
    unsigned s = 1;
    for (float& v : w) { s = s * 1664525u + 1013904223u; v = ((int)(s >> 16) - 32768) * 1e-6f; }
    const void* hw[10];
    for (const void*& p : hw) p = w.data();
    aae_encoder* enc = nullptr;
    if (aae_encoder_create(&d, hw, 10, &enc) != AAE_OK) { fprintf(stderr, "aae_encoder_create: %s\n", aae_last_error()); exit(1); }
    return enc;
}

void print_settings(const aae_codebook* cb) {
    printf("[%d, %d, %d, %d, %d, %d, %d, %d]", cb->scan_mode, cb->scan_ticket, cb->topk_prune, cb->scan_walk, cb->scan_fused_norm, cb->scan_rh4,
           cb->scan_resident_fin, cb->scan_topk_stream);
}

}  // namespace

int main() {
#ifdef AAE_EXPERIMENTS
    printf("\"experiments\": {\n");
#else
    printf("\"product\": {\n");
#endif
    aae_encoder* enc = default_encoder();
    const size_t n = sizeof(kOptions) / sizeof(kOptions[0]);
    std::vector<int> defaults(n, 0);
    for (size_t i = 0; i < n; ++i)
        if (kOptions[i].field) defaults[i] = enc->*kOptions[i].field;
    printf(" \"options\": {\n");
    for (size_t i = 0; i < n; ++i) {
        const Probe& o = kOptions[i];
        std::set<long long> values = {INT_MIN, -1, 0, 1, 2, INT_MAX};
        std::vector<int> marks = o.bounds;
        marks.push_back(defaults[i]);
        for (int b : marks)
            for (long long v = (long long)b - 1; v <= (long long)b + 1; ++v)
                if (v >= INT_MIN && v <= INT_MAX) values.insert(v);
        printf("  \"%s\": {\"default\": ", o.name);
        if (o.field) printf("%d", defaults[i]); else printf("null");
        printf(", \"probes\": [");
        bool first = true;
        for (long long v : values) {
            for (size_t k = 0; k < n; ++k)
                if (kOptions[k].field) enc->*kOptions[k].field = defaults[k];
            enc->wavek_timeline = nullptr;          // (a buffer made for an earlier probe stays with the handle's allocations)
            const int rc = aae_encoder_set_option(enc, o.name, (int)v);
            printf("%s[%lld, %d, ", first ? "" : ", ", v, rc);
            if (o.field) printf("%d]", enc->*o.field); else printf("null]");
            first = false;
        }
        printf("]}%s\n", i + 1 < n ? "," : "");
    }
    printf(" },\n \"unknown\": [");
    const char* unknown[3] = {"", "wavek_", "no_such_option"};
    for (int i = 0; i < 3; ++i) printf("%s[\"%s\", %d]", i ? ", " : "", unknown[i], aae_encoder_set_option(enc, unknown[i], 1));
    printf("],\n");
    aae_encoder_destroy(enc);

    // scan modes: a fresh codebook per mode, one upright copy (every 2nd row) prepared before the call and one (every 3rd row) after it
    printf(" \"scan_modes\": [\n");
    const std::vector<float> E((size_t)64 * 128, 0.5f);
    for (int mode = -1; mode <= 12; ++mode) {
        aae_codebook* cb = nullptr;
        if (aae_codebook_create(E.data(), 64, 128, AAE_DTYPE_F32, 0, &cb) != AAE_OK || aae_codebook_prepare_upright(cb, 2, nullptr) != AAE_OK) return 1;
        const int rc = aae_codebook_set_scan_mode(cb, mode);
        if (aae_codebook_prepare_upright(cb, 3, nullptr) != AAE_OK || cb->upright_copies.size() != 2) return 1;
        printf("  {\"mode\": %d, \"rc\": %d, \"fields\": ", mode, rc);
        print_settings(cb);
        printf(", \"upright_before\": ");
        print_settings(cb->upright_copies[0].second);
        printf(", \"upright_after\": ");
        print_settings(cb->upright_copies[1].second);
        printf("}%s\n", mode < 12 ? "," : "");
        aae_codebook_destroy(cb);
    }
    printf(" ]\n}\n");
    return 0;
}
