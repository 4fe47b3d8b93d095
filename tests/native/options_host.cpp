// Stand-alone driver of csrc/aae_options.h (no HIP, no emulator): tests/test_options.py compiles it with and without
// -DAAE_EXPERIMENTS and compares its answers with tests/golden/option_rules.json.
//   options_host --list                 the option names, one per line
//   options_host --scan                 for the modes -1 ... 12: "mode rc" and the eight ScanSettings fields after the call
//   options_host                        reads "name value" lines; answers "rc stored default" per line, every call on fresh
//                                       defaults ("-" where the option has no field or the name is unknown)
#include <stdio.h>

#include "../../augmentedautoencoder_amd/csrc/aae_options.h"

using namespace aae_host;

int main(int argc, char** argv) {
    char err[256];
    if (argc > 1 && !strcmp(argv[1], "--list")) {
        for (const OptionRow& r : kOptionTable) printf("%s\n", r.name);
        return 0;
    }
    if (argc > 1 && !strcmp(argv[1], "--scan")) {
        for (int mode = -1; mode <= 12; ++mode) {
            ScanSettings s;
            const int rc = apply_scan_mode(s, mode, err, sizeof(err));
            printf("%d %d %d %d %d %d %d %d %d %d\n", mode, rc, s.scan_mode, s.scan_ticket, s.topk_prune, s.scan_walk, s.scan_fused_norm, s.scan_rh4,
                   s.scan_resident_fin, s.scan_topk_stream);
        }
        return 0;
    }
    char name[128];
    int value = 0;
    for (;;) {
        name[0] = 0;                                             // (a line "  7": the empty name)
        char line[256];
        if (!fgets(line, sizeof(line), stdin)) break;
        if (sscanf(line, " %d", &value) != 1 && sscanf(line, "%127s %d", name, &value) != 2) return 2;
        EncoderOptions o;
        err[0] = 0;
        const int rc = apply_option(o, name, value, err, sizeof(err));
        if (rc != AAE_OK && (!strstr(err, name) || !err[0])) return 3;      // an error text names the option
        const int EncoderOptions::*field = nullptr;
        for (const OptionRow& r : kOptionTable)
            if (!strcmp(name, r.name)) field = r.field;
        if (field) printf("%d %d %d\n", rc, o.*field, EncoderOptions{}.*field);
        else printf("%d - -\n", rc);
    }
    return 0;
}
