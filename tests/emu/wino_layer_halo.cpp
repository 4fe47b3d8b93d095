// Direct driver of the Winograd layer launch on the CPU fiber emulator (TEST INFRASTRUCTURE ONLY; see hip_emu.h), like wino_layer_direct.cpp,
// for BOTH block geometries and with the "winograd_static_halo" choice per call: 16 x 16-pixel regions (geom 0: 32 | H) and four 8 x 8-output
// images per block (geom 1: H = 16).  Built by tests/test_emu_winograd_static_halo.py with the compiler and flags of the Makefile here,
// together with hip_emu.cpp.
#include "hip_emu.h"

#include "../../augmentedautoencoder_amd/csrc/kernels/conv_winograd_f32.h"
#include "../../augmentedautoencoder_amd/csrc/aae_wino_launch.h"

namespace {
bool layer_geometry(aae::ConvWinoArgs& c, int geom, int H, int Cin, int Cout, int relu, int xcd_cols) {
    memset(&c, 0, sizeof(c));
    if (geom == 0 ? (H < 32 || H % 32 != 0) : H != 16) return false;
    c.H = c.W = H; c.Cin = Cin; c.Cout = Cout; c.Ho = c.Wo = H / 2; c.relu = relu;
    c.blocks_x = c.blocks_y = geom == 0 ? H / 32 : 1;
    c.xcd_cols = xcd_cols;
    return true;
}
int regions_of(const aae::ConvWinoArgs& c, int geom, int B) { return geom == 0 ? c.blocks_x * c.blocks_y * B : (B + 3) / 4; }
// what the launch ran as: 1000 * geometry tag + 100 * static halo + stage channels
int form_of(const aae::ConvWinoArgs& c, int geom, int stage32, int static_halo) {
    const bool st = aae::wino_layer_static_halo(geom, c.blocks_x, c.blocks_y, static_halo != 0);
    return 1000 * aae::wino_layer_geom_tag(geom, st) + 100 * (st ? 1 : 0) + aae::wino_layer_stage_channels(geom, c.Cin, stage32 != 0, st);
}
}  // namespace

// one 5 x 5 stride-2 'SAME' layer with square inputs of H x H pixels.  U4: the four components' packed weights, index 2 eh + ew.
extern "C" int wino_halo_layer(int geom, const float* x, const float* const* U4, const float* bias, float* out, int B, int H, int Cin, int Cout, int relu, int stage32,
                               int static_halo, int xcd_cols) {
    aae::ConvWinoLayerArgs p;
    memset(&p, 0, sizeof(p));
    if (!layer_geometry(p.c, geom, H, Cin, Cout, relu, xcd_cols)) return -1;
    p.c.x = x; p.c.bias = bias; p.c.out = out; p.c.B = B;
    p.c.regions = regions_of(p.c, geom, B);
    for (int i = 0; i < 4; ++i) p.U4[i] = U4[i];
    aae_host::wino_layer_launch(geom, 0, stage32, aae::wino_grid_blocks(p.c.regions, Cout / 64, xcd_cols), nullptr, p, static_halo);
    return form_of(p.c, geom, stage32, static_halo);
}

// the same layer shape over n objects in ONE launch: object o has B[o] images at x[o], weights U4[4 o ... 4 o + 3], bias[o], output out[o]
extern "C" int wino_halo_layer_multi(int geom, int n, const float* const* x, const float* const* U4, const float* const* bias, float* const* out, const int* B, int H,
                                     int Cin, int Cout, int relu, int stage32, int static_halo, int xcd_cols) {
    if (n < 1 || n > aae::kMultiMax) return -1;
    aae::ConvWinoMultiArgs m;
    memset(&m, 0, sizeof(m));
    if (!layer_geometry(m.c, geom, H, Cin, Cout, relu, xcd_cols)) return -1;
    m.range.n = n;
    int at = 0;
    for (int o = 0; o < n; ++o) {
        m.range.first[o] = at;
        at += regions_of(m.c, geom, B[o]);
        aae::ConvWinoObject& ob = m.obj[o];
        ob.x = x[o]; ob.out = out[o]; ob.bias = bias[o]; ob.bn_scale = nullptr; ob.bn_shift = nullptr; ob.B = B[o];
        for (int i = 0; i < 4; ++i) ob.U4[i] = U4[4 * o + i];
    }
    for (int o = n; o <= aae::kMultiMax; ++o) m.range.first[o] = at;
    m.c.regions = at;
    aae_host::wino_layer_multi_launch(geom, stage32, aae::wino_grid_blocks(at, Cout / 64, xcd_cols), nullptr, m, static_halo);
    return form_of(m.c, geom, stage32, static_halo);
}
