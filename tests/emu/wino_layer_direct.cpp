// Direct driver of the Winograd layer launch on the CPU fiber emulator (TEST INFRASTRUCTURE ONLY; see hip_emu.h): the launch wrappers of
// csrc/aae_wino_launch.h on caller-supplied activations and Winograd-domain weights, without an encoder around them -- for layer
// widths no EncoderConfig reaches (the planner gives the Winograd form to layers with 32 | Cin only) and for choosing the stage size per call.
// Built by tests/test_emu_winograd_stages32.py with the compiler and flags of the Makefile here, together with hip_emu.cpp.
#include "hip_emu.h"

#include "../../augmentedautoencoder_amd/csrc/kernels/conv_winograd_f32.h"
#include "../../augmentedautoencoder_amd/csrc/aae_wino_launch.h"

namespace {
void layer_geometry(aae::ConvWinoArgs& c, int H, int Cin, int Cout, int relu, int xcd_cols) {
    memset(&c, 0, sizeof(c));
    c.H = c.W = H; c.Cin = Cin; c.Cout = Cout; c.Ho = c.Wo = H / 2; c.relu = relu;
    c.blocks_x = c.blocks_y = H / 32;
    c.xcd_cols = xcd_cols;
}
}  // namespace

// one 5 x 5 stride-2 'SAME' layer with square inputs of H x H pixels, 32 | H (16 x 16-pixel output regions: block geometry 0).
// U4: the four components' packed weights, index 2 eh + ew.  Returns the stage channels the launch ran with.
extern "C" int wino_direct_layer(const float* x, const float* const* U4, const float* bias, float* out, int B, int H, int Cin, int Cout, int relu, int stage32,
                                 int xcd_cols) {
    aae::ConvWinoLayerArgs p;
    memset(&p, 0, sizeof(p));
    layer_geometry(p.c, H, Cin, Cout, relu, xcd_cols);
    p.c.x = x; p.c.bias = bias; p.c.out = out; p.c.B = B;
    p.c.regions = p.c.blocks_x * p.c.blocks_y * B;
    for (int i = 0; i < 4; ++i) p.U4[i] = U4[i];
    aae_host::wino_layer_launch(0, 0, stage32, aae::wino_grid_blocks(p.c.regions, Cout / 64, xcd_cols), nullptr, p);
    return aae::wino_layer_stage_channels(0, Cin, stage32 != 0);
}

// the same layer shape over n objects in ONE launch: object o has B[o] images at x[o], weights U4[4 o ... 4 o + 3], bias[o], output out[o]
extern "C" int wino_direct_layer_multi(int n, const float* const* x, const float* const* U4, const float* const* bias, float* const* out, const int* B, int H, int Cin,
                                       int Cout, int relu, int stage32, int xcd_cols) {
    if (n < 1 || n > aae::kMultiMax) return -1;
    aae::ConvWinoMultiArgs m;
    memset(&m, 0, sizeof(m));
    layer_geometry(m.c, H, Cin, Cout, relu, xcd_cols);
    m.range.n = n;
    int at = 0;
    for (int o = 0; o < n; ++o) {
        m.range.first[o] = at;
        at += m.c.blocks_x * m.c.blocks_y * B[o];
        aae::ConvWinoObject& ob = m.obj[o];
        ob.x = x[o]; ob.out = out[o]; ob.bias = bias[o]; ob.bn_scale = nullptr; ob.bn_shift = nullptr; ob.B = B[o];
        for (int i = 0; i < 4; ++i) ob.U4[i] = U4[4 * o + i];
    }
    for (int o = n; o <= aae::kMultiMax; ++o) m.range.first[o] = at;
    m.c.regions = at;
    aae_host::wino_layer_multi_launch(0, stage32, aae::wino_grid_blocks(at, Cout / 64, xcd_cols), nullptr, m);
    return aae::wino_layer_stage_channels(0, Cin, stage32 != 0);
}
