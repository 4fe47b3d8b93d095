// Launch wrappers of the Winograd layer kernel (kernels/conv_winograd_f32.h).  In the product build they are compiled in a translation
// unit of their own (aae_wino.hip, in parallel with the rest: the four phase bodies x two block geometries are a fifth of the library's
// compile time); the experiments build and the CPU emulator include this header into their single translation unit.
#pragma once

namespace aae_host {

#ifdef AAE_WINO_DECLARATIONS_ONLY
// (stage32: 32-channel stages where the layer allows them -- aae::wino_layer_stage_channels; static_halo: the zero halo written once per block
//  where the blocks cover whole sub-images -- aae::wino_layer_static_halo, from p.c.blocks_x / blocks_y; the same bits either way)
void wino_layer_launch(int geom, int wide, int stage32, unsigned grid, hipStream_t stream, const aae::ConvWinoLayerArgs& p, int static_halo = 1);
void wino_layer_multi_launch(int geom, int stage32, unsigned grid, hipStream_t stream, const aae::ConvWinoMultiArgs& p, int static_halo = 1);
void wino_set_attributes();
#else
#ifdef AAE_WINO_TU
#define AAE_WINO_LINKAGE
#else
#define AAE_WINO_LINKAGE static
#endif
// the instantiations of the 8-wave layer kernels: (geometry tag, stage channels, static halo) -- aae::wino_layer_geom_tag
#define AAE_WINO_FORMS(X) X(0, 16, false) X(0, 32, false) X(0, 16, true) X(0, 32, true) X(1, 16, true) X(1, 32, true) X(2, 16, false)
AAE_WINO_LINKAGE void wino_layer_launch(int geom, int wide, int stage32, unsigned grid, hipStream_t stream, const aae::ConvWinoLayerArgs& p, int static_halo = 1) {
#ifdef AAE_EXPERIMENTS
    if (wide) {      // blocks of 4 waves over both 32-channel halves: measured 13 % slower than two waves per SIMD (tools/ubench/wino_layer_time.hip)
        if (geom == 0) AAE_LAUNCH((aae::conv_wino_layer_kernel<0, true>), dim3(grid), dim3(256), aae::wino_layer_smem_bytes<0>(), stream, p);
        else AAE_LAUNCH((aae::conv_wino_layer_kernel<2, true>), dim3(grid), dim3(256), aae::wino_layer_smem_bytes<2>(), stream, p);
        return;
    }
#endif
    (void)wide;
    const bool st = aae::wino_layer_static_halo(geom, p.c.blocks_x, p.c.blocks_y, static_halo != 0);
    const int tag = aae::wino_layer_geom_tag(geom, st), sc = aae::wino_layer_stage_channels(geom, p.c.Cin, stage32 != 0, st);
#define AAE_WINO_X(G, SC, ST) \
    if (tag == G && sc == SC && st == ST) AAE_LAUNCH((aae::conv_wino_layer_kernel<G, false, SC, ST>), dim3(grid), dim3(512), (aae::wino_layer_smem_bytes<G, SC>()), stream, p);
    AAE_WINO_FORMS(AAE_WINO_X)
#undef AAE_WINO_X
}
AAE_WINO_LINKAGE void wino_layer_multi_launch(int geom, int stage32, unsigned grid, hipStream_t stream, const aae::ConvWinoMultiArgs& p, int static_halo = 1) {
    const bool st = aae::wino_layer_static_halo(geom, p.c.blocks_x, p.c.blocks_y, static_halo != 0);
    const int tag = aae::wino_layer_geom_tag(geom, st), sc = aae::wino_layer_stage_channels(geom, p.c.Cin, stage32 != 0, st);
#define AAE_WINO_X(G, SC, ST) \
    if (tag == G && sc == SC && st == ST) AAE_LAUNCH((aae::conv_wino_layer_multi_kernel<G, SC, ST>), dim3(grid), dim3(512), (aae::wino_layer_smem_bytes<G, SC>()), stream, p);
    AAE_WINO_FORMS(AAE_WINO_X)
#undef AAE_WINO_X
}
AAE_WINO_LINKAGE void wino_set_attributes() {
#define AAE_WINO_X(G, SC, ST) \
    (void)hipFuncSetAttribute((const void*)aae::conv_wino_layer_multi_kernel<G, SC, ST>, hipFuncAttributeMaxDynamicSharedMemorySize, aae::wino_layer_smem_bytes<G, SC>()); \
    (void)hipFuncSetAttribute((const void*)aae::conv_wino_layer_kernel<G, false, SC, ST>, hipFuncAttributeMaxDynamicSharedMemorySize, aae::wino_layer_smem_bytes<G, SC>());
    AAE_WINO_FORMS(AAE_WINO_X)
#undef AAE_WINO_X
#ifdef AAE_EXPERIMENTS
    (void)hipFuncSetAttribute((const void*)aae::conv_wino_layer_kernel<0, true>, hipFuncAttributeMaxDynamicSharedMemorySize, aae::wino_layer_smem_bytes<0>());
    (void)hipFuncSetAttribute((const void*)aae::conv_wino_layer_kernel<2, true>, hipFuncAttributeMaxDynamicSharedMemorySize, aae::wino_layer_smem_bytes<2>());
#endif
}
#endif

}  // namespace aae_host
