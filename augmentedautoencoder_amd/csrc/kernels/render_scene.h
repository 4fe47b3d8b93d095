// Several meshes into one frame (gfx950): the draws of a call, each (mesh of a set, R, t, scene), rasterised into the key buffer
// of their scene in six launches, no host synchronisation between them.  The scene rule (key = fp32 bits of z << 32 |
// draw * Fmax + triangle, the per-draw box) is stated in render_core.h; per-draw geometry is the single-mesh path's, through the
// helpers of render_raster.h.
//
//   scene_init      per scene: empty screen rectangle (the workspace may arrive full of garbage)
//   scene_vertex    per (draw, vertex): snapped xy, float64 z, varyings into the draw's slot; the SCENE's rectangle by one
//                   filtered integer min / max atomic per block and word
//   scene_clear     visibility keys of each scene's rectangle := background
//   scene_raster    per (draw, triangle): as render_raster; every thread keeps the extremes of the pixels its fragments fell
//                   on, the block reduces them and stores its partial bounds with plain stores: no atomic for the boxes
//   scene_bbox      per draw: the partial bounds of its blocks -> calc_2d_bbox, the visible flag
//   scene_frame     per (scene, pixel): the key decoded into (draw, triangle), that fragment shaded from the draw's slot
//   overlay_blend   PoseVisualizer's blend of a rendered frame into the camera image, one thread per byte
#pragma once

#include "render_raster.h"

namespace aae_render {

#define SCENE_MAX_DRAWS 256          /* AAE_SCENE_MAX_DRAWS: the draw table travels in the kernel arguments */

struct SceneMesh {                   // one row of the device table aae_mesh_set_create writes
    const float* verts;
    const float* normals;
    const float* colors;
    const int32_t* faces;
    int32_t V, F;
};

struct SceneDraws {                  // the draw table, in the kernel arguments (no copy from pageable memory, capturable)
    uint16_t obj[SCENE_MAX_DRAWS];
    uint16_t scene[SCENE_MAX_DRAWS];
};

struct SceneArgs {
    const SceneMesh* meshes;         // [meshes of the set]
    int32_t Vmax, Fmax;              // the largest vertex / face count of the set: slot strides, the key's radix
    const double* Rs;                // [n_draws,9]
    const double* ts;                // [n_draws,3]
    RcCamera cam;
    RcLight light;
    int32_t n_draws, n_scenes;
    int32_t* rect;                   // [n_scenes,4] x0, y0, x1, y1 inclusive; empty when x0 > x1
    int32_t* bounds;                 // [n_draws,raster_blocks,4]  RcBounds of the fragments of each block of scene_raster
    int32_t raster_blocks;           // ceil(Fmax / RENDER_BLOCK)
    int32_t* draw_obj;               // [n_draws]    draws.obj in global memory, for scene_frame (the winning draw differs per lane)
    RcVertex* vtx;                   // [n_draws,Vmax]
    float* vary;                     // [n_draws,Vmax,RC_VARY]
    unsigned long long* keys;        // [n_scenes,H,W]
    SceneDraws draws;
};

// Integer min / max onto a word that the draws of a scene share, behind a load: the word only ever moves one way, so a value
// that would not move it needs no atomic (the filter the visibility key has).  Atomics onto one word are served one after the
// other (~11 ns each), and the rectangles of a call lie in a few cache lines: one per wave, unfiltered, they and not the
// arithmetic set the time of scene_vertex.
__device__ inline void shared_min(int32_t* p, int v) {
    if (v < __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(p, v);
}

__device__ inline void shared_max(int32_t* p, int v) {
    if (v > __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(p, v);
}

__global__ void __launch_bounds__(RENDER_BLOCK) scene_init(SceneArgs a) {
    const int i = blockIdx.x * RENDER_BLOCK + threadIdx.x;
    if (i < a.n_scenes) rect_reset(a.rect + (size_t)i * 4);
    if (i < a.n_draws) a.draw_obj[i] = a.draws.obj[i];
}

template <bool CAD>
__global__ void __launch_bounds__(RENDER_BLOCK) scene_vertex(SceneArgs a) {
    const int draw = blockIdx.y;
    const int i = blockIdx.x * RENDER_BLOCK + threadIdx.x;
    const SceneMesh m = a.meshes[a.draws.obj[draw]];
    RcBounds b;
    rc_bounds_empty(&b);
    if (i < m.V) {
        const double t[3] = {a.ts[(size_t)draw * 3], a.ts[(size_t)draw * 3 + 1], a.ts[(size_t)draw * 3 + 2]};
        const size_t slot = (size_t)draw * a.Vmax + i;
        b = vertex_stage<CAD, RC_VARY>(a.Rs + (size_t)draw * 9, t, a.cam, a.light, m.verts, m.normals, i, slot, a.vtx, a.vary,
                                       [](const double*, const double*, const float*, float*) {});
    }
    block_bounds(&b);
    if (threadIdx.x == 0 && b.x0 != INT32_MAX) {
        int32_t* r = a.rect + (size_t)a.draws.scene[draw] * 4;
        shared_min(r + 0, b.x0);
        shared_min(r + 1, b.y0);
        shared_max(r + 2, b.x1);
        shared_max(r + 3, b.y1);
    }
}

__global__ void __launch_bounds__(RENDER_BLOCK) scene_clear(SceneArgs a) {
    const int scene = blockIdx.y;
    clear_rect(a.rect + (size_t)scene * 4, a.keys + (size_t)scene * a.cam.W * a.cam.H, a.cam.W, a.cam.H);
}

__global__ void __launch_bounds__(RENDER_BLOCK) scene_raster(SceneArgs a) {
    const int draw = blockIdx.y;
    const SceneMesh m = a.meshes[a.draws.obj[draw]];
    RcBounds b;
    rc_bounds_empty(&b);
    raster_stage<true>(m.faces, m.F, a.vtx + (size_t)draw * a.Vmax, rc_scene_index((unsigned)draw, (unsigned)a.Fmax, 0u),
                       a.keys + (size_t)a.draws.scene[draw] * a.cam.W * a.cam.H, a.cam, &b);
    // the block's share of the draw's bounds: written by every block, empty or not, so the slot needs no initialisation
    block_bounds(&b);
    if (threadIdx.x == 0) {
        int32_t* d = a.bounds + ((size_t)draw * a.raster_blocks + blockIdx.x) * 4;
        d[0] = b.x0; d[1] = b.y0; d[2] = b.x1; d[3] = b.y1;
    }
}

// one wave per draw over the partial bounds of its raster blocks
__global__ void __launch_bounds__(64) scene_bbox(SceneArgs a, int32_t* bbs, int32_t* visible) {
    const int draw = blockIdx.x;
    const int32_t* d = a.bounds + (size_t)draw * a.raster_blocks * 4;
    RcBounds b;
    rc_bounds_empty(&b);
    for (int k = threadIdx.x; k < a.raster_blocks; k += 64) {
        b.x0 = min(b.x0, d[k * 4]); b.y0 = min(b.y0, d[k * 4 + 1]); b.x1 = max(b.x1, d[k * 4 + 2]); b.y1 = max(b.y1, d[k * 4 + 3]);
    }
    wave_bounds(&b);
    if (threadIdx.x == 0) rc_bounds_box(b, a.cam.W, a.cam.H, bbs + (size_t)draw * 4, visible + draw);
}

template <bool CAD>
__global__ void __launch_bounds__(RENDER_BLOCK) scene_frame(SceneArgs a, uint8_t* bgr_out, float* depth_out, int32_t* draw_out, int32_t* tri_out) {
    const int scene = blockIdx.y;
    const int o = blockIdx.x * RENDER_BLOCK + threadIdx.x;
    if (o >= a.cam.W * a.cam.H) return;
    const int x = o % a.cam.W, y = o / a.cam.W;
    int rx0, ry0, rw, rh;
    rect_of(a.rect + (size_t)scene * 4, a.cam.W, a.cam.H, &rx0, &ry0, &rw, &rh);
    const size_t p = (size_t)scene * a.cam.W * a.cam.H + o;
    const unsigned long long key = key_at(a.keys + p, x, y, rx0, ry0, rw, rh);
    int32_t draw, tri;
    rc_scene_decode(key, (uint32_t)a.Fmax, &draw, &tri);
    uint8_t bgr[3] = {0, 0, 0};
    if (draw >= 0) {
        const SceneMesh m = a.meshes[a.draw_obj[draw]];
        shade_of<CAD>(m.faces, m.colors, a.vtx + (size_t)draw * a.Vmax, a.vary + (size_t)draw * a.Vmax * RC_VARY, (unsigned)tri, x, y, a.cam.W,
                      a.cam.H, a.light, bgr);
    }
    bgr_out[p * 3] = bgr[0]; bgr_out[p * 3 + 1] = bgr[1]; bgr_out[p * 3 + 2] = bgr[2];
    depth_out[p] = rc_key_depth(key);
    if (draw_out) draw_out[p] = draw;
    if (tri_out) tri_out[p] = tri;
}

__global__ void __launch_bounds__(RENDER_BLOCK) overlay_blend(const uint8_t* image, const uint8_t* render, size_t n_bytes, int channel,
                                                              uint8_t* out) {
    const size_t e = (size_t)blockIdx.x * RENDER_BLOCK + threadIdx.x;
    if (e >= n_bytes) return;
    out[e] = rc_overlay(render[e], image[e], (int)(e % 3) == channel);
}

}  // namespace aae_render
