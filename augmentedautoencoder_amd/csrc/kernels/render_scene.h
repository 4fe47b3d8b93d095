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

// (min, min, max, max) of four ints over the block; the result is valid in thread 0.  Every thread of the block must call it.
__device__ inline void block_bounds(int* x0, int* y0, int* x1, int* y1) {
    __shared__ int red[4][RENDER_BLOCK / 64];
    *x0 = wave_min(*x0); *y0 = wave_min(*y0); *x1 = wave_max(*x1); *y1 = wave_max(*y1);
    const int wv = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        red[0][wv] = *x0; red[1][wv] = *y0; red[2][wv] = *x1; red[3][wv] = *y1;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 1; k < RENDER_BLOCK / 64; ++k) {
            *x0 = min(*x0, red[0][k]); *y0 = min(*y0, red[1][k]); *x1 = max(*x1, red[2][k]); *y1 = max(*y1, red[3][k]);
        }
    }
}

__global__ void __launch_bounds__(RENDER_BLOCK) scene_init(SceneArgs a) {
    const int i = blockIdx.x * RENDER_BLOCK + threadIdx.x;
    if (i < a.n_scenes) {
        int32_t* r = a.rect + (size_t)i * 4;
        r[0] = INT32_MAX; r[1] = INT32_MAX; r[2] = INT32_MIN; r[3] = INT32_MIN;
    }
    if (i < a.n_draws) a.draw_obj[i] = a.draws.obj[i];
}

template <bool CAD>
__global__ void __launch_bounds__(RENDER_BLOCK) scene_vertex(SceneArgs a) {
    const int draw = blockIdx.y;
    const int i = blockIdx.x * RENDER_BLOCK + threadIdx.x;
    const SceneMesh m = a.meshes[a.draws.obj[draw]];
    int x0 = INT32_MAX, y0 = INT32_MAX, x1 = INT32_MIN, y1 = INT32_MIN;
    if (i < m.V) {
        const double* R = a.Rs + (size_t)draw * 9;
        const double t[3] = {a.ts[(size_t)draw * 3], a.ts[(size_t)draw * 3 + 1], a.ts[(size_t)draw * 3 + 2]};
        double Rr[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) Rr[k] = R[k];
        const float p[3] = {m.verts[(size_t)i * 3], m.verts[(size_t)i * 3 + 1], m.verts[(size_t)i * 3 + 2]};
        const float nr[3] = {m.normals[(size_t)i * 3], m.normals[(size_t)i * 3 + 1], m.normals[(size_t)i * 3 + 2]};
        RcVertex out;
        float vary[RC_VARY];
        rc_vertex<CAD>(Rr, t, a.cam, a.light, p, nr, &out, vary);
        const size_t slot = (size_t)draw * a.Vmax + i;
        a.vtx[slot] = out;
        float* vd = a.vary + slot * RC_VARY;
#pragma unroll
        for (int k = 0; k < RC_VARY; ++k) vd[k] = vary[k];
        if (out.x != RC_INVALID) {
            x0 = rc_clampi(rc_pixel_lo(out.x), 0, a.cam.W - 1);
            x1 = rc_clampi(rc_pixel_hi(out.x), 0, a.cam.W - 1);
            y0 = rc_clampi(rc_pixel_lo(out.y), 0, a.cam.H - 1);
            y1 = rc_clampi(rc_pixel_hi(out.y), 0, a.cam.H - 1);
        }
    }
    block_bounds(&x0, &y0, &x1, &y1);
    if (threadIdx.x == 0 && x0 != INT32_MAX) {
        int32_t* r = a.rect + (size_t)a.draws.scene[draw] * 4;
        shared_min(r + 0, x0);
        shared_min(r + 1, y0);
        shared_max(r + 2, x1);
        shared_max(r + 3, y1);
    }
}

__global__ void __launch_bounds__(RENDER_BLOCK) scene_clear(SceneArgs a) {
    const int scene = blockIdx.y;
    int x0, y0, w, h;
    rect_of(a.rect + (size_t)scene * 4, a.cam.W, a.cam.H, &x0, &y0, &w, &h);
    unsigned long long* keys = a.keys + (size_t)scene * a.cam.W * a.cam.H;
    const int total = w * h;
    for (int i = blockIdx.x * RENDER_BLOCK + threadIdx.x; i < total; i += gridDim.x * RENDER_BLOCK) {
        const int y = y0 + i / w, x = x0 + i % w;
        keys[(size_t)y * a.cam.W + x] = RC_BACKGROUND;
    }
}

__global__ void __launch_bounds__(RENDER_BLOCK) scene_raster(SceneArgs a) {
    const int draw = blockIdx.y;
    const int tri = blockIdx.x * RENDER_BLOCK + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const SceneMesh m = a.meshes[a.draws.obj[draw]];
    unsigned long long* keys = a.keys + (size_t)a.draws.scene[draw] * a.cam.W * a.cam.H;
    const RcVertex* vv = a.vtx + (size_t)draw * a.Vmax;
    const unsigned base = rc_scene_index((unsigned)draw, (unsigned)a.Fmax, 0u);
    RcBounds b;
    rc_bounds_empty(&b);
    RcTri T;
    T.ok = 0;
    T.px0 = T.py0 = 0;
    T.px1 = T.py1 = -1;
    if (tri < m.F) tri_of(m.faces, vv, tri, a.cam.W, a.cam.H, &T);
    const int bw = T.px1 - T.px0 + 1, bh = T.py1 - T.py0 + 1;
    const bool large = T.ok && (long long)bw * bh > RENDER_WAVE_BOX;
    if (T.ok && !large) {
        for (int y = T.py0; y <= T.py1; ++y)
            for (int x = T.px0; x <= T.px1; ++x)
                if (raster_pixel(T, x, y, a.cam.far_, base + (unsigned)tri, keys, a.cam.W)) rc_bounds_add(&b, x, y);
    }
    // the wave takes its large triangles one after the other, lanes striding over the pixel box
    unsigned long long todo = __ballot(large);
    while (todo) {
        const int src = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        const int wtri = __shfl(tri, src);
        RcTri S;
        tri_of(m.faces, vv, wtri, a.cam.W, a.cam.H, &S);
        const int sw = S.px1 - S.px0 + 1;
        const long long total = (long long)sw * (S.py1 - S.py0 + 1);
        for (long long i = lane; i < total; i += 64) {
            const int y = S.py0 + (int)(i / sw), x = S.px0 + (int)(i % sw);
            if (raster_pixel(S, x, y, a.cam.far_, base + (unsigned)wtri, keys, a.cam.W)) rc_bounds_add(&b, x, y);
        }
    }
    // the block's share of the draw's bounds: written by every block, empty or not, so the slot needs no initialisation
    int x0 = b.x0, y0 = b.y0, x1 = b.x1, y1 = b.y1;
    block_bounds(&x0, &y0, &x1, &y1);
    if (threadIdx.x == 0) {
        int32_t* d = a.bounds + ((size_t)draw * a.raster_blocks + blockIdx.x) * 4;
        d[0] = x0; d[1] = y0; d[2] = x1; d[3] = y1;
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
    b.x0 = wave_min(b.x0); b.y0 = wave_min(b.y0); b.x1 = wave_max(b.x1); b.y1 = wave_max(b.y1);
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
    // background outside the scene's rectangle (never cleared there, never read)
    const unsigned long long key = (x < rx0 || y < ry0 || x >= rx0 + rw || y >= ry0 + rh) ? RC_BACKGROUND : a.keys[p];
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
