// The mesh rasteriser's kernels (gfx950): a batch of views of one mesh in six launches, no host synchronisation between
// them.  All arithmetic that decides an image lives in render_core.h; this file is the iteration space around it.
//
//   render_init_rect     per view: empty screen rectangle (the workspace may arrive full of garbage)
//   render_vertex        per (view, vertex): snapped xy, float64 z, fp32 varyings; the view's screen rectangle by
//                        wave-reduced integer min / max atomics
//   render_clear         visibility keys of each view's rectangle := background
//   render_raster        per (view, triangle): one thread rasterises a small triangle; a triangle whose pixel box holds
//                        more than RENDER_WAVE_BOX pixels is rasterised by its whole wave, 64 pixels at a time
//   render_bbox          per view: calc_2d_bbox of the covered pixels, the visible flag
//   render_crop          the fused embedding path: one thread per OUTPUT pixel of the square crop, shaded from the
//                        visibility buffer (the colour frame is never materialised)
//   render_frame         full frames: BGR + fp32 depth (+ the index of the visible face)
//
// The bodies of the stages are __device__ functions of this file (rect_reset, vertex_stage, clear_rect, raster_stage,
// block_bounds, key_at, shade_of): the scene kernels (render_scene.h) and the training forms (render_train.h) are other
// iteration spaces and reductions around the same bodies.
//
// Visibility is a 64-bit atomicMin per fragment on global memory (a vector atomic); everything else is plain stores.
#pragma once

#include "render_core.h"

namespace aae_render {

#define RENDER_BLOCK 256
#define RENDER_WAVE_BOX 128          /* pixel-box area above which a triangle goes to the wave-cooperative path */
#define RENDER_CLEAR_BLOCKS 32       /* blocks per view of the clear launch (each strides over the rectangle)   */

struct RenderArgs {
    const float* verts;              // [V,3] (already scaled by vertex_scale)
    const float* normals;            // [V,3]
    const float* colors;             // [V,3] rgb in [0,1]
    const int32_t* faces;            // [F,3], every index in [0,V) (checked by aae_mesh_create)
    int32_t V, F;
    const double* Rs;                // [n,9]
    const double* ts;                // [n,3], or nullptr: t below for every view
    double t[3];
    RcCamera cam;
    RcLight light;
    int32_t n;
    int32_t* rect;                   // [n,4] x0, y0, x1, y1 inclusive; empty when x0 > x1
    RcVertex* vtx;                   // [n,V]
    float* vary;                     // [n,V,RC_VARY]
    unsigned long long* keys;        // [n,H,W]
};

// the empty rectangle of a view (scene): every usable vertex shrinks x0, y0 and grows x1, y1
__device__ inline void rect_reset(int32_t* r) {
    r[0] = INT32_MAX; r[1] = INT32_MAX; r[2] = INT32_MIN; r[3] = INT32_MIN;
}

__global__ void __launch_bounds__(RENDER_BLOCK) render_init_rect(RenderArgs a) {
    const int v = blockIdx.x * RENDER_BLOCK + threadIdx.x;
    if (v < a.n) rect_reset(a.rect + (size_t)v * 4);
}

__device__ inline int wave_min(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o));
    return v;
}

__device__ inline int wave_max(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o));
    return v;
}

__device__ inline void wave_bounds(RcBounds* b) {
    b->x0 = wave_min(b->x0); b->y0 = wave_min(b->y0); b->x1 = wave_max(b->x1); b->y1 = wave_max(b->y1);
}

// bounds over the block; the result is valid in thread 0.  Every thread of the block must call it.
__device__ inline void block_bounds(RcBounds* b) {
    __shared__ int red[4][RENDER_BLOCK / 64];
    wave_bounds(b);
    const int wv = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        red[0][wv] = b->x0; red[1][wv] = b->y0; red[2][wv] = b->x1; red[3][wv] = b->y1;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 1; k < RENDER_BLOCK / 64; ++k) {
            b->x0 = min(b->x0, red[0][k]); b->y0 = min(b->y0, red[1][k]); b->x1 = max(b->x1, red[2][k]); b->y1 = max(b->y1, red[3][k]);
        }
    }
}

// The vertex stage of one vertex: vertex i of the mesh under (R, t) -> vtx[slot], its NV varyings -> vary_out[slot * NV ...]; returns
// the pixels the vertex may touch, clamped to the frame (empty for a vertex no triangle may use).  more(Rr, t, p, vary) runs between
// rc_vertex and the stores: the training form fills its varyings beyond RC_VARY there.  The kernels around it differ in how they
// reduce the bounds.  (The slot's addresses are formed after rc_vertex: formed by the caller, the training form takes other registers.)
template <bool CAD, int NV, class More>
__device__ inline RcBounds vertex_stage(const double* R, const double* t, const RcCamera& cam, const RcLight& light, const float* verts,
                                        const float* normals, int i, size_t slot, RcVertex* vtx, float* vary_out, More more) {
    double Rr[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) Rr[k] = R[k];
    const float p[3] = {verts[(size_t)i * 3], verts[(size_t)i * 3 + 1], verts[(size_t)i * 3 + 2]};
    const float nr[3] = {normals[(size_t)i * 3], normals[(size_t)i * 3 + 1], normals[(size_t)i * 3 + 2]};
    RcVertex out;
    float vary[NV];
    rc_vertex<CAD>(Rr, t, cam, light, p, nr, &out, vary);
    more(Rr, t, p, vary);
    vtx[slot] = out;
    float* vd = vary_out + slot * NV;
#pragma unroll
    for (int k = 0; k < NV; ++k) vd[k] = vary[k];
    RcBounds b;
    rc_bounds_empty(&b);
    if (out.x != RC_INVALID) {
        b.x0 = rc_clampi(rc_pixel_lo(out.x), 0, cam.W - 1);
        b.x1 = rc_clampi(rc_pixel_hi(out.x), 0, cam.W - 1);
        b.y0 = rc_clampi(rc_pixel_lo(out.y), 0, cam.H - 1);
        b.y1 = rc_clampi(rc_pixel_hi(out.y), 0, cam.H - 1);
    }
    return b;
}

// the view's rectangle from the bounds of a block's vertices: one integer min / max atomic per wave and word
__device__ inline void view_rect_add(const RenderArgs& a, int view, RcBounds b) {
    wave_bounds(&b);
    if ((threadIdx.x & 63) == 0 && b.x0 != INT32_MAX) {
        int32_t* r = a.rect + (size_t)view * 4;
        atomicMin(r + 0, b.x0);
        atomicMin(r + 1, b.y0);
        atomicMax(r + 2, b.x1);
        atomicMax(r + 3, b.y1);
    }
}

template <bool CAD>
__global__ void __launch_bounds__(RENDER_BLOCK) render_vertex(RenderArgs a) {
    const int view = blockIdx.y;
    const int i = blockIdx.x * RENDER_BLOCK + threadIdx.x;
    RcBounds b;
    rc_bounds_empty(&b);
    if (i < a.V) {
        double t[3];
        if (a.ts) {
            t[0] = a.ts[(size_t)view * 3]; t[1] = a.ts[(size_t)view * 3 + 1]; t[2] = a.ts[(size_t)view * 3 + 2];
        } else {
            t[0] = a.t[0]; t[1] = a.t[1]; t[2] = a.t[2];
        }
        b = vertex_stage<CAD, RC_VARY>(a.Rs + (size_t)view * 9, t, a.cam, a.light, a.verts, a.normals, i, (size_t)view * a.V + i, a.vtx, a.vary,
                                       [](const double*, const double*, const float*, float*) {});
    }
    view_rect_add(a, view, b);
}

// the view's rectangle, or an empty one (w == 0) when no usable vertex set it
__device__ inline void rect_of(const int32_t* r, int W, int H, int* x0, int* y0, int* w, int* h) {
    const int rx0 = r[0], ry0 = r[1], rx1 = r[2], ry1 = r[3];
    const bool ok = rx0 >= 0 && ry0 >= 0 && rx1 < W && ry1 < H && rx0 <= rx1 && ry0 <= ry1;
    *x0 = ok ? rx0 : 0;
    *y0 = ok ? ry0 : 0;
    *w = ok ? rx1 - rx0 + 1 : 0;
    *h = ok ? ry1 - ry0 + 1 : 0;
}

__device__ inline void load_rect(const RenderArgs& a, int view, int* x0, int* y0, int* w, int* h) {
    rect_of(a.rect + (size_t)view * 4, a.cam.W, a.cam.H, x0, y0, w, h);
}

// keys of the rectangle r of one key plane := background; the blocks of grid.x stride over the rectangle
__device__ inline void clear_rect(const int32_t* r, unsigned long long* keys, int W, int H) {
    int x0, y0, w, h;
    rect_of(r, W, H, &x0, &y0, &w, &h);
    const int total = w * h;
    for (int i = blockIdx.x * RENDER_BLOCK + threadIdx.x; i < total; i += gridDim.x * RENDER_BLOCK) {
        const int y = y0 + i / w, x = x0 + i % w;
        keys[(size_t)y * W + x] = RC_BACKGROUND;
    }
}

__global__ void __launch_bounds__(RENDER_BLOCK) render_clear(RenderArgs a) {
    const int view = blockIdx.y;
    clear_rect(a.rect + (size_t)view * 4, a.keys + (size_t)view * a.cam.W * a.cam.H, a.cam.W, a.cam.H);
}

// triangle `tri` of a face list, from the snapped vertices vv of its view (scenes: of its draw)
__device__ inline void tri_of(const int32_t* faces, const RcVertex* vv, int tri, int W, int H, RcTri* T) {
    const int32_t* f = faces + (size_t)tri * 3;
    const RcVertex v0 = vv[f[0]], v1 = vv[f[1]], v2 = vv[f[2]];
    rc_tri_setup(v0, v1, v2, W, H, T);
}

// true when the pixel holds a fragment of the triangle (covered, not beyond the far plane), whether or not it is visible
__device__ inline bool raster_pixel(const RcTri& T, int x, int y, double far_, unsigned tri, unsigned long long* keys, int W) {
    uint64_t key;
    if (rc_fragment_key(T, x, y, far_, tri, &key)) {
        unsigned long long* k = keys + (size_t)y * W + x;
        if ((unsigned long long)key < *k) atomicMin(k, (unsigned long long)key);      // keys only ever decrease: the plain read is a filter
        return true;
    }
    return false;
}

// The raster stage of thread blockIdx.x * RENDER_BLOCK + threadIdx.x: triangle `tri` of the F faces, from the snapped vertices vv,
// into the key plane `keys` with index base + tri.  BOUNDS: *b grows by the pixels the thread's fragments fell on.
template <bool BOUNDS>
__device__ inline void raster_stage(const int32_t* faces, int F, const RcVertex* vv, unsigned base, unsigned long long* keys, const RcCamera& cam,
                                    RcBounds* b) {
    const int tri = blockIdx.x * RENDER_BLOCK + threadIdx.x;
    const int lane = threadIdx.x & 63;
    RcTri T;
    T.ok = 0;
    T.px0 = T.py0 = 0;
    T.px1 = T.py1 = -1;
    if (tri < F) tri_of(faces, vv, tri, cam.W, cam.H, &T);
    const int bw = T.px1 - T.px0 + 1, bh = T.py1 - T.py0 + 1;
    const bool large = T.ok && (long long)bw * bh > RENDER_WAVE_BOX;
    if (T.ok && !large) {
        for (int y = T.py0; y <= T.py1; ++y)
            for (int x = T.px0; x <= T.px1; ++x) {
                const bool hit = raster_pixel(T, x, y, cam.far_, base + (unsigned)tri, keys, cam.W);
                if constexpr (BOUNDS) if (hit) rc_bounds_add(b, x, y);
            }
    }
    // the wave takes its large triangles one after the other, lanes striding over the pixel box
    unsigned long long todo = __ballot(large);
    while (todo) {
        const int src = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        const int wtri = __shfl(tri, src);
        RcTri S;
        tri_of(faces, vv, wtri, cam.W, cam.H, &S);
        const int sw = S.px1 - S.px0 + 1;
        const long long total = (long long)sw * (S.py1 - S.py0 + 1);
        for (long long i = lane; i < total; i += 64) {
            const int y = S.py0 + (int)(i / sw), x = S.px0 + (int)(i % sw);
            const bool hit = raster_pixel(S, x, y, cam.far_, base + (unsigned)wtri, keys, cam.W);
            if constexpr (BOUNDS) if (hit) rc_bounds_add(b, x, y);
        }
    }
}

__global__ void __launch_bounds__(RENDER_BLOCK) render_raster(RenderArgs a) {
    const int view = blockIdx.y;
    raster_stage<false>(a.faces, a.F, a.vtx + (size_t)view * a.V, 0u, a.keys + (size_t)view * a.cam.W * a.cam.H, a.cam, nullptr);
}

// calc_2d_bbox over the covered pixels of the view's rectangle; visible[view] = 0 when nothing is covered (bb := 0)
__global__ void __launch_bounds__(RENDER_BLOCK) render_bbox(RenderArgs a, int32_t* bbs, int32_t* visible) {
    const int view = blockIdx.x;
    int x0, y0, w, h;
    load_rect(a, view, &x0, &y0, &w, &h);
    const unsigned long long* keys = a.keys + (size_t)view * a.cam.W * a.cam.H;
    RcBounds b;
    rc_bounds_empty(&b);
    const int total = w * h;
    for (int i = threadIdx.x; i < total; i += RENDER_BLOCK) {
        const int y = y0 + i / w, x = x0 + i % w;
        if (keys[(size_t)y * a.cam.W + x] != RC_BACKGROUND) rc_bounds_add(&b, x, y);
    }
    block_bounds(&b);
    if (threadIdx.x == 0) rc_bounds_box(b, a.cam.W, a.cam.H, bbs + (size_t)view * 4, visible + view);
}

// the key *k of pixel (x, y) of a key plane with rectangle (rx0, ry0, rw, rh): background outside it (never cleared there, never read)
__device__ inline unsigned long long key_at(const unsigned long long* k, int x, int y, int rx0, int ry0, int rw, int rh) {
    if (x < rx0 || y < ry0 || x >= rx0 + rw || y >= ry0 + rh) return RC_BACKGROUND;
    return *k;
}

__device__ inline unsigned long long key_at(const RenderArgs& a, int view, int x, int y, int rx0, int ry0, int rw, int rh) {
    return key_at(a.keys + ((size_t)view * a.cam.H + y) * a.cam.W + x, x, y, rx0, ry0, rw, rh);
}

// colour of the fragment of triangle `tri` at (x, y): vv / vb are the snapped vertices and varyings of its view (draw)
template <bool CAD>
__device__ inline void shade_of(const int32_t* faces, const float* colors, const RcVertex* vv, const float* vb, unsigned tri, int x, int y,
                                int W, int H, const RcLight& light, uint8_t* bgr) {
    RcTri T;
    tri_of(faces, vv, (int)tri, W, H, &T);
    const int32_t* f = faces + (size_t)tri * 3;
    rc_shade<CAD>(T, x, y, vb + (size_t)f[0] * RC_VARY, vb + (size_t)f[1] * RC_VARY, vb + (size_t)f[2] * RC_VARY,
                  colors + (size_t)f[0] * 3, colors + (size_t)f[1] * 3, colors + (size_t)f[2] * 3, light, bgr);
}

template <bool CAD>
__device__ inline void shade_pixel(const RenderArgs& a, int view, unsigned tri, int x, int y, uint8_t* bgr) {
    shade_of<CAD>(a.faces, a.colors, a.vtx + (size_t)view * a.V, a.vary + (size_t)view * a.V * RC_VARY, tri, x, y, a.cam.W, a.cam.H, a.light, bgr);
}

template <bool CAD>
__global__ void __launch_bounds__(RENDER_BLOCK) render_crop(RenderArgs a, const int32_t* bbs, const int32_t* visible, double pad_factor,
                                                            int crop, uint8_t* out) {
    const int view = blockIdx.y;
    const int o = blockIdx.x * RENDER_BLOCK + threadIdx.x;
    if (o >= crop * crop) return;
    uint8_t bgr[3] = {0, 0, 0};
    if (visible[view]) {
        int32_t left, right, top, bottom;
        rc_crop_rect(bbs + (size_t)view * 4, pad_factor, a.cam.W, a.cam.H, &left, &right, &top, &bottom);
        if (right > left && bottom > top) {
            const int x = left + rc_nearest_src(o % crop, crop, right - left), y = top + rc_nearest_src(o / crop, crop, bottom - top);
            int rx0, ry0, rw, rh;
            load_rect(a, view, &rx0, &ry0, &rw, &rh);
            const unsigned long long key = key_at(a, view, x, y, rx0, ry0, rw, rh);
            if (key != RC_BACKGROUND) shade_pixel<CAD>(a, view, (unsigned)(key & 0xFFFFFFFFull), x, y, bgr);
        }
    }
    uint8_t* d = out + ((size_t)view * crop * crop + o) * 3;
    d[0] = bgr[0]; d[1] = bgr[1]; d[2] = bgr[2];
}

template <bool CAD>
__global__ void __launch_bounds__(RENDER_BLOCK) render_frame(RenderArgs a, uint8_t* bgr_out, float* depth_out, int32_t* tri_out) {
    const int view = blockIdx.y;
    const int o = blockIdx.x * RENDER_BLOCK + threadIdx.x;
    if (o >= a.cam.W * a.cam.H) return;
    const int x = o % a.cam.W, y = o / a.cam.W;
    int rx0, ry0, rw, rh;
    load_rect(a, view, &rx0, &ry0, &rw, &rh);
    const unsigned long long key = key_at(a, view, x, y, rx0, ry0, rw, rh);
    uint8_t bgr[3] = {0, 0, 0};
    if (key != RC_BACKGROUND) shade_pixel<CAD>(a, view, (unsigned)(key & 0xFFFFFFFFull), x, y, bgr);
    const size_t p = (size_t)view * a.cam.W * a.cam.H + o;
    bgr_out[p * 3] = bgr[0]; bgr_out[p * 3 + 1] = bgr[1]; bgr_out[p * 3 + 2] = bgr[2];
    depth_out[p] = rc_key_depth(key);
    if (tri_out) tri_out[p] = key == RC_BACKGROUND ? -1 : (int32_t)(key & 0xFFFFFFFFull);
}

}  // namespace aae_render
