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

__global__ void __launch_bounds__(RENDER_BLOCK) render_init_rect(RenderArgs a) {
    const int v = blockIdx.x * RENDER_BLOCK + threadIdx.x;
    if (v >= a.n) return;
    int32_t* r = a.rect + (size_t)v * 4;
    r[0] = INT32_MAX; r[1] = INT32_MAX; r[2] = INT32_MIN; r[3] = INT32_MIN;
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

template <bool CAD>
__global__ void __launch_bounds__(RENDER_BLOCK) render_vertex(RenderArgs a) {
    const int view = blockIdx.y;
    const int i = blockIdx.x * RENDER_BLOCK + threadIdx.x;
    int x0 = INT32_MAX, y0 = INT32_MAX, x1 = INT32_MIN, y1 = INT32_MIN;
    if (i < a.V) {
        const double* R = a.Rs + (size_t)view * 9;
        double t[3];
        if (a.ts) {
            t[0] = a.ts[(size_t)view * 3]; t[1] = a.ts[(size_t)view * 3 + 1]; t[2] = a.ts[(size_t)view * 3 + 2];
        } else {
            t[0] = a.t[0]; t[1] = a.t[1]; t[2] = a.t[2];
        }
        double Rr[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) Rr[k] = R[k];
        const float p[3] = {a.verts[(size_t)i * 3], a.verts[(size_t)i * 3 + 1], a.verts[(size_t)i * 3 + 2]};
        const float nr[3] = {a.normals[(size_t)i * 3], a.normals[(size_t)i * 3 + 1], a.normals[(size_t)i * 3 + 2]};
        RcVertex out;
        float vary[RC_VARY];
        rc_vertex<CAD>(Rr, t, a.cam, a.light, p, nr, &out, vary);
        const size_t slot = (size_t)view * a.V + i;
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
    x0 = wave_min(x0); y0 = wave_min(y0); x1 = wave_max(x1); y1 = wave_max(y1);
    if ((threadIdx.x & 63) == 0 && x0 != INT32_MAX) {
        int32_t* r = a.rect + (size_t)view * 4;
        atomicMin(r + 0, x0);
        atomicMin(r + 1, y0);
        atomicMax(r + 2, x1);
        atomicMax(r + 3, y1);
    }
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

__global__ void __launch_bounds__(RENDER_BLOCK) render_clear(RenderArgs a) {
    const int view = blockIdx.y;
    int x0, y0, w, h;
    load_rect(a, view, &x0, &y0, &w, &h);
    unsigned long long* keys = a.keys + (size_t)view * a.cam.W * a.cam.H;
    const int total = w * h;
    for (int i = blockIdx.x * RENDER_BLOCK + threadIdx.x; i < total; i += gridDim.x * RENDER_BLOCK) {
        const int y = y0 + i / w, x = x0 + i % w;
        keys[(size_t)y * a.cam.W + x] = RC_BACKGROUND;
    }
}

// triangle `tri` of a face list, from the snapped vertices vv of its view (scenes: of its draw)
__device__ inline void tri_of(const int32_t* faces, const RcVertex* vv, int tri, int W, int H, RcTri* T) {
    const int32_t* f = faces + (size_t)tri * 3;
    const RcVertex v0 = vv[f[0]], v1 = vv[f[1]], v2 = vv[f[2]];
    rc_tri_setup(v0, v1, v2, W, H, T);
}

__device__ inline void load_tri(const RenderArgs& a, int view, int tri, RcTri* T) {
    tri_of(a.faces, a.vtx + (size_t)view * a.V, tri, a.cam.W, a.cam.H, T);
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

__global__ void __launch_bounds__(RENDER_BLOCK) render_raster(RenderArgs a) {
    const int view = blockIdx.y;
    const int tri = blockIdx.x * RENDER_BLOCK + threadIdx.x;
    const int lane = threadIdx.x & 63;
    unsigned long long* keys = a.keys + (size_t)view * a.cam.W * a.cam.H;
    RcTri T;
    T.ok = 0;
    T.px0 = T.py0 = 0;
    T.px1 = T.py1 = -1;
    if (tri < a.F) load_tri(a, view, tri, &T);
    const int bw = T.px1 - T.px0 + 1, bh = T.py1 - T.py0 + 1;
    const bool large = T.ok && (long long)bw * bh > RENDER_WAVE_BOX;
    if (T.ok && !large) {
        for (int y = T.py0; y <= T.py1; ++y)
            for (int x = T.px0; x <= T.px1; ++x) raster_pixel(T, x, y, a.cam.far_, (unsigned)tri, keys, a.cam.W);
    }
    // the wave takes its large triangles one after the other, lanes striding over the pixel box
    unsigned long long todo = __ballot(large);
    while (todo) {
        const int src = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        const int wtri = __shfl(tri, src);
        RcTri S;
        load_tri(a, view, wtri, &S);
        const int sw = S.px1 - S.px0 + 1;
        const long long total = (long long)sw * (S.py1 - S.py0 + 1);
        for (long long i = lane; i < total; i += 64) {
            const int y = S.py0 + (int)(i / sw), x = S.px0 + (int)(i % sw);
            raster_pixel(S, x, y, a.cam.far_, (unsigned)wtri, keys, a.cam.W);
        }
    }
}

// calc_2d_bbox over the covered pixels of the view's rectangle; visible[view] = 0 when nothing is covered (bb := 0)
__global__ void __launch_bounds__(RENDER_BLOCK) render_bbox(RenderArgs a, int32_t* bbs, int32_t* visible) {
    __shared__ int red[4][RENDER_BLOCK / 64];
    const int view = blockIdx.x;
    int x0, y0, w, h;
    load_rect(a, view, &x0, &y0, &w, &h);
    const unsigned long long* keys = a.keys + (size_t)view * a.cam.W * a.cam.H;
    int mnx = INT32_MAX, mny = INT32_MAX, mxx = INT32_MIN, mxy = INT32_MIN;
    const int total = w * h;
    for (int i = threadIdx.x; i < total; i += RENDER_BLOCK) {
        const int y = y0 + i / w, x = x0 + i % w;
        if (keys[(size_t)y * a.cam.W + x] != RC_BACKGROUND) {
            mnx = min(mnx, x); mny = min(mny, y); mxx = max(mxx, x); mxy = max(mxy, y);
        }
    }
    mnx = wave_min(mnx); mny = wave_min(mny); mxx = wave_max(mxx); mxy = wave_max(mxy);
    const int wv = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        red[0][wv] = mnx; red[1][wv] = mny; red[2][wv] = mxx; red[3][wv] = mxy;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 1; k < RENDER_BLOCK / 64; ++k) {
            mnx = min(mnx, red[0][k]); mny = min(mny, red[1][k]); mxx = max(mxx, red[2][k]); mxy = max(mxy, red[3][k]);
        }
        int32_t* bb = bbs + (size_t)view * 4;
        if (mnx == INT32_MAX) {
            bb[0] = bb[1] = bb[2] = bb[3] = 0;
            visible[view] = 0;
        } else {
            rc_bbox(mnx, mny, mxx, mxy, a.cam.W, a.cam.H, bb);
            visible[view] = 1;
        }
    }
}

// key of frame pixel (x, y) of a view: background outside the view's rectangle (never cleared there, never read)
__device__ inline unsigned long long key_at(const RenderArgs& a, int view, int x, int y, int rx0, int ry0, int rw, int rh) {
    if (x < rx0 || y < ry0 || x >= rx0 + rw || y >= ry0 + rh) return RC_BACKGROUND;
    return a.keys[((size_t)view * a.cam.H + y) * a.cam.W + x];
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
