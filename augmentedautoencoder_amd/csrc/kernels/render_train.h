// Training pairs (gfx950): dataset.py:219-306 for a batch of rotations in six launches.  The geometry of a pair is done once:
// render_init_rect, render_clear, render_raster and render_bbox of render_raster.h run as they are; the vertex stage below
// also writes v_L of the view's own light, and the crop kernel maps every output pixel twice (true box: train_y, shifted
// box: train_x and mask_x) and shades each sample from the shared visibility buffer.
//
//   render_vertex_train  per (view, vertex): what render_vertex writes, with RC_VARY_TRAIN floats of varyings
//   render_train_crop    per (view, output pixel): train_y BGR, train_x BGR, mask_x
//
// Stores.  A thread owns 7 bytes (3 + 3 + 1) in three arrays.  Consecutive lanes own consecutive pixels, so a wave's byte
// stores of one channel fall into one 192-byte (mask: 64-byte) span and the six colour stores of a wave fill two spans
// completely; the write-back cache merges them into whole lines.  Packing four pixels a thread into dword stores would cut
// the store instructions by 4 but also the threads that hide the latency of the two dependent gathers (key, then vertices)
// each sample needs, which is where this kernel spends its time (as render_crop does); the stores stay bytes.
#pragma once

#include "render_raster.h"

namespace aae_render {

struct TrainArgs {
    const float* lights;             // [n,6] pos xyz, ambient, diffuse, specular of train_x
    const double* offsets;           // [n,2] u_x, u_y: the shift of train_x's box in units of its width / height
};

__device__ inline RcLight light_of(const float* lights, int view) {
    const float* l = lights + (size_t)view * 6;
    RcLight out;
    out.pos[0] = l[0]; out.pos[1] = l[1]; out.pos[2] = l[2];
    out.ambient = l[3]; out.diffuse = l[4]; out.specular = l[5];
    return out;
}

// a.vary holds RC_VARY_TRAIN floats per (view, vertex); a.ts is null (one translation a call)
template <bool CAD>
__global__ void __launch_bounds__(RENDER_BLOCK) render_vertex_train(RenderArgs a, TrainArgs ta) {
    const int view = blockIdx.y;
    const int i = blockIdx.x * RENDER_BLOCK + threadIdx.x;
    RcBounds b;
    rc_bounds_empty(&b);
    if (i < a.V) {
        const double t[3] = {a.t[0], a.t[1], a.t[2]};
        const size_t slot = (size_t)view * a.V + i;
        b = vertex_stage<CAD, RC_VARY_TRAIN>(a.Rs + (size_t)view * 9, t, a.cam, a.light, a.verts, a.normals, i, slot, a.vtx, a.vary,
                                             [&](const double* Rr, const double* t, const float* p, float* vary) {
                                                 rc_light_dir<CAD>(Rr, t, light_of(ta.lights, view), p, vary + RC_VARY);
                                             });
    }
    view_rect_add(a, view, b);
}

// the frame pixel that output pixel o of a crop x crop patch of box bb samples (extract_square_patch + resizeNN), and its key;
// false when the source rectangle is empty
__device__ inline bool train_sample(const RenderArgs& a, int view, const int32_t* bb, double pad_factor, int crop, int o, int rx0, int ry0,
                                    int rw, int rh, int* x, int* y, unsigned long long* key) {
    int32_t left, right, top, bottom;
    rc_crop_rect(bb, pad_factor, a.cam.W, a.cam.H, &left, &right, &top, &bottom);
    if (!(right > left && bottom > top)) return false;
    *x = left + rc_nearest_src(o % crop, crop, right - left);
    *y = top + rc_nearest_src(o / crop, crop, bottom - top);
    *key = key_at(a, view, *x, *y, rx0, ry0, rw, rh);
    return true;
}

// The two samples spell out their triangle lookup and shading (shade_of with the training stride): through one function the CAD
// form of this kernel compiles to other registers and another occupancy, which nobody has measured.
template <bool CAD>
__global__ void __launch_bounds__(RENDER_BLOCK) render_train_crop(RenderArgs a, TrainArgs ta, const int32_t* bbs, const int32_t* visible,
                                                                  double pad_factor, int crop, uint8_t* train_x, uint8_t* mask_x,
                                                                  uint8_t* train_y) {
    const int view = blockIdx.y;
    const int o = blockIdx.x * RENDER_BLOCK + threadIdx.x;
    if (o >= crop * crop) return;
    uint8_t by[3] = {0, 0, 0}, bx[3] = {0, 0, 0};
    uint8_t mask = 1;
    if (visible[view]) {
        const int32_t* bb = bbs + (size_t)view * 4;
        const RcVertex* vv = a.vtx + (size_t)view * a.V;
        const float* vb = a.vary + (size_t)view * a.V * RC_VARY_TRAIN;
        int rx0, ry0, rw, rh;
        load_rect(a, view, &rx0, &ry0, &rw, &rh);
        int x, y;
        unsigned long long key;
        if (train_sample(a, view, bb, pad_factor, crop, o, rx0, ry0, rw, rh, &x, &y, &key) && key != RC_BACKGROUND) {
            const unsigned tri = (unsigned)(key & 0xFFFFFFFFull);
            RcTri T;
            tri_of(a.faces, vv, (int)tri, a.cam.W, a.cam.H, &T);
            const int32_t* f = a.faces + (size_t)tri * 3;
            rc_shade<CAD>(T, x, y, vb + (size_t)f[0] * RC_VARY_TRAIN, vb + (size_t)f[1] * RC_VARY_TRAIN, vb + (size_t)f[2] * RC_VARY_TRAIN,
                          a.colors + (size_t)f[0] * 3, a.colors + (size_t)f[1] * 3, a.colors + (size_t)f[2] * 3, a.light, by);
        }
        int32_t off[4];
        rc_offset_box(bb, ta.offsets[(size_t)view * 2], ta.offsets[(size_t)view * 2 + 1], off);
        if (train_sample(a, view, off, pad_factor, crop, o, rx0, ry0, rw, rh, &x, &y, &key) && key != RC_BACKGROUND) {
            mask = 0;
            const unsigned tri = (unsigned)(key & 0xFFFFFFFFull);
            RcTri T;
            tri_of(a.faces, vv, (int)tri, a.cam.W, a.cam.H, &T);
            const int32_t* f = a.faces + (size_t)tri * 3;
            rc_shade_relit<CAD>(T, x, y, vb + (size_t)f[0] * RC_VARY_TRAIN, vb + (size_t)f[1] * RC_VARY_TRAIN, vb + (size_t)f[2] * RC_VARY_TRAIN,
                                a.colors + (size_t)f[0] * 3, a.colors + (size_t)f[1] * 3, a.colors + (size_t)f[2] * 3, light_of(ta.lights, view), bx);
        }
    }
    const size_t p = (size_t)view * crop * crop + o;
    uint8_t* dy = train_y + p * 3;
    dy[0] = by[0]; dy[1] = by[1]; dy[2] = by[2];
    uint8_t* dx = train_x + p * 3;
    dx[0] = bx[0]; dx[1] = bx[1]; dx[2] = bx[2];
    mask_x[p] = mask;
}

}  // namespace aae_render
