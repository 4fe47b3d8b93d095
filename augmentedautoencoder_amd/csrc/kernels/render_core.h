// The mesh rasteriser's per-vertex, per-triangle and per-fragment functions as plain inline C++: the kernels of
// render_raster.h, render_scene.h and render_train.h call them on the device, tests/native/render_host.cpp, scene_host.cpp and
// train_host.cpp call the same text from serial loops on the host.
//
// What they restate (paths relative to the reference's auto_pose/meshrenderer/):
//   camera      gl_utils/camera.py:86-98,139-166 (realCamera + setIntrinsic: OpenCV extrinsics, z flipped into GL eye space)
//   reconst     shader/depth_shader_phong.vs, shader/depth_shader_phong.frag, meshrenderer_phong.py:41-60,101-168
//   cad         shader/cad_shader.vs, shader/cad_shader.frag, meshrenderer.py:37-47,84-137
//   bbox, crop  pysixd/view_sampler.py:10-15 (calc_2d_bbox), auto_pose/ae/dataset.py:354-373 (extract_square_patch)
//   pairs       auto_pose/ae/dataset.py:238-303 (render_training_images: second light, shifted box)
//
// The exact-geometry rule.  Pixel coordinates are computed in float64, snapped to 1/256 pixel, and everything that decides
// WHICH triangle a pixel shows is integer arithmetic on the snapped vertices or float64 arithmetic in one fixed order of
// operations (no contraction into fused multiply-adds: see the pragma below), so a float64 restatement in another language
// reproduces the visibility buffer bit for bit.  Only the colour of a fragment is computed in fp32.
#pragma once

#include <math.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define RC_HD __host__ __device__ inline
#else
#define RC_HD inline
#endif

// geometry must not depend on whether the compiler fuses a*b + c (hipcc contracts by default, NumPy never does)
#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace aae_render {

#define RC_SUBPIXEL_BITS 8                        /* vertices snap to 1/256 pixel                                  */
#define RC_SUBPIXEL 256
#define RC_HALF 128                               /* pixel (row i, column j) is sampled at (j + 0.5, i + 0.5)      */
#define RC_MAX_PIXEL 4194304.0                    /* a vertex beyond +-2^22 pixels drops its triangles             */
#define RC_INVALID INT32_MIN                      /* RcVertex.x of a vertex no triangle may use                    */
#define RC_BACKGROUND 0xFFFFFFFFFFFFFFFFull       /* visibility key of a pixel nothing covers                      */

struct RcCamera {
    double K00, K01, K02, K11, K12;               // the entries of K the projection reads (camera.py:156-157)
    double near_, far_;
    int32_t W, H;
};

struct RcLight {
    float pos[3];                                 // u_light_eye_pos / light_pos, eye coordinates
    float ambient, diffuse, specular;
};

struct RcVertex {                                 // one (view, vertex) after the vertex stage
    int32_t x, y;                                 // pixel coordinates in 1/256 pixel; x == RC_INVALID: unusable
    double z;                                     // z_c = v_view.z, the depth the fragment shader writes
};

#define RC_VARY 9                                 /* v_view, v_L (v_light_dir), v_normal                           */

// ---- vertex stage ----------------------------------------------------------------------------------------------------
// X_c = R X + t (OpenCV: z forward); eye coordinates P = (x_c, y_c, -z_c) (camera.py:88-93: T_world_view . z_flip);
// u = (K00 x_c + K01 y_c) / z_c + K02, v = K11 y_c / z_c + K12 (setIntrinsic's persp and glOrtho(0, W, H, 0), the
// viewport transform and the flipud of the read-back composed: row 0 is the top).
template <bool CAD>
RC_HD void rc_vertex(const double* R, const double* t, const RcCamera& cam, const RcLight& light, const float* p, const float* n,
                     RcVertex* out, float* vary) {
    const double X = (double)p[0], Y = (double)p[1], Z = (double)p[2];
    const double xc = ((R[0] * X + R[1] * Y) + R[2] * Z) + t[0];
    const double yc = ((R[3] * X + R[4] * Y) + R[5] * Z) + t[1];
    const double zc = ((R[6] * X + R[7] * Y) + R[8] * Z) + t[2];
    const double u = (cam.K00 * xc + cam.K01 * yc) / zc + cam.K02;
    const double v = (cam.K11 * yc) / zc + cam.K12;
    // a triangle with a vertex in front of the near plane is dropped whole (GL would clip it: a documented deviation)
    const bool ok = (zc >= cam.near_) && (fabs(u) <= RC_MAX_PIXEL) && (fabs(v) <= RC_MAX_PIXEL);
    out->x = ok ? (int32_t)floor(u * (double)RC_SUBPIXEL + 0.5) : RC_INVALID;
    out->y = ok ? (int32_t)floor(v * (double)RC_SUBPIXEL + 0.5) : 0;
    out->z = zc;

    // varyings, float64 here and fp32 from the interpolation on
    const double Px = xc, Py = yc, Pz = -zc;
    vary[0] = (float)(-Px);                                                  // v_view = -P
    vary[1] = (float)(-Py);
    vary[2] = (float)(-Pz);
    double Lx = (double)light.pos[0] - Px, Ly = (double)light.pos[1] - Py, Lz = (double)light.pos[2] - Pz;
    if (!CAD) {                                                              // depth_shader_phong.vs:30 normalises, cad_shader.vs:33 does not
        const double ll = sqrt(Lx * Lx + Ly * Ly + Lz * Lz);
        Lx /= ll; Ly /= ll; Lz /= ll;
    }
    vary[3] = (float)Lx;
    vary[4] = (float)Ly;
    vary[5] = (float)Lz;
    // normalize(transpose(inverse(view)) * vec4(n, 1.0)).xyz normalises the FOUR-vector (both vertex shaders, line 31):
    // with view = [A | b], A = diag(1,1,-1) R, b = (t_x, t_y, -t_z) that is A n / sqrt(|A n|^2 + w^2), w = 1 - b.(A n)
    const double nx = (double)n[0], ny = (double)n[1], nz = (double)n[2];
    const double ax = R[0] * nx + R[1] * ny + R[2] * nz;
    const double ay = R[3] * nx + R[4] * ny + R[5] * nz;
    const double az = -(R[6] * nx + R[7] * ny + R[8] * nz);
    const double w = 1.0 - (t[0] * ax + t[1] * ay - t[2] * az);
    const double nl = sqrt(ax * ax + ay * ay + az * az + w * w);
    vary[6] = (float)(ax / nl);
    vary[7] = (float)(ay / nl);
    vary[8] = (float)(az / nl);
}

// v_L of the same vertex under another light (training pairs: the view's own light next to the call's default one): the
// float64 expressions of rc_vertex's v_L in their order, so a view rendered with that light alone has these three floats
#define RC_VARY_TRAIN 12                          /* RC_VARY of the default light, then v_L of the view's light    */

template <bool CAD>
RC_HD void rc_light_dir(const double* R, const double* t, const RcLight& light, const float* p, float* vL) {
    const double X = (double)p[0], Y = (double)p[1], Z = (double)p[2];
    const double xc = ((R[0] * X + R[1] * Y) + R[2] * Z) + t[0];
    const double yc = ((R[3] * X + R[4] * Y) + R[5] * Z) + t[1];
    const double zc = ((R[6] * X + R[7] * Y) + R[8] * Z) + t[2];
    const double Px = xc, Py = yc, Pz = -zc;
    double Lx = (double)light.pos[0] - Px, Ly = (double)light.pos[1] - Py, Lz = (double)light.pos[2] - Pz;
    if (!CAD) {
        const double ll = sqrt(Lx * Lx + Ly * Ly + Lz * Lz);
        Lx /= ll; Ly /= ll; Lz /= ll;
    }
    vL[0] = (float)Lx;
    vL[1] = (float)Ly;
    vL[2] = (float)Lz;
}

// pixel columns (rows) whose sample can lie inside a triangle that has a vertex at snapped coordinate c: the screen
// rectangle of a view is the union of these over its usable vertices, clamped to the frame
RC_HD int32_t rc_pixel_lo(int32_t c) { return (int32_t)(((int64_t)c - RC_HALF + (RC_SUBPIXEL - 1)) >> RC_SUBPIXEL_BITS); }
RC_HD int32_t rc_pixel_hi(int32_t c) { return (int32_t)(((int64_t)c - RC_HALF) >> RC_SUBPIXEL_BITS); }
RC_HD int32_t rc_clampi(int32_t v, int32_t lo, int32_t hi) { return v < lo ? lo : (v > hi ? hi : v); }

// ---- triangle setup --------------------------------------------------------------------------------------------------
// Edge i is the one opposite vertex i; e_i(p) = A_i (p_x - ox_i) + B_i (p_y - oy_i) is its int64 edge function, oriented so
// that the interior is positive for either winding (the reference enables no culling).  e_0 + e_1 + e_2 = |2 area|.
struct RcTri {
    int64_t A[3], B[3];
    int32_t ox[3], oy[3];
    int32_t tl[3];                                // 1: a pixel exactly on this edge belongs to the triangle (top-left rule)
    double z[3];
    int32_t px0, py0, px1, py1;                   // inclusive pixel box, clipped to the frame
    int32_t ok;                                   // 0: dropped (unusable vertex, zero area, or a box outside the frame)
};

RC_HD void rc_tri_setup(const RcVertex& v0, const RcVertex& v1, const RcVertex& v2, int32_t W, int32_t H, RcTri* T) {
    T->ok = 0;
    T->px0 = T->py0 = 0;
    T->px1 = T->py1 = -1;
    if (v0.x == RC_INVALID || v1.x == RC_INVALID || v2.x == RC_INVALID) return;
    const int32_t xs[3] = {v0.x, v1.x, v2.x}, ys[3] = {v0.y, v1.y, v2.y};
    // |coordinates| <= 2^30, so differences fit 2^31 and each product 2^62; 2*area of a triangle inside that square fits too
    const int64_t area2 = (int64_t)(xs[2] - (int64_t)xs[1]) * ((int64_t)ys[0] - ys[1]) - ((int64_t)ys[2] - ys[1]) * ((int64_t)xs[0] - xs[1]);
    if (area2 == 0) return;                       // zero-area triangles are skipped
    const int64_t s = area2 > 0 ? 1 : -1;
#if defined(__clang__)
#pragma unroll
#endif
    for (int i = 0; i < 3; ++i) {
        const int a = (i + 1) % 3, b = (i + 2) % 3;                          // edge i runs from vertex a to vertex b
        const int64_t dx = (int64_t)xs[b] - xs[a], dy = (int64_t)ys[b] - ys[a];
        T->A[i] = -dy * s;
        T->B[i] = dx * s;
        T->ox[i] = xs[a];
        T->oy[i] = ys[a];
        // rows grow downwards: a left edge has the interior at larger x (A > 0), a top edge is horizontal with the
        // interior below (A == 0, B > 0); the edge a neighbour shares runs the other way and so excludes the pixel
        T->tl[i] = (T->A[i] > 0 || (T->A[i] == 0 && T->B[i] > 0)) ? 1 : 0;
    }
    T->z[0] = v0.z; T->z[1] = v1.z; T->z[2] = v2.z;
    int32_t xmin = xs[0] < xs[1] ? xs[0] : xs[1]; xmin = xmin < xs[2] ? xmin : xs[2];
    int32_t xmax = xs[0] > xs[1] ? xs[0] : xs[1]; xmax = xmax > xs[2] ? xmax : xs[2];
    int32_t ymin = ys[0] < ys[1] ? ys[0] : ys[1]; ymin = ymin < ys[2] ? ymin : ys[2];
    int32_t ymax = ys[0] > ys[1] ? ys[0] : ys[1]; ymax = ymax > ys[2] ? ymax : ys[2];
    const int32_t x0 = rc_pixel_lo(xmin), x1 = rc_pixel_hi(xmax), y0 = rc_pixel_lo(ymin), y1 = rc_pixel_hi(ymax);
    T->px0 = x0 < 0 ? 0 : x0;
    T->px1 = x1 > W - 1 ? W - 1 : x1;
    T->py0 = y0 < 0 ? 0 : y0;
    T->py1 = y1 > H - 1 ? H - 1 : y1;
    T->ok = (T->px0 <= T->px1 && T->py0 <= T->py1) ? 1 : 0;
}

// the three edge values at the sample of pixel (column px, row py); true when the sample is covered
RC_HD bool rc_edges(const RcTri& T, int32_t px, int32_t py, int64_t* e) {
    const int64_t sx = (int64_t)px * RC_SUBPIXEL + RC_HALF, sy = (int64_t)py * RC_SUBPIXEL + RC_HALF;
    bool in = true;
#if defined(__clang__)
#pragma unroll
#endif
    for (int i = 0; i < 3; ++i) {
        e[i] = T.A[i] * (sx - T.ox[i]) + T.B[i] * (sy - T.oy[i]);
        in = in && (e[i] > 0 || (e[i] == 0 && T.tl[i]));
    }
    return in;
}

// perspective-correct interpolation of v_view.z from the integer edge values, float64, rounded once to fp32
RC_HD double rc_depth_den(const RcTri& T, const int64_t* e) {
    return ((double)e[0] / T.z[0] + (double)e[1] / T.z[1]) + (double)e[2] / T.z[2];
}

RC_HD uint32_t rc_float_bits(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
}

RC_HD float rc_bits_float(uint32_t u) {
    float f;
    memcpy(&f, &u, 4);
    return f;
}

// The fragment of triangle `tri` at pixel (px, py): false when not covered or beyond the far plane, else its visibility
// key (fp32 bits of z) << 32 | tri.  z > 0, so the bits order as the values do; the minimum key over all triangles is
// GL_LESS with the first-drawn triangle winning ties, whatever order the triangles are rasterised in.
RC_HD bool rc_fragment_key(const RcTri& T, int32_t px, int32_t py, double far_, uint32_t tri, uint64_t* key) {
    int64_t e[3];
    if (!rc_edges(T, px, py, e)) return false;
    const double den = rc_depth_den(T, e);
    const double z = (double)(e[0] + e[1] + e[2]) / den;
    if (!(z <= far_)) return false;
    *key = ((uint64_t)rc_float_bits((float)z) << 32) | (uint64_t)tri;
    return true;
}

RC_HD float rc_key_depth(uint64_t key) { return key == RC_BACKGROUND ? 0.0f : rc_bits_float((uint32_t)(key >> 32)); }

// ---- fragment stage (fp32) -------------------------------------------------------------------------------------------
RC_HD void rc_normalize3(float* v) {
    const float l = sqrtf(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    v[0] /= l; v[1] /= l; v[2] /= l;
}

// Colour of the visible fragment of triangle T at (px, py): varyings interpolated perspective-correctly (weights
// (e_i / z_i) / sum_j (e_j / z_j)), then depth_shader_phong.frag:20-34 / cad_shader.frag:17-39; stored as the GL_RGB8
// attachment stores it, round(c * 255), in the B, G, R order glReadPixels(GL_BGR) returns.
// vary0..2: the RC_VARY floats of the three vertices; col0..2: their rgb in [0,1] (reconst only).
template <bool CAD>
RC_HD void rc_shade(const RcTri& T, int32_t px, int32_t py, const float* vary0, const float* vary1, const float* vary2,
                    const float* col0, const float* col1, const float* col2, const RcLight& light, uint8_t* bgr) {
    int64_t e[3];
    rc_edges(T, px, py, e);
    const double den = rc_depth_den(T, e);
    const float b0 = (float)(((double)e[0] / T.z[0]) / den), b1 = (float)(((double)e[1] / T.z[1]) / den),
                b2 = (float)(((double)e[2] / T.z[2]) / den);
    float vw[RC_VARY];
#if defined(__clang__)
#pragma unroll
#endif
    for (int k = 0; k < RC_VARY; ++k) vw[k] = b0 * vary0[k] + b1 * vary1[k] + b2 * vary2[k];
    float color[3];
    if (CAD) {
        color[0] = 223.f / 255; color[1] = 214.f / 255; color[2] = 205.f / 255;       // cad_shader.frag:21-23
    } else {
#if defined(__clang__)
#pragma unroll
#endif
        for (int k = 0; k < 3; ++k) color[k] = b0 * col0[k] + b1 * col1[k] + b2 * col2[k];
    }
    float* V = vw;
    float* L = vw + 3;
    float* N = vw + 6;
    rc_normalize3(N);
    rc_normalize3(L);
    rc_normalize3(V);
    const float ndl = N[0] * L[0] + N[1] * L[1] + N[2] * L[2];
    const float diff = fmaxf(ndl, 0.0f);
    // reflect(-L, N) = -L - 2 dot(N, -L) N = 2 (N.L) N - L; no shininess exponent
    const float rv = (2.0f * ndl * N[0] - L[0]) * V[0] + (2.0f * ndl * N[1] - L[1]) * V[1] + (2.0f * ndl * N[2] - L[2]) * V[2];
    const float spec = fmaxf(rv, 0.0f);
    const float wgt = light.ambient + light.diffuse * diff + light.specular * spec;
#if defined(__clang__)
#pragma unroll
#endif
    for (int k = 0; k < 3; ++k) {
        float c = fminf(wgt * color[k], 1.0f);
        c = fmaxf(c, 0.0f);
        bgr[2 - k] = (uint8_t)(int)(c * 255.0f + 0.5f);
    }
}

// ---- bounding box and crop -------------------------------------------------------------------------------------------
// calc_2d_bbox (pysixd/view_sampler.py:10-15) from the extremes of the covered pixels
RC_HD void rc_bbox(int32_t xmin, int32_t ymin, int32_t xmax, int32_t ymax, int32_t W, int32_t H, int32_t* bb) {
    const int32_t tlx = xmin - 1 > 0 ? xmin - 1 : 0, tly = ymin - 1 > 0 ? ymin - 1 : 0;
    const int32_t brx = xmax + 1 < W - 1 ? xmax + 1 : W - 1, bry = ymax + 1 < H - 1 ? ymax + 1 : H - 1;
    bb[0] = tlx; bb[1] = tly; bb[2] = brx - tlx; bb[3] = bry - tly;
}

// extract_square_patch (dataset.py:356-362): the source rectangle [left,right) x [top,bottom) of the frame
RC_HD void rc_crop_rect(const int32_t* bb, double pad_factor, int32_t W, int32_t H, int32_t* left, int32_t* right, int32_t* top,
                        int32_t* bottom) {
    const int32_t x = bb[0], y = bb[1], w = bb[2], h = bb[3];
    const int32_t size = (int32_t)((double)(h > w ? h : w) * pad_factor);
    const double cx = (double)x + (double)w / 2.0, cy = (double)y + (double)h / 2.0, hs = (double)size / 2.0;
    *left = (int32_t)fmax(cx - hs, 0.0);
    *right = (int32_t)fmin(cx + hs, (double)W);
    *top = (int32_t)fmax(cy - hs, 0.0);
    *bottom = (int32_t)fmin(cy + hs, (double)H);
}

// The shifted box of a training image (dataset.py:282-285, 356): obj_bb + [u_x w, u_y h, 0, 0] in float64, then
// .astype(np.int32), which truncates toward zero; w and h stay.  Its source rectangle is rc_crop_rect of the result.
RC_HD void rc_offset_box(const int32_t* bb, double ux, double uy, int32_t* out) {
    out[0] = (int32_t)((double)bb[0] + ux * (double)bb[2]);
    out[1] = (int32_t)((double)bb[1] + uy * (double)bb[3]);
    out[2] = bb[2];
    out[3] = bb[3];
}

// rc_shade of a fragment under the view's own light: tv0..2 are the RC_VARY_TRAIN floats of the three vertices; rc_shade gets
// copies of their varyings with v_L replaced, so the bytes are those of a render with that light alone
template <bool CAD>
RC_HD void rc_shade_relit(const RcTri& T, int32_t px, int32_t py, const float* tv0, const float* tv1, const float* tv2,
                          const float* col0, const float* col1, const float* col2, const RcLight& light, uint8_t* bgr) {
    float v0[RC_VARY], v1[RC_VARY], v2[RC_VARY];
#if defined(__clang__)
#pragma unroll
#endif
    for (int k = 0; k < RC_VARY; ++k) {
        const int s = (k >= 3 && k < 6) ? k + 6 : k;
        v0[k] = tv0[s]; v1[k] = tv1[s]; v2[k] = tv2[s];
    }
    rc_shade<CAD>(T, px, py, v0, v1, v2, col0, col1, col2, light, bgr);
}

// cv2.resize(INTER_NEAREST): OpenCV modules/imgproc/src/resize.cpp, resizeNN: x_ofs[x] = min(cvFloor(x * ifx), ssize.width - 1)
// with ifx = 1. / inv_scale_x and inv_scale_x = (double)dsize.width / ssize.width; rows alike (unpinned: cv2 is not a dependency)
RC_HD int32_t rc_nearest_src(int32_t d, int32_t dst, int32_t src) {
    const double inv = 1.0 / ((double)dst / (double)src);
    const int32_t s = (int32_t)floor((double)d * inv);
    return s < src - 1 ? s : src - 1;
}

// ---- scenes: several draws into one frame ------------------------------------------------------------------------------
// A draw is (mesh of a set, R, t, scene); the draws of one scene share one key buffer.  Within a draw nothing changes: the
// key's high word is still the fp32 bits of z.  The low word becomes draw * fmax + triangle (fmax: the largest face count of
// the set, draw: the draw's index in the call's arrays), so at equal fp32 depth the earlier draw wins, then the lower
// triangle: GL_LESS with the first-drawn fragment kept, whatever order the draws are rasterised in.
RC_HD bool rc_scene_fits(uint64_t n_draws, uint64_t fmax) { return n_draws * fmax <= 0xFFFFFFFFull; }      // 0 <= both < 2^32

RC_HD uint32_t rc_scene_index(uint32_t draw, uint32_t fmax, uint32_t tri) { return draw * fmax + tri; }

RC_HD void rc_scene_decode(uint64_t key, uint32_t fmax, int32_t* draw, int32_t* tri) {
    if (key == RC_BACKGROUND) {
        *draw = -1; *tri = -1;
        return;
    }
    const uint32_t low = (uint32_t)(key & 0xFFFFFFFFull);
    *draw = (int32_t)(low / fmax);
    *tri = (int32_t)(low % fmax);
}

// The box of a draw is calc_2d_bbox of the draw rendered alone (meshrenderer.py:172-183), not of its visible part: the
// extremes of the pixels of its fragments (rc_fragment_key true), taken before the depth comparison.
struct RcBounds {
    int32_t x0, y0, x1, y1;                       // empty when x0 > x1
};

RC_HD void rc_bounds_empty(RcBounds* b) { b->x0 = INT32_MAX; b->y0 = INT32_MAX; b->x1 = INT32_MIN; b->y1 = INT32_MIN; }

RC_HD void rc_bounds_add(RcBounds* b, int32_t px, int32_t py) {
    b->x0 = px < b->x0 ? px : b->x0; b->y0 = py < b->y0 ? py : b->y0;
    b->x1 = px > b->x1 ? px : b->x1; b->y1 = py > b->y1 ? py : b->y1;
}

// bounds -> (x, y, w, h), visible; a draw that covers no pixel gets box 0 and flag 0
RC_HD void rc_bounds_box(const RcBounds& b, int32_t W, int32_t H, int32_t* bb, int32_t* visible) {
    if (b.x0 > b.x1) {
        bb[0] = bb[1] = bb[2] = bb[3] = 0;
        *visible = 0;
    } else {
        rc_bbox(b.x0, b.y0, b.x1, b.y1, W, H, bb);
        *visible = 1;
    }
}

// ---- overlay ---------------------------------------------------------------------------------------------------------------
// One byte of visualization/render_pose.py:44-46: image_show[bgr > 0] = g_y[bgr > 0]*2./3. + image_show[bgr > 0]*1./3. assigned
// into a uint8 array; g_y holds the render's `channel` and 0 elsewhere.  NumPy's float64 operations in NumPy's order, then the
// truncating cast.
RC_HD uint8_t rc_overlay(uint8_t render, uint8_t image, bool in_channel) {
    if (render == 0) return image;
    const double g = in_channel ? (double)render : 0.0;
    return (uint8_t)(g * 2. / 3. + (double)image * 1. / 3.);
}

}  // namespace aae_render
