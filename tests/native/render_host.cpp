// Host driver of csrc/kernels/render_core.h: the stages of the rasteriser as serial loops in place of the launches of
// render_raster.h (same order, same screen-rectangle bookkeeping, a workspace that starts full of 0xA5), reading a scene file
// and writing frames, depth, winning triangle, boxes and crops.  Built and run by tests/test_render_cpu.py (also with
// -fsanitize=address,undefined: this is the sanitizer run of the rasteriser's arithmetic).
//
// scene file (little endian): int32 V, F, model, n, W, H, crop, has_ts; float64 K[9], t[3], near, far, pad_factor;
//   float32 light[3], ambient, diffuse, specular; float32 verts[V*3], normals[V*3], colors[V*3]; int32 faces[F*3];
//   float64 Rs[n*9]; float64 ts[n*3] when has_ts.
// output file, per view: uint8 bgr[H*W*3]; float32 depth[H*W]; int32 tri[H*W]; int32 bb[4]; int32 visible;
//   uint8 crop[crop*crop*3] when crop > 0.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../augmentedautoencoder_amd/csrc/kernels/render_core.h"

using namespace aae_render;

template <typename T>
static void rd(FILE* f, T* p, size_t n) {
    if (n && fread(p, sizeof(T), n, f) != n) {
        fprintf(stderr, "render_host: short scene file\n");
        exit(2);
    }
}

template <bool CAD>
static int run(FILE* in, FILE* out, const int32_t* hd) {
    const int V = hd[0], F = hd[1], n = hd[3], W = hd[4], H = hd[5], crop = hd[6], has_ts = hd[7];
    double K[9], t0[3], nfp[3];
    float lt[6];
    rd(in, K, 9); rd(in, t0, 3); rd(in, nfp, 3); rd(in, lt, 6);
    std::vector<float> verts((size_t)V * 3), normals((size_t)V * 3), colors((size_t)V * 3);
    std::vector<int32_t> faces((size_t)F * 3);
    std::vector<double> Rs((size_t)n * 9), ts((size_t)n * 3);
    rd(in, verts.data(), verts.size()); rd(in, normals.data(), normals.size()); rd(in, colors.data(), colors.size());
    rd(in, faces.data(), faces.size()); rd(in, Rs.data(), Rs.size());
    if (has_ts) rd(in, ts.data(), ts.size());
    for (int32_t i : faces)
        if (i < 0 || i >= V) return 3;
    RcCamera cam;
    cam.K00 = K[0]; cam.K01 = K[1]; cam.K02 = K[2]; cam.K11 = K[4]; cam.K12 = K[5];
    cam.near_ = nfp[0]; cam.far_ = nfp[1]; cam.W = W; cam.H = H;
    RcLight light;
    light.pos[0] = lt[0]; light.pos[1] = lt[1]; light.pos[2] = lt[2];
    light.ambient = lt[3]; light.diffuse = lt[4]; light.specular = lt[5];

    std::vector<RcVertex> vtx(V);
    std::vector<float> vary((size_t)V * RC_VARY);
    std::vector<uint64_t> keys((size_t)W * H);
    std::vector<uint8_t> bgr((size_t)W * H * 3), cr((size_t)crop * crop * 3);
    std::vector<float> depth((size_t)W * H);
    std::vector<int32_t> tri((size_t)W * H);
    for (int view = 0; view < n; ++view) {
        const double* R = &Rs[(size_t)view * 9];
        const double* t = has_ts ? &ts[(size_t)view * 3] : t0;
        for (auto& k : keys) k = 0xA5A5A5A5A5A5A5A5ull;
        // vertex stage + screen rectangle
        int rx0 = INT32_MAX, ry0 = INT32_MAX, rx1 = INT32_MIN, ry1 = INT32_MIN;
        for (int i = 0; i < V; ++i) {
            rc_vertex<CAD>(R, t, cam, light, &verts[(size_t)i * 3], &normals[(size_t)i * 3], &vtx[i], &vary[(size_t)i * RC_VARY]);
            if (vtx[i].x == RC_INVALID) continue;
            const int a0 = rc_clampi(rc_pixel_lo(vtx[i].x), 0, W - 1), a1 = rc_clampi(rc_pixel_hi(vtx[i].x), 0, W - 1);
            const int b0 = rc_clampi(rc_pixel_lo(vtx[i].y), 0, H - 1), b1 = rc_clampi(rc_pixel_hi(vtx[i].y), 0, H - 1);
            rx0 = a0 < rx0 ? a0 : rx0; rx1 = a1 > rx1 ? a1 : rx1; ry0 = b0 < ry0 ? b0 : ry0; ry1 = b1 > ry1 ? b1 : ry1;
        }
        const bool have = rx0 <= rx1 && ry0 <= ry1 && rx0 != INT32_MAX;
        // clear
        if (have)
            for (int y = ry0; y <= ry1; ++y)
                for (int x = rx0; x <= rx1; ++x) keys[(size_t)y * W + x] = RC_BACKGROUND;
        // raster
        for (int f = 0; f < F; ++f) {
            RcTri T;
            rc_tri_setup(vtx[faces[(size_t)f * 3]], vtx[faces[(size_t)f * 3 + 1]], vtx[faces[(size_t)f * 3 + 2]], W, H, &T);
            if (!T.ok) continue;
            if (T.px0 < rx0 || T.px1 > rx1 || T.py0 < ry0 || T.py1 > ry1) return 4;          // a triangle outside the cleared rectangle
            for (int y = T.py0; y <= T.py1; ++y)
                for (int x = T.px0; x <= T.px1; ++x) {
                    uint64_t key;
                    if (rc_fragment_key(T, x, y, cam.far_, (uint32_t)f, &key) && key < keys[(size_t)y * W + x]) keys[(size_t)y * W + x] = key;
                }
        }
        // bbox
        int mnx = INT32_MAX, mny = INT32_MAX, mxx = INT32_MIN, mxy = INT32_MIN;
        if (have)
            for (int y = ry0; y <= ry1; ++y)
                for (int x = rx0; x <= rx1; ++x)
                    if (keys[(size_t)y * W + x] != RC_BACKGROUND) {
                        mnx = x < mnx ? x : mnx; mny = y < mny ? y : mny; mxx = x > mxx ? x : mxx; mxy = y > mxy ? y : mxy;
                    }
        int32_t bb[4] = {0, 0, 0, 0}, visible = 0;
        if (mnx != INT32_MAX) {
            rc_bbox(mnx, mny, mxx, mxy, W, H, bb);
            visible = 1;
        }
        // frame
        auto key_at = [&](int x, int y) -> uint64_t {
            if (!have || x < rx0 || x > rx1 || y < ry0 || y > ry1) return RC_BACKGROUND;
            return keys[(size_t)y * W + x];
        };
        auto shade = [&](uint64_t key, int x, int y, uint8_t* px) {
            px[0] = px[1] = px[2] = 0;
            if (key == RC_BACKGROUND) return;
            const int f = (int)(key & 0xFFFFFFFFull);
            const int32_t* fi = &faces[(size_t)f * 3];
            RcTri T;
            rc_tri_setup(vtx[fi[0]], vtx[fi[1]], vtx[fi[2]], W, H, &T);
            rc_shade<CAD>(T, x, y, &vary[(size_t)fi[0] * RC_VARY], &vary[(size_t)fi[1] * RC_VARY], &vary[(size_t)fi[2] * RC_VARY],
                          &colors[(size_t)fi[0] * 3], &colors[(size_t)fi[1] * 3], &colors[(size_t)fi[2] * 3], light, px);
        };
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) {
                const uint64_t key = key_at(x, y);
                shade(key, x, y, &bgr[((size_t)y * W + x) * 3]);
                depth[(size_t)y * W + x] = rc_key_depth(key);
                tri[(size_t)y * W + x] = key == RC_BACKGROUND ? -1 : (int32_t)(key & 0xFFFFFFFFull);
            }
        fwrite(bgr.data(), 1, bgr.size(), out);
        fwrite(depth.data(), 4, depth.size(), out);
        fwrite(tri.data(), 4, tri.size(), out);
        fwrite(bb, 4, 4, out);
        fwrite(&visible, 4, 1, out);
        // crop
        if (crop > 0) {
            for (auto& c : cr) c = 0;
            int32_t left, right, top, bottom;
            rc_crop_rect(bb, nfp[2], W, H, &left, &right, &top, &bottom);
            if (visible && right > left && bottom > top)
                for (int oy = 0; oy < crop; ++oy)
                    for (int ox = 0; ox < crop; ++ox) {
                        const int x = left + rc_nearest_src(ox, crop, right - left), y = top + rc_nearest_src(oy, crop, bottom - top);
                        shade(key_at(x, y), x, y, &cr[((size_t)oy * crop + ox) * 3]);
                    }
            fwrite(cr.data(), 1, cr.size(), out);
        }
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: render_host <scene.bin> <out.bin>\n");
        return 1;
    }
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) return 1;
    int32_t hd[8];
    rd(in, hd, 8);
    if (hd[0] < 1 || hd[1] < 1 || hd[3] < 1 || hd[4] < 1 || hd[5] < 1 || hd[6] < 0) return 1;
    const int rc = hd[2] == 1 ? run<true>(in, out, hd) : run<false>(in, out, hd);
    fclose(in);
    fclose(out);
    return rc;
}
