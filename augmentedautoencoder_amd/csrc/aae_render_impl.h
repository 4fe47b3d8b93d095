// Host side of the mesh rasteriser: the mesh handle, the workspace layout and the launch sequence behind aae_render_*
// (include/aae_hip.h).  Part of aae_render.hip.
#pragma once

#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/aae_hip.h"
#include "kernels/render_raster.h"
#include "kernels/render_scene.h"
#include "kernels/render_train.h"

namespace aae_host {
void set_last_error(const char* msg);          // aae_host_types.h: the thread's aae_last_error() text lives in aae_hip.hip
}

struct aae_mesh {
    float* verts = nullptr;
    float* normals = nullptr;
    float* colors = nullptr;
    int32_t* faces = nullptr;
    int V = 0, F = 0, model = 0;
};

struct aae_mesh_set {
    aae_render::SceneMesh* table = nullptr;        // device, [n]: written once by aae_mesh_set_create
    int n = 0, Vmax = 0, Fmax = 0, model = 0;
};

namespace aae_render {

static int rfail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    aae_host::set_last_error(buf);
    return code;
}

#define AAE_RENDER_TRY(expr)                                                                                            \
    do {                                                                                                                \
        hipError_t e__ = (expr);                                                                                        \
        if (e__ != hipSuccess)                                                                                          \
            return aae_render::rfail(AAE_ERR_RUNTIME, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e__), __FILE__, __LINE__); \
    } while (0)

#define AAE_RENDER_OK(call) do { if (int rc__ = (call)) return rc__; } while (0)

// the two model kinds of a kernel template: kernel<true> for AAE_MODEL_CAD, kernel<false> otherwise
#define AAE_LAUNCH_KIND(cad, kernel, ...) do { if (cad) AAE_LAUNCH(kernel<true>, __VA_ARGS__); else AAE_LAUNCH(kernel<false>, __VA_ARGS__); } while (0)

// The events of a timed call: seven marks around six launches, then one synchronise on the last.  An untimed call creates no
// event and records nothing.  The destructor is the only place that destroys events, so no return between begin and finish leaks one.
struct StageTimer {
    hipEvent_t ev[7] = {};
    int made = 0, stage = 0;
    bool timed = false;

    int begin(bool timed_) {
        timed = timed_;
        for (int i = 0; timed && i < 7; ++i, ++made) AAE_RENDER_TRY(hipEventCreate(&ev[i]));
        return AAE_OK;
    }
    int mark(hipStream_t stream) {
        if (timed) AAE_RENDER_TRY(hipEventRecord(ev[stage++], stream));
        return AAE_OK;
    }
    // after the last mark; kernel_ms: 6 floats when timed
    int finish(float* kernel_ms) {
        AAE_RENDER_TRY(hipGetLastError());
        if (timed) {
            AAE_RENDER_TRY(hipEventSynchronize(ev[6]));
            for (int i = 0; i < 6; ++i) AAE_RENDER_TRY(hipEventElapsedTime(&kernel_ms[i], ev[i], ev[i + 1]));
        }
        return AAE_OK;
    }
    ~StageTimer() { for (int i = 0; i < made; ++i) (void)hipEventDestroy(ev[i]); }
};

static inline size_t up256(size_t v) { return (v + 255) / 256 * 256; }

struct WsLayout {
    size_t rect, vtx, vary, keys, total;
};

static WsLayout ws_layout(int V, int n, int W, int H, int n_vary = RC_VARY) {
    WsLayout l;
    size_t o = 0;
    l.rect = o; o += up256((size_t)n * 4 * sizeof(int32_t));
    l.vtx = o;  o += up256((size_t)n * V * sizeof(RcVertex));
    l.vary = o; o += up256((size_t)n * V * n_vary * sizeof(float));
    l.keys = o; o += up256((size_t)n * W * H * sizeof(unsigned long long));
    l.total = o;
    return l;
}

#define AAE_RENDER_MAX_DIM 4096
#define AAE_RENDER_MAX_VIEWS 65535           /* the view is blockIdx.y */

// frame size, K and the clip planes, in this order
static int check_camera(const aae_render_params* p, const char* who) {
    if (p->W < 1 || p->H < 1 || p->W > AAE_RENDER_MAX_DIM || p->H > AAE_RENDER_MAX_DIM)
        return rfail(AAE_ERR_UNSUPPORTED, "%s: render dims %dx%d outside [1,%d]", who, p->W, p->H, AAE_RENDER_MAX_DIM);
    if (p->K[3] != 0.0 || p->K[6] != 0.0 || p->K[7] != 0.0)
        return rfail(AAE_ERR_INVALID, "%s: K[1,0], K[2,0] and K[2,1] must be 0", who);
    if (!(p->clip_near > 0.0) || !(p->clip_far > p->clip_near)) return rfail(AAE_ERR_INVALID, "%s: need 0 < near < far", who);
    return AAE_OK;
}

static int check_workspace(const void* ws, size_t ws_bytes, size_t need, const char* who) {
    if (ws_bytes < need) return rfail(AAE_ERR_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", who, ws_bytes, need);
    if (((uintptr_t)ws & 255) != 0) return rfail(AAE_ERR_WORKSPACE, "%s: workspace must be 256-byte aligned", who);
    return AAE_OK;
}

// the checks every batch-of-views call makes after its null checks, in this order; crop: nullptr when the call cuts no patches
static int check_views(int n, const aae_render_params* p, const int* crop, const WsLayout& l, const void* ws, size_t ws_bytes, const char* who) {
    if (n < 1 || n > AAE_RENDER_MAX_VIEWS) return rfail(AAE_ERR_UNSUPPORTED, "%s: %d views outside [1,%d] per call", who, n, AAE_RENDER_MAX_VIEWS);
    AAE_RENDER_OK(check_camera(p, who));
    if (crop && (*crop < 1 || *crop > AAE_RENDER_MAX_DIM)) return rfail(AAE_ERR_UNSUPPORTED, "%s: crop size %d outside [1,%d]", who, *crop, AAE_RENDER_MAX_DIM);
    return check_workspace(ws, ws_bytes, l.total, who);
}

static void fill_camera_light(const aae_render_params* p, RcCamera* cam, RcLight* light) {
    cam->K00 = p->K[0]; cam->K01 = p->K[1]; cam->K02 = p->K[2]; cam->K11 = p->K[4]; cam->K12 = p->K[5];
    cam->near_ = p->clip_near; cam->far_ = p->clip_far;
    cam->W = p->W; cam->H = p->H;
    light->pos[0] = p->light[0]; light->pos[1] = p->light[1]; light->pos[2] = p->light[2];
    light->ambient = p->ambient; light->diffuse = p->diffuse; light->specular = p->specular;
}

static RenderArgs render_args(const aae_mesh* m, const double* Rs, const double* ts, int n, const aae_render_params* p, const WsLayout& l, void* ws) {
    char* base = (char*)ws;
    RenderArgs a;
    a.verts = m->verts; a.normals = m->normals; a.colors = m->colors; a.faces = m->faces;
    a.V = m->V; a.F = m->F;
    a.Rs = Rs; a.ts = ts;
    a.t[0] = p->t[0]; a.t[1] = p->t[1]; a.t[2] = p->t[2];
    fill_camera_light(p, &a.cam, &a.light);
    a.n = n;
    a.rect = (int32_t*)(base + l.rect);
    a.vtx = (RcVertex*)(base + l.vtx);
    a.vary = (float*)(base + l.vary);
    a.keys = (unsigned long long*)(base + l.keys);
    return a;
}

// The six launches of a batch of views of one mesh.  vertex(grid, block) launches the vertex form and final_stage(block) the last
// kernel (crops, frames or training pairs); the four launches between and around them are the same for every call.
// kernel_ms: nullptr, or 6 floats (the timed variant: events around every launch, then a synchronise)
template <class Vertex, class Final>
static int views_run(const RenderArgs& a, int32_t* bbs_out, int32_t* visible_out, hipStream_t stream, float* kernel_ms, Vertex vertex,
                     Final final_stage) {
    StageTimer tm;
    AAE_RENDER_OK(tm.begin(kernel_ms != nullptr));
    const dim3 block(RENDER_BLOCK);
    AAE_RENDER_OK(tm.mark(stream));
    AAE_LAUNCH(render_init_rect, dim3((a.n + RENDER_BLOCK - 1) / RENDER_BLOCK), block, 0, stream, a);
    AAE_RENDER_OK(tm.mark(stream));
    vertex(dim3((a.V + RENDER_BLOCK - 1) / RENDER_BLOCK, a.n), block);
    AAE_RENDER_OK(tm.mark(stream));
    AAE_LAUNCH(render_clear, dim3(RENDER_CLEAR_BLOCKS, a.n), block, 0, stream, a);
    AAE_RENDER_OK(tm.mark(stream));
    AAE_LAUNCH(render_raster, dim3((a.F + RENDER_BLOCK - 1) / RENDER_BLOCK, a.n), block, 0, stream, a);
    AAE_RENDER_OK(tm.mark(stream));
    AAE_LAUNCH(render_bbox, dim3(a.n), block, 0, stream, a, bbs_out, visible_out);
    AAE_RENDER_OK(tm.mark(stream));
    final_stage(block);
    AAE_RENDER_OK(tm.mark(stream));
    return tm.finish(kernel_ms);
}

// embedding crops (crops_out) or full frames (bgr_out, depth_out, tri_out)
static int render_run(const aae_mesh* m, const double* Rs, const double* ts, int n, const aae_render_params* p, int crop,
                      void* crops_out, void* bgr_out, float* depth_out, int32_t* tri_out, int32_t* bbs_out, int32_t* visible_out, void* ws, size_t ws_bytes,
                      void* stream_, float* kernel_ms, const char* who) {
    if (!m || !Rs || !p || !bbs_out || !visible_out || !ws) return rfail(AAE_ERR_INVALID, "%s: null argument", who);
    const WsLayout l = ws_layout(m->V, n, p->W, p->H);
    AAE_RENDER_OK(check_views(n, p, crops_out ? &crop : nullptr, l, ws, ws_bytes, who));

    hipStream_t stream = (hipStream_t)stream_;
    const RenderArgs a = render_args(m, Rs, ts, n, p, l, ws);
    const bool cad = m->model == AAE_MODEL_CAD;
    return views_run(
        a, bbs_out, visible_out, stream, kernel_ms,
        [&](dim3 grid, dim3 block) { AAE_LAUNCH_KIND(cad, render_vertex, grid, block, 0, stream, a); },
        [&](dim3 block) {
            if (crops_out)
                AAE_LAUNCH_KIND(cad, render_crop, dim3((crop * crop + RENDER_BLOCK - 1) / RENDER_BLOCK, n), block, 0, stream, a, (const int32_t*)bbs_out,
                                (const int32_t*)visible_out, p->pad_factor, crop, (uint8_t*)crops_out);
            else
                AAE_LAUNCH_KIND(cad, render_frame, dim3((p->W * p->H + RENDER_BLOCK - 1) / RENDER_BLOCK, n), block, 0, stream, a, (uint8_t*)bgr_out, depth_out,
                                tri_out);
        });
}

// a batch of training pairs: the launches of a batch of views with the training forms of the vertex stage and the crop
static int train_run(const aae_mesh* m, const double* Rs, const float* lights, const double* offsets, int n, const aae_render_params* p, int crop,
                     void* train_x, void* mask_x, void* train_y, int32_t* bbs_out, int32_t* visible_out, void* ws, size_t ws_bytes, void* stream_,
                     float* kernel_ms, const char* who) {
    if (!m || !Rs || !lights || !offsets || !p || !train_x || !mask_x || !train_y || !bbs_out || !visible_out || !ws)
        return rfail(AAE_ERR_INVALID, "%s: null argument", who);
    const WsLayout l = ws_layout(m->V, n, p->W, p->H, RC_VARY_TRAIN);
    AAE_RENDER_OK(check_views(n, p, &crop, l, ws, ws_bytes, who));

    hipStream_t stream = (hipStream_t)stream_;
    const RenderArgs a = render_args(m, Rs, nullptr, n, p, l, ws);
    TrainArgs ta;
    ta.lights = lights; ta.offsets = offsets;
    const bool cad = m->model == AAE_MODEL_CAD;
    return views_run(
        a, bbs_out, visible_out, stream, kernel_ms,
        [&](dim3 grid, dim3 block) { AAE_LAUNCH_KIND(cad, render_vertex_train, grid, block, 0, stream, a, ta); },
        [&](dim3 block) {
            AAE_LAUNCH_KIND(cad, render_train_crop, dim3((crop * crop + RENDER_BLOCK - 1) / RENDER_BLOCK, n), block, 0, stream, a, ta, (const int32_t*)bbs_out,
                            (const int32_t*)visible_out, p->pad_factor, crop, (uint8_t*)train_x, (uint8_t*)mask_x, (uint8_t*)train_y);
        });
}

struct SceneLayout {
    size_t rect, bounds, draw_obj, vtx, vary, keys, total;
};

static inline int scene_raster_blocks(int Fmax) { return (Fmax + RENDER_BLOCK - 1) / RENDER_BLOCK; }

static SceneLayout scene_layout(int Vmax, int Fmax, int n_draws, int n_scenes, int W, int H) {
    SceneLayout l;
    size_t o = 0;
    l.rect = o;     o += up256((size_t)n_scenes * 4 * sizeof(int32_t));
    l.bounds = o;   o += up256((size_t)n_draws * scene_raster_blocks(Fmax) * 4 * sizeof(int32_t));
    l.draw_obj = o; o += up256((size_t)n_draws * sizeof(int32_t));
    l.vtx = o;      o += up256((size_t)n_draws * Vmax * sizeof(RcVertex));
    l.vary = o;     o += up256((size_t)n_draws * Vmax * RC_VARY * sizeof(float));
    l.keys = o;     o += up256((size_t)n_scenes * W * H * sizeof(unsigned long long));
    l.total = o;
    return l;
}

#define AAE_SCENE_MAX_SCENES 65535           /* the scene is blockIdx.y, and a uint16 in the draw table */
#define AAE_SCENE_MAX_MESHES 65536           /* the mesh is a uint16 in the draw table */

// kernel_ms: nullptr, or 6 floats (the timed variant: events around every launch, then a synchronise)
static int scene_run(const aae_mesh_set* set, const int32_t* obj_ids, const int32_t* scene_ids, const double* Rs, const double* ts, int n_draws,
                     int n_scenes, const aae_render_params* p, void* bgr_out, float* depth_out, int32_t* draw_out, int32_t* tri_out, int32_t* bbs_out,
                     int32_t* visible_out, void* ws, size_t ws_bytes, void* stream_, float* kernel_ms, const char* who) {
    if (!set || !obj_ids || !scene_ids || !Rs || !ts || !p || !bgr_out || !depth_out || !bbs_out || !visible_out || !ws)
        return rfail(AAE_ERR_INVALID, "%s: null argument", who);
    if (n_draws < 1 || n_draws > AAE_SCENE_MAX_DRAWS)
        return rfail(AAE_ERR_UNSUPPORTED, "%s: %d draws outside [1,%d] per call (split by scene)", who, n_draws, AAE_SCENE_MAX_DRAWS);
    if (n_scenes < 1 || n_scenes > AAE_SCENE_MAX_SCENES)
        return rfail(AAE_ERR_UNSUPPORTED, "%s: %d scenes outside [1,%d] per call", who, n_scenes, AAE_SCENE_MAX_SCENES);
    if (!rc_scene_fits((uint64_t)n_draws, (uint64_t)set->Fmax))
        return rfail(AAE_ERR_UNSUPPORTED, "%s: %d draws of up to %d faces do not fit the 32-bit index of the visibility key", who, n_draws, set->Fmax);
    AAE_RENDER_OK(check_camera(p, who));
    SceneArgs a;
    memset(&a.draws, 0, sizeof(a.draws));
    for (int d = 0; d < n_draws; ++d) {
        if (obj_ids[d] < 0 || obj_ids[d] >= set->n)
            return rfail(AAE_ERR_INVALID, "%s: draw %d names mesh %d of a set of %d", who, d, obj_ids[d], set->n);
        if (scene_ids[d] < 0 || scene_ids[d] >= n_scenes)
            return rfail(AAE_ERR_INVALID, "%s: draw %d names scene %d of %d", who, d, scene_ids[d], n_scenes);
        a.draws.obj[d] = (uint16_t)obj_ids[d];
        a.draws.scene[d] = (uint16_t)scene_ids[d];
    }
    const SceneLayout l = scene_layout(set->Vmax, set->Fmax, n_draws, n_scenes, p->W, p->H);
    AAE_RENDER_OK(check_workspace(ws, ws_bytes, l.total, who));

    hipStream_t stream = (hipStream_t)stream_;
    char* base = (char*)ws;
    a.meshes = set->table;
    a.Vmax = set->Vmax; a.Fmax = set->Fmax;
    a.Rs = Rs; a.ts = ts;
    fill_camera_light(p, &a.cam, &a.light);
    a.n_draws = n_draws; a.n_scenes = n_scenes;
    a.rect = (int32_t*)(base + l.rect);
    a.bounds = (int32_t*)(base + l.bounds);
    a.raster_blocks = scene_raster_blocks(set->Fmax);
    a.draw_obj = (int32_t*)(base + l.draw_obj);
    a.vtx = (RcVertex*)(base + l.vtx);
    a.vary = (float*)(base + l.vary);
    a.keys = (unsigned long long*)(base + l.keys);

    StageTimer tm;
    AAE_RENDER_OK(tm.begin(kernel_ms != nullptr));
    const bool cad = set->model == AAE_MODEL_CAD;
    const dim3 block(RENDER_BLOCK);
    const int n_init = n_draws > n_scenes ? n_draws : n_scenes;
    AAE_RENDER_OK(tm.mark(stream));
    AAE_LAUNCH(scene_init, dim3((n_init + RENDER_BLOCK - 1) / RENDER_BLOCK), block, 0, stream, a);
    AAE_RENDER_OK(tm.mark(stream));
    AAE_LAUNCH_KIND(cad, scene_vertex, dim3((set->Vmax + RENDER_BLOCK - 1) / RENDER_BLOCK, n_draws), block, 0, stream, a);
    AAE_RENDER_OK(tm.mark(stream));
    AAE_LAUNCH(scene_clear, dim3(RENDER_CLEAR_BLOCKS, n_scenes), block, 0, stream, a);
    AAE_RENDER_OK(tm.mark(stream));
    AAE_LAUNCH(scene_raster, dim3(a.raster_blocks, n_draws), block, 0, stream, a);
    AAE_RENDER_OK(tm.mark(stream));
    AAE_LAUNCH(scene_bbox, dim3(n_draws), dim3(64), 0, stream, a, bbs_out, visible_out);
    AAE_RENDER_OK(tm.mark(stream));
    AAE_LAUNCH_KIND(cad, scene_frame, dim3((p->W * p->H + RENDER_BLOCK - 1) / RENDER_BLOCK, n_scenes), block, 0, stream, a, (uint8_t*)bgr_out, depth_out,
                    draw_out, tri_out);
    AAE_RENDER_OK(tm.mark(stream));
    return tm.finish(kernel_ms);
}

}  // namespace aae_render

extern "C" {

int aae_mesh_create(const float* verts, const float* normals, const float* colors, int n_verts, const int32_t* faces, int n_faces,
                    int model, float vertex_scale, aae_mesh** out) {
    using namespace aae_render;
    if (!verts || !normals || !faces || !out) return rfail(AAE_ERR_INVALID, "aae_mesh_create: null argument");
    if (n_verts < 1 || n_faces < 1) return rfail(AAE_ERR_INVALID, "aae_mesh_create: %d vertices, %d faces", n_verts, n_faces);
    if (model != AAE_MODEL_RECONST && model != AAE_MODEL_CAD) return rfail(AAE_ERR_UNSUPPORTED, "aae_mesh_create: unknown model kind %d", model);
    for (size_t i = 0; i < (size_t)n_faces * 3; ++i)
        if (faces[i] < 0 || faces[i] >= n_verts)
            return rfail(AAE_ERR_INVALID, "aae_mesh_create: face %zu names vertex %d of %d", i / 3, faces[i], n_verts);
    const size_t nv3 = (size_t)n_verts * 3;
    std::vector<float> scaled(nv3), col(nv3);
    for (size_t i = 0; i < nv3; ++i) {
        scaled[i] = verts[i] * vertex_scale;                                  // meshrenderer_phong.py:52-55: float32
        col[i] = colors ? colors[i] : 160.0f / 255.0f;                         // meshrenderer_phong.py:50
    }
    aae_mesh* m = new aae_mesh();
    m->V = n_verts; m->F = n_faces; m->model = model;
    hipError_t e = hipMalloc((void**)&m->verts, nv3 * sizeof(float));
    if (e == hipSuccess) e = hipMalloc((void**)&m->normals, nv3 * sizeof(float));
    if (e == hipSuccess) e = hipMalloc((void**)&m->colors, nv3 * sizeof(float));
    if (e == hipSuccess) e = hipMalloc((void**)&m->faces, (size_t)n_faces * 3 * sizeof(int32_t));
    if (e == hipSuccess) e = hipMemcpy(m->verts, scaled.data(), nv3 * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(m->normals, normals, nv3 * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(m->colors, col.data(), nv3 * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(m->faces, faces, (size_t)n_faces * 3 * sizeof(int32_t), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        aae_mesh_destroy(m);
        return rfail(AAE_ERR_RUNTIME, "aae_mesh_create: %s", hipGetErrorString(e));
    }
    *out = m;
    return AAE_OK;
}

void aae_mesh_destroy(aae_mesh* m) {
    if (!m) return;
    if (m->verts) (void)hipFree(m->verts);
    if (m->normals) (void)hipFree(m->normals);
    if (m->colors) (void)hipFree(m->colors);
    if (m->faces) (void)hipFree(m->faces);
    delete m;
}

size_t aae_render_workspace_bytes(const aae_mesh* mesh, int n_views, int W, int H) {
    if (!mesh || n_views < 1 || W < 1 || H < 1) return 0;
    return aae_render::ws_layout(mesh->V, n_views, W, H).total;
}

int aae_render_embedding_views(const aae_mesh* mesh, const double* Rs, int n, const aae_render_params* params, int crop,
                               void* crops_out, int32_t* bbs_out, int32_t* visible_out, void* workspace, size_t ws_bytes, void* stream) {
    if (!crops_out) return aae_render::rfail(AAE_ERR_INVALID, "aae_render_embedding_views: null argument");
    return aae_render::render_run(mesh, Rs, nullptr, n, params, crop, crops_out, nullptr, nullptr, nullptr, bbs_out, visible_out, workspace, ws_bytes,
                                  stream, nullptr, "aae_render_embedding_views");
}

int aae_render_embedding_views_timed(const aae_mesh* mesh, const double* Rs, int n, const aae_render_params* params, int crop,
                                     void* crops_out, int32_t* bbs_out, int32_t* visible_out, void* workspace, size_t ws_bytes,
                                     void* stream, float* kernel_ms) {
    if (!crops_out || !kernel_ms) return aae_render::rfail(AAE_ERR_INVALID, "aae_render_embedding_views_timed: null argument");
    return aae_render::render_run(mesh, Rs, nullptr, n, params, crop, crops_out, nullptr, nullptr, nullptr, bbs_out, visible_out, workspace, ws_bytes,
                                  stream, kernel_ms, "aae_render_embedding_views_timed");
}

int aae_render_frames(const aae_mesh* mesh, const double* Rs, const double* ts, int n, const aae_render_params* params,
                      void* bgr_out, float* depth_out, int32_t* tri_out, int32_t* bbs_out, int32_t* visible_out, void* workspace,
                      size_t ws_bytes, void* stream) {
    if (!bgr_out || !depth_out) return aae_render::rfail(AAE_ERR_INVALID, "aae_render_frames: null argument");
    return aae_render::render_run(mesh, Rs, ts, n, params, 0, nullptr, bgr_out, depth_out, tri_out, bbs_out, visible_out, workspace, ws_bytes,
                                  stream, nullptr, "aae_render_frames");
}

size_t aae_render_training_workspace_bytes(const aae_mesh* mesh, int n_views, int W, int H) {
    if (!mesh || n_views < 1 || W < 1 || H < 1) return 0;
    return aae_render::ws_layout(mesh->V, n_views, W, H, RC_VARY_TRAIN).total;
}

int aae_render_training_views(const aae_mesh* mesh, const double* Rs, const float* lights, const double* offsets, int n,
                              const aae_render_params* params, int crop, void* train_x, void* mask_x, void* train_y, int32_t* bbs_out,
                              int32_t* visible_out, void* workspace, size_t ws_bytes, void* stream) {
    return aae_render::train_run(mesh, Rs, lights, offsets, n, params, crop, train_x, mask_x, train_y, bbs_out, visible_out, workspace, ws_bytes,
                                 stream, nullptr, "aae_render_training_views");
}

int aae_render_training_views_timed(const aae_mesh* mesh, const double* Rs, const float* lights, const double* offsets, int n,
                                    const aae_render_params* params, int crop, void* train_x, void* mask_x, void* train_y, int32_t* bbs_out,
                                    int32_t* visible_out, void* workspace, size_t ws_bytes, void* stream, float* kernel_ms) {
    if (!kernel_ms) return aae_render::rfail(AAE_ERR_INVALID, "aae_render_training_views_timed: null argument");
    return aae_render::train_run(mesh, Rs, lights, offsets, n, params, crop, train_x, mask_x, train_y, bbs_out, visible_out, workspace, ws_bytes,
                                 stream, kernel_ms, "aae_render_training_views_timed");
}

int aae_mesh_set_create(const aae_mesh* const* meshes, int n_meshes, aae_mesh_set** out) {
    using namespace aae_render;
    if (!meshes || !out) return rfail(AAE_ERR_INVALID, "aae_mesh_set_create: null argument");
    if (n_meshes < 1 || n_meshes > AAE_SCENE_MAX_MESHES)
        return rfail(AAE_ERR_UNSUPPORTED, "aae_mesh_set_create: %d meshes outside [1,%d]", n_meshes, AAE_SCENE_MAX_MESHES);
    std::vector<SceneMesh> rows((size_t)n_meshes);
    aae_mesh_set* set = new aae_mesh_set();
    set->n = n_meshes;
    for (int i = 0; i < n_meshes; ++i) {
        const aae_mesh* m = meshes[i];
        if (!m) {
            delete set;
            return rfail(AAE_ERR_INVALID, "aae_mesh_set_create: mesh %d is null", i);
        }
        if (i == 0) set->model = m->model;
        if (m->model != set->model) {
            delete set;
            return rfail(AAE_ERR_UNSUPPORTED, "aae_mesh_set_create: mesh %d is of model kind %d, mesh 0 of kind %d (one kind per set)", i, m->model, set->model);
        }
        rows[i].verts = m->verts; rows[i].normals = m->normals; rows[i].colors = m->colors; rows[i].faces = m->faces;
        rows[i].V = m->V; rows[i].F = m->F;
        set->Vmax = m->V > set->Vmax ? m->V : set->Vmax;
        set->Fmax = m->F > set->Fmax ? m->F : set->Fmax;
    }
    hipError_t e = hipMalloc((void**)&set->table, rows.size() * sizeof(SceneMesh));
    if (e == hipSuccess) e = hipMemcpy(set->table, rows.data(), rows.size() * sizeof(SceneMesh), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        aae_mesh_set_destroy(set);
        return rfail(AAE_ERR_RUNTIME, "aae_mesh_set_create: %s", hipGetErrorString(e));
    }
    *out = set;
    return AAE_OK;
}

void aae_mesh_set_destroy(aae_mesh_set* set) {
    if (!set) return;
    if (set->table) (void)hipFree(set->table);
    delete set;
}

size_t aae_render_scenes_workspace_bytes(const aae_mesh_set* set, int n_draws, int n_scenes, int W, int H) {
    if (!set || n_draws < 1 || n_scenes < 1 || W < 1 || H < 1) return 0;
    return aae_render::scene_layout(set->Vmax, set->Fmax, n_draws, n_scenes, W, H).total;
}

int aae_render_scenes(const aae_mesh_set* set, const int32_t* obj_ids, const int32_t* scene_ids, const double* Rs, const double* ts,
                      int n_draws, int n_scenes, const aae_render_params* params, void* bgr_out, float* depth_out,
                      int32_t* draw_out, int32_t* tri_out, int32_t* bbs_out, int32_t* visible_out,
                      void* workspace, size_t ws_bytes, void* stream) {
    return aae_render::scene_run(set, obj_ids, scene_ids, Rs, ts, n_draws, n_scenes, params, bgr_out, depth_out, draw_out, tri_out, bbs_out,
                                 visible_out, workspace, ws_bytes, stream, nullptr, "aae_render_scenes");
}

int aae_render_scenes_timed(const aae_mesh_set* set, const int32_t* obj_ids, const int32_t* scene_ids, const double* Rs, const double* ts,
                            int n_draws, int n_scenes, const aae_render_params* params, void* bgr_out, float* depth_out,
                            int32_t* draw_out, int32_t* tri_out, int32_t* bbs_out, int32_t* visible_out,
                            void* workspace, size_t ws_bytes, void* stream, float* kernel_ms) {
    if (!kernel_ms) return aae_render::rfail(AAE_ERR_INVALID, "aae_render_scenes_timed: null argument");
    return aae_render::scene_run(set, obj_ids, scene_ids, Rs, ts, n_draws, n_scenes, params, bgr_out, depth_out, draw_out, tri_out, bbs_out,
                                 visible_out, workspace, ws_bytes, stream, kernel_ms, "aae_render_scenes_timed");
}

int aae_overlay_blend(const void* image, const void* render, size_t n_pixels, int channel, void* out, void* stream) {
    using namespace aae_render;
    if (!image || !render || !out) return rfail(AAE_ERR_INVALID, "aae_overlay_blend: null argument");
    if (channel < 0 || channel > 2) return rfail(AAE_ERR_INVALID, "aae_overlay_blend: channel %d outside [0,2]", channel);
    if (n_pixels == 0) return AAE_OK;
    const size_t n_bytes = n_pixels * 3;
    const size_t blocks = (n_bytes + RENDER_BLOCK - 1) / RENDER_BLOCK;
    if (blocks > 0x7FFFFFFFull) return rfail(AAE_ERR_UNSUPPORTED, "aae_overlay_blend: %zu pixels are too many for one launch", n_pixels);
    AAE_LAUNCH(overlay_blend, dim3((unsigned)blocks), dim3(RENDER_BLOCK), 0, (hipStream_t)stream, (const uint8_t*)image, (const uint8_t*)render,
               n_bytes, channel, (uint8_t*)out);
    AAE_RENDER_TRY(hipGetLastError());
    return AAE_OK;
}

}  // extern "C"
