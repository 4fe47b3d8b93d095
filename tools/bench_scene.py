"""Several objects into one frame: the scene call next to the per-draw route, in one process:

    python tools/bench_scene.py [--iters 50] [--faces 51200] [--out profiles/r22_scene/bench_scene_run1.json]

The mesh and the camera are those of tools/bench_render.py (the ~50k-face bumpy torus; the template's K scaled to 640x480).
A frame holds 8 draws of it on a 4x2 grid at 900 / 1000 mm, each at its own rotation, neighbours overlapping.  Timed, for 1
scene and for 16 scenes (8 draws each, 128 draws a call):

  scene      one Renderer.render_scenes call (aae_render_scenes: six launches for all draws and frames);
  per_draw   what the single-mesh interface offers: one Renderer.render_batch per draw (the same draw of every scene in one batch)
             plus a torch.where depth merge and colour select per draw.

Wall time per call is the median over `iters` calls, each synchronised; the per-launch split comes from the events of
aae_render_scenes_timed, averaged over `iters` calls.  Both routes are checked to give the same depth.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

KERNELS = ('scene_init', 'scene_vertex', 'scene_clear', 'scene_raster', 'scene_bbox', 'scene_frame')
W, H = 640, 480
DRAWS = 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--faces', type=int, default=51200)
    ap.add_argument('--model', default='reconst', choices=['reconst', 'cad'])
    ap.add_argument('--out', default=None)
    args = ap.parse_args()

    import torch
    from bench_render import bumpy_torus
    from augmentedautoencoder_amd import viewsphere as vs
    from augmentedautoencoder_amd.meshrenderer import Renderer

    torch.cuda.set_device(0)
    nv = int(round((args.faces / 2 / 2) ** 0.5))
    model = bumpy_torus(2 * nv, nv)
    r = Renderer([model], model=args.model)
    s = W / 720.0
    K = np.array([1075.65 * s, 0, W / 2, 0, 1073.90 * s, H / 2, 0, 0, 1]).reshape(3, 3)
    Rs_all = vs.viewsphere_for_embedding(2562, 700.0, 36)

    def scene_poses(n_scenes):
        pick = np.linspace(0, len(Rs_all) - 1, n_scenes * DRAWS).astype(np.int64)
        Rs = Rs_all[pick].reshape(n_scenes, DRAWS, 3, 3)
        ts = np.zeros((n_scenes, DRAWS, 3))
        for d in range(DRAWS):
            z = 900.0 if d % 2 == 0 else 1000.0
            u, v = (d % 4 + 0.5) * W / 4, (d // 4 + 0.5) * H / 2
            ts[:, d] = [(u - K[0, 2]) * z / K[0, 0], (v - K[1, 2]) * z / K[1, 1], z]
        return Rs, ts

    def timed(fn, iters):
        fn()
        torch.cuda.synchronize()
        out = []
        for _ in range(iters):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            out.append(time.perf_counter() - t0)
        return float(np.median(out)) * 1e3, float(np.min(out)) * 1e3

    res = {'tool': 'bench_scene', 'model': args.model, 'faces': int(len(model['faces'])), 'vertices': int(len(r._arrays[0][0])),
           'render_dims': [W, H], 'draws_per_scene': DRAWS, 'iters': args.iters, 'cases': {}}
    for n_scenes in (1, 16):
        Rs, ts = scene_poses(n_scenes)
        obj = [0] * (n_scenes * DRAWS)
        scn = np.repeat(np.arange(n_scenes), DRAWS).tolist()
        Rd = torch.as_tensor(Rs.reshape(-1, 9), device='cuda')
        td = torch.as_tensor(ts.reshape(-1, 3), device='cuda')
        Rdraw = [torch.as_tensor(np.ascontiguousarray(Rs[:, d]).reshape(-1, 9), device='cuda') for d in range(DRAWS)]
        tdraw = [torch.as_tensor(np.ascontiguousarray(ts[:, d]), device='cuda') for d in range(DRAWS)]

        def scene():
            return r.render_scenes(obj, scn, n_scenes, W, H, K, Rd, td, 10., 10000.)

        def per_draw():
            bgr, depth, _, _ = r.render_batch(0, W, H, K, Rdraw[0], tdraw[0], 10., 10000.)
            for d in range(1, DRAWS):
                b, z, _, _ = r.render_batch(0, W, H, K, Rdraw[d], tdraw[d], 10., 10000.)
                nearer = (z > 0) & ((depth == 0) | (z < depth))
                depth = torch.where(nearer, z, depth)
                bgr = torch.where(nearer[..., None], b, bgr)
            return bgr, depth

        a, b = scene(), per_draw()
        assert torch.equal(a[1], b[1]) and torch.equal(a[0], b[0]) and int(a[3].min()) == 1, 'the two routes disagree'
        covered = float((a[1] > 0).float().mean())
        scene_ms, scene_min = timed(scene, args.iters)
        draw_ms, draw_min = timed(per_draw, args.iters)
        ms = np.zeros(6)
        for _ in range(args.iters):
            ms += np.array(r.render_scenes(obj, scn, n_scenes, W, H, K, Rd, td, 10., 10000., timed=True)[-1])
        ms /= args.iters
        res['cases']['%d_scenes' % n_scenes] = {
            'draws': n_scenes * DRAWS, 'covered_fraction': round(covered, 4),
            'scene_call_ms': round(scene_ms, 4), 'scene_call_ms_min': round(scene_min, 4), 'scene_ms_per_frame': round(scene_ms / n_scenes, 4),
            'per_draw_route_ms': round(draw_ms, 4), 'per_draw_route_ms_min': round(draw_min, 4), 'per_draw_ms_per_frame': round(draw_ms / n_scenes, 4),
            'per_draw_over_scene': round(draw_ms / scene_ms, 3),
            'launch_ms': {k: round(float(v), 4) for k, v in zip(KERNELS, ms)}, 'launch_ms_sum': round(float(ms.sum()), 4)}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')
    r.close()


if __name__ == '__main__':
    main()
