"""Throughput of the training-pair call next to what the single-light interface offers, in one process:

    python tools/bench_train_render.py [--pairs 4096] [--batch 256] [--route-pairs 256] [--out profiles/bench_train_render.json]

bench_render.py's bumpy torus at the template's settings (720x540, radius 700, 128x128 crops, PAD_FACTOR 1.2) and
MAX_REL_OFFSET 0.2; rotations, lights and offsets from draw_training_params under a fixed seed.  Three legs:

  (a) `pairs` training pairs through aae_render_training_views in batches of `batch`: wall clock and the per-launch split;
  (b) two render_embedding_views calls per batch over the same rotations -- the most the single-light interface can do: the
      wrong train_x (one light, no offset), the same amount of output;
  (c) on `route-pairs` pairs only, the one correct route of that interface: one render_batch per image for x with its light,
      one embedding batch for y, the patches and masks cut with torch on the device; checked byte for byte against (a).

Prints one JSON line: pairs/s of each leg and the time for 20 000 images including the copies to the host."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

KERNELS = ('render_init_rect', 'render_vertex_train', 'render_clear', 'render_raster', 'render_bbox', 'render_train_crop')
EMBED_KERNELS = ('render_init_rect', 'render_vertex', 'render_clear', 'render_raster', 'render_bbox', 'render_crop')


def torch_patch(img, bb, pad, size):
    """extract_square_patch + resizeNN of one device image [H,W,...] for a host box (float64, truncated as the reference does)"""
    import torch
    x, y, w, h = np.array(bb).astype(np.int32)
    s = int(np.maximum(h, w) * pad)
    left, right = int(np.maximum(x + w / 2 - s / 2, 0)), int(np.minimum(x + w / 2 + s / 2, img.shape[1]))
    top, bottom = int(np.maximum(y + h / 2 - s / 2, 0)), int(np.minimum(y + h / 2 + s / 2, img.shape[0]))
    cols = np.minimum(np.floor(np.arange(size) * (1.0 / (float(size) / (right - left)))).astype(np.int64), right - left - 1) + left
    rows = np.minimum(np.floor(np.arange(size) * (1.0 / (float(size) / (bottom - top)))).astype(np.int64), bottom - top - 1) + top
    return img[torch.as_tensor(rows, device=img.device)][:, torch.as_tensor(cols, device=img.device)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--pairs', type=int, default=4096)
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--route-pairs', type=int, default=256)
    ap.add_argument('--faces', type=int, default=51200)
    ap.add_argument('--model', default='reconst', choices=['reconst', 'cad'])
    ap.add_argument('--out', default=None)
    args = ap.parse_args()

    import torch
    from bench_render import bumpy_torus
    from augmentedautoencoder_amd.meshrenderer import Renderer, draw_training_params

    torch.cuda.set_device(0)
    nv = int(round((args.faces / 2 / 2) ** 0.5))
    model = bumpy_torus(2 * nv, nv)
    r = Renderer([model], model=args.model)
    np.random.seed(24)
    Rs_h, lights_h, offsets_h = draw_training_params(args.pairs, 0.2, args.model)
    Rs = torch.as_tensor(Rs_h.reshape(-1, 9), device='cuda')
    lights = torch.as_tensor(lights_h, device='cuda')
    offsets = torch.as_tensor(offsets_h, device='cuda')
    W, H, crop, pad = 720, 540, 128, 1.2
    K = np.array([1075.65, 0, 720 / 2, 0, 1073.90, 540 / 2, 0, 0, 1]).reshape(3, 3)
    t = np.array([0., 0., 700.])
    B = args.batch
    pair = lambda a, n=B, **kw: r.render_training_views(0, W, H, K, Rs[a:a + n], t, 10., 10000., pad, crop, lights[a:a + n], offsets[a:a + n], **kw)
    embed = lambda a, **kw: r.render_embedding_views(0, W, H, K, Rs[a:a + B], t, 10., 10000., pad, crop, **kw)
    starts = list(range(0, args.pairs, B))

    def wall(fn, to_host=False):
        fn(0)                                                   # warm-up: module load, workspace
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for a in starts:
            out = fn(a)
            if to_host:
                [o.cpu() for o in out]
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    # (a) and (b), alternating, the better of three passes each (the same process, the same clocks)
    two_embeds = lambda a: embed(a)[:1] + embed(a)[:1]
    a_s, b_s = [], []
    for _ in range(3):
        a_s.append(wall(pair))
        b_s.append(wall(two_embeds))
    a_host = wall(lambda a: pair(a)[:3], to_host=True)
    ms = np.zeros(6)
    ms_e = np.zeros(6)
    for a in starts:
        ms += np.array(pair(a, timed=True)[5])
        ms_e += np.array(embed(a, timed=True)[3])
    assert all(int(pair(a)[4].min()) == 1 for a in starts[:2])

    # (c) the correct route through the single-light interface, on the first route-pairs pairs
    n_c = min(args.route_pairs, args.pairs)

    def route():
        y, bbs, _ = r.render_embedding_views(0, W, H, K, Rs[:n_c], t, 10., 10000., pad, crop)
        bbs_h = bbs.cpu().numpy()
        xs, masks = [], []
        for i in range(n_c):
            lt = lights_h[i]
            bgr, depth, _, _ = r.render_batch(0, W, H, K, Rs[i:i + 1], t, 10., 10000., light=(tuple(lt[:3]), lt[3], lt[4], lt[5]))
            shifted = bbs_h[i] + np.array([offsets_h[i, 0] * bbs_h[i, 2], offsets_h[i, 1] * bbs_h[i, 3], 0, 0])
            xs.append(torch_patch(bgr[0], shifted, pad, crop))
            masks.append(torch_patch(depth[0], shifted, pad, crop) == 0)
        return torch.stack(xs), torch.stack(masks), y

    route()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    cx, cm, cy = route()
    torch.cuda.synchronize()
    c_s = time.perf_counter() - t0
    ax, am, ay = pair(0, n_c)[:3]
    identical = bool(torch.equal(ax, cx) and torch.equal(am, cm) and torch.equal(ay, cy))

    a_best, b_best = min(a_s), min(b_s)
    res = {'tool': 'bench_train_render', 'model': args.model, 'faces': int(len(model['faces'])), 'vertices': int(len(r._arrays[0][0])),
           'render_dims': [W, H], 'crop': crop, 'pairs': args.pairs, 'batch': args.batch, 'max_rel_offset': 0.2,
           'a_training_call': {'seconds': [round(v, 5) for v in a_s], 'pairs_per_s': round(args.pairs / a_best, 1),
                               'kernel_ms_total': {k: round(float(v), 3) for k, v in zip(KERNELS, ms)}, 'kernel_ms_sum': round(float(ms.sum()), 3),
                               'seconds_with_host_copies': round(a_host, 5),
                               'seconds_20000_images_with_host_copies': round(a_host * 20000 / args.pairs, 3)},
           'b_two_embedding_calls': {'seconds': [round(v, 5) for v in b_s], 'pairs_per_s': round(args.pairs / b_best, 1),
                                     'kernel_ms_total_one_call': {k: round(float(v), 3) for k, v in zip(EMBED_KERNELS, ms_e)},
                                     'kernel_ms_sum_one_call': round(float(ms_e.sum()), 3)},
           'a_over_b': round(a_best / b_best, 3), 'a_over_one_embedding_call': round(float(ms.sum() / ms_e.sum()), 3),
           'c_per_image_route': {'pairs': n_c, 'seconds': round(c_s, 4), 'pairs_per_s': round(n_c / c_s, 1), 'bytes_identical_to_a': identical,
                                 'seconds_20000_images': round(c_s * 20000 / n_c, 2)},
           'workspace_MB': round(r._ws.numel() / 2 ** 20, 1)}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')
    r.close()


if __name__ == '__main__':
    main()
