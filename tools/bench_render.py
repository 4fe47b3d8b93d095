"""Throughput of the mesh rasteriser next to the encoder it feeds, in one process:

    python tools/bench_render.py [--views 4096] [--batch 256] [--faces 51200] [--out profiles/bench_render.json]

A procedurally generated mesh of T-LESS size (a bumpy torus, ~50k faces, ~140 mm across, per-vertex normals and colours) is
rendered at the template's settings (cfg/train_template.cfg: 720x540, K, radius 700, 128x128 crops, PAD_FACTOR 1.2) for
`views` rows spread evenly over the 92232-row viewsphere, through the fused embedding path (aae_render_embedding_views);
the same crops then go through the default encoder (aae_encoder_forward).  Prints one JSON line: views/s, the per-kernel
split of the six launches, the encode time of the same views and the ratio render / encode."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KERNELS = ('render_init_rect', 'render_vertex', 'render_clear', 'render_raster', 'render_bbox', 'render_crop')


def bumpy_torus(nu, nv, R=45.0, r=22.0):
    a = np.arange(nu) * 2 * np.pi / nu
    b = np.arange(nv) * 2 * np.pi / nv
    A, B = np.meshgrid(a, b, indexing='ij')
    rr_ = r * (1 + 0.15 * np.sin(5 * A) * np.cos(3 * B))

    def pos(A, B, rr_):
        return np.stack([(R + rr_ * np.cos(B)) * np.cos(A), (R + rr_ * np.cos(B)) * np.sin(A), 1.4 * rr_ * np.sin(B)], axis=-1)
    P = pos(A, B, rr_)
    e = 1e-4
    dA = pos(A + e, B, r * (1 + 0.15 * np.sin(5 * (A + e)) * np.cos(3 * B))) - P
    dB = pos(A, B + e, r * (1 + 0.15 * np.sin(5 * A) * np.cos(3 * (B + e)))) - P
    N = np.cross(dA, dB)
    N /= np.linalg.norm(N, axis=-1, keepdims=True)
    C = np.stack([140 + 100 * np.cos(A), 120 + 90 * np.sin(2 * B), 130 + 80 * np.sin(A + B)], axis=-1)
    i, j = np.meshgrid(np.arange(nu), np.arange(nv), indexing='ij')
    p00, p10 = i * nv + j, ((i + 1) % nu) * nv + j
    p01, p11 = i * nv + (j + 1) % nv, ((i + 1) % nu) * nv + (j + 1) % nv
    faces = np.concatenate([np.stack([p00, p10, p11], -1).reshape(-1, 3), np.stack([p00, p11, p01], -1).reshape(-1, 3)])
    return dict(pts=P.reshape(-1, 3), normals=N.reshape(-1, 3), colors=np.floor(C.reshape(-1, 3)), faces=faces.astype(np.float64))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--views', type=int, default=4096)
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--faces', type=int, default=51200)
    ap.add_argument('--model', default='reconst', choices=['reconst', 'cad'])
    ap.add_argument('--out', default=None)
    args = ap.parse_args()

    import torch
    from augmentedautoencoder_amd import viewsphere as vs
    from augmentedautoencoder_amd.engine import EncoderEngine
    from augmentedautoencoder_amd.meshrenderer import Renderer
    from augmentedautoencoder_amd.weights import EncoderConfig
    from oracle import synth

    torch.cuda.set_device(0)
    nv = int(round((args.faces / 2 / 2) ** 0.5))
    model = bumpy_torus(2 * nv, nv)
    r = Renderer([model], model=args.model)
    Rs_all = vs.viewsphere_for_embedding(2562, 700.0, 36)
    pick = np.linspace(0, len(Rs_all) - 1, args.views).astype(np.int64)
    Rs = torch.as_tensor(Rs_all[pick].reshape(-1, 9), device='cuda')
    W, H, crop = 720, 540, 128
    K = np.array([1075.65, 0, 720 / 2, 0, 1073.90, 540 / 2, 0, 0, 1]).reshape(3, 3)
    t = np.array([0., 0., 700.])
    call = lambda a, **kw: r.render_embedding_views(0, W, H, K, Rs[a:a + args.batch], t, 10., 10000., 1.2, crop, **kw)

    crops, bbs, vis = call(0)                                   # warm-up: module load, workspace
    torch.cuda.synchronize()
    starts = list(range(0, args.views, args.batch))
    t0 = time.perf_counter()
    kept = [call(a)[0] for a in starts]
    torch.cuda.synchronize()
    render_s = time.perf_counter() - t0
    assert all(int(call(a)[2].min()) == 1 for a in starts[:2])
    box = bbs.cpu().numpy()

    ms = np.zeros(6)
    for a in starts:
        ms += np.array(call(a, timed=True)[3])
    split = {k: round(float(v), 3) for k, v in zip(KERNELS, ms)}

    enc = EncoderEngine(EncoderConfig(), synth.make_weights(seed=2024), max_batch=args.batch)
    enc.encode(kept[0])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for x in kept:
        enc.encode(x)
    torch.cuda.synchronize()
    encode_s = time.perf_counter() - t0

    res = {'tool': 'bench_render', 'model': args.model, 'faces': int(len(model['faces'])), 'vertices': int(len(r._arrays[0][0])),
           'render_dims': [W, H], 'crop': crop, 'views': args.views, 'batch': args.batch,
           'render_seconds': round(render_s, 4), 'views_per_s': round(args.views / render_s, 1),
           'kernel_ms_total': split, 'kernel_ms_sum': round(float(ms.sum()), 3),
           'encode_seconds': round(encode_s, 4), 'encode_views_per_s': round(args.views / encode_s, 1),
           'render_over_encode': round(render_s / encode_s, 3),
           'projected_92232_views': {'render_s': round(render_s * 92232 / args.views, 2), 'encode_s': round(encode_s * 92232 / args.views, 2)},
           'mean_obj_bb_wh': [round(float(box[:, 2].mean()), 1), round(float(box[:, 3].mean()), 1)],
           'workspace_MB': round(r._ws.numel() / 2 ** 20, 1)}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')
    r.close()
    enc.close()


if __name__ == '__main__':
    main()
