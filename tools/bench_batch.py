"""Throughput of Dataset.batch_device at the template's shape and chain, next to the only baseline there is:

    python tools/bench_batch.py [--batches 64 256 1024] [--window 0.6] [--out profiles/r26_augment_batch/bench_batch.json]

Random uint8 training images, masks and backgrounds at 128x128x3 (the pixel values do not change the work), the cfg template's
[Augmentation] CODE.  Per batch size:

  batch_device      Dataset.batch_device end to end (np.random draws on the host, one upload of the programs, one launch), host
                    clock around as many calls as fill `window` seconds, ending in a synchronise, the best of three passes: images/s;
  kernel            the launch alone for one drawn batch, as many launches as fill `window` seconds between two device events,
                    three passes: ms and images/s, and the bytes it must move (inputs read once, the two fp32 outputs written)
                    over that time;
  numpy_float64     the float64 restatement of tests/augment_reference.py on the host for the same programs, the images only
                    (track=False: without the acceptance mask the tests compute beside them): seconds and images/s.
                    The parent commit has no batch path; this is a restatement written for checking, not a tuned CPU pipeline.

Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

TEMPLATE_CODE = """Sequential([
    Sometimes(0.5, Affine(scale=(1.0, 1.2))),
    Sometimes(0.5, CoarseDropout( p=0.2, size_percent=0.05) ),
    Sometimes(0.5, GaussianBlur(1.2*np.random.rand())),
    Sometimes(0.5, Add((-25, 25), per_channel=0.3)),
    Sometimes(0.3, Invert(0.2, per_channel=True)),
    Sometimes(0.5, Multiply((0.6, 1.4), per_channel=0.5)),
    Sometimes(0.5, Multiply((0.6, 1.4))),
    Sometimes(0.5, ContrastNormalization((0.5, 2.2), per_channel=0.3))
    ], random_order=False)"""


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', type=int, nargs='+', default=[64, 256, 1024])
    ap.add_argument('--window', type=float, default=0.6, help='seconds each timed window must last')
    ap.add_argument('--train', type=int, default=2048)
    ap.add_argument('--bg', type=int, default=2048)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()

    import torch
    import augment_reference as ar
    from augmentedautoencoder_amd import augmentation as aug
    from augmentedautoencoder_amd.dataset import Dataset

    assert torch.cuda.is_available(), 'bench_batch needs the GPU'
    torch.cuda.set_device(0)
    H = W = 128
    C = 3
    rng = np.random.RandomState(26)
    np.random.seed(26)
    ds = Dataset('', h=H, w=W, c=C, code=TEMPLATE_CODE, realistic_occlusion='False', square_occlusion='False', noof_training_imgs=args.train)
    ds.train_x = rng.randint(0, 256, (args.train, H, W, C)).astype(np.uint8)
    ds.train_y = rng.randint(0, 256, (args.train, H, W, C)).astype(np.uint8)
    ds.mask_x = rng.rand(args.train, H, W) < 0.6
    ds.bg_imgs = rng.randint(0, 256, (args.bg, H, W, C)).astype(np.uint8)
    ds.to_device()
    dev = ds._on_device()

    res = {'tool': 'bench_batch', 'shape': [H, W, C], 'train_images': args.train, 'bg_images': args.bg, 'window_s': args.window,
           'blur_sigma_of_the_parsed_chain': round(ds._aug_plan[2]['args']['sigma'], 4), 'batches': {}}
    for B in args.batches:
        for _ in range(3):                                      # warm-up of this shape
            ds.batch_device(B)
        torch.cuda.synchronize()
        def device_pass(n):
            t0 = time.perf_counter()
            for _ in range(n):
                ds.batch_device(B)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / n
        n_calls = max(20, int(np.ceil(args.window / device_pass(20))))
        passes = [device_pass(n_calls) for _ in range(3)]
        t0 = time.perf_counter()
        for _ in range(20):
            ti, bi, pb = ds._draw_batch(B)
        draw_s = (time.perf_counter() - t0) / 20
        estimate = aug.run_batch(*dev, ti, bi, pb, want_u8=False, timed=20)[3]
        n_launches = max(20, int(np.ceil(args.window * 1e3 / estimate)))
        kernel_ms = [aug.run_batch(*dev, ti, bi, pb, want_u8=False, timed=n_launches)[3] for _ in range(3)]
        t0 = time.perf_counter()
        ref, _, _ = ar.reference_batch(ds.train_x, ds.mask_x, ds.train_y, ds.bg_imgs, ti, bi, pb.programs, track=False)
        y64 = ds.train_y[ti] / 255.
        x64 = ref / 255.
        host_s = time.perf_counter() - t0
        del x64, y64
        moved = B * H * W * C * (1 + 1 + 1 + 4 + 4) + B * H * W               # train_x, bg, train_y read; two fp32 outputs written; the mask
        best, kms = min(passes), min(kernel_ms)
        res['batches'][str(B)] = {
            'batch_device_calls_per_pass': n_calls, 'kernel_launches_per_pass': n_launches,
            'batch_device_seconds': [round(v, 6) for v in passes], 'batch_device_images_per_s': round(B / best, 1),
            'host_draws_seconds': round(draw_s, 6),
            'kernel_ms': [round(v, 4) for v in kernel_ms], 'kernel_images_per_s': round(B / (kms * 1e-3), 1),
            'kernel_bytes_moved': moved, 'kernel_GB_per_s': round(moved / (kms * 1e-3) / 1e9, 1),
            'ops_per_image': round(float(pb.n_ops.mean()), 2), 'blurred_images': int(sum(any(o[0] == 'blur' for o in p) for p in pb.programs)),
            'numpy_float64_seconds': round(host_s, 4), 'numpy_float64_images_per_s': round(B / host_s, 1),
            'kernel_over_numpy': round(host_s / (kms * 1e-3), 1)}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
