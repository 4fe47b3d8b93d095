#!/usr/bin/env python
"""The decoder's backward pass on the template network (128 x 128 x 3, filters 512-512-256-128, 5 x 5, latent 128) at B = 64 and 256:
the whole call in windows of at least 0.5 s (two runs each), per-kernel times from the timed call, executed FLOP against the fp32
matrix peak, the forward decode of the same batch beside it, and torch autograd over interpolate + conv2d on the same GPU.
One JSON line per measurement; --out DIR also writes them to DIR/bench_decoder_bwd.jsonl.

Executed FLOP are what the phase-folded kernels multiply (zero-padded tile edges not counted): per stage 2 P U^2 Cin Cout B H W for
the weight gradient and the same for the data gradient (K padded to a multiple of 4 channels), 2 B J U for each dense product."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK_F32_TFLOPS = 157.3


def executed_flops(cfg, B):
    dims = cfg.layer_dimensions() + [list(cfg.shape[:2])]
    chans = cfg.num_filters + [cfg.shape[2]]
    k = cfg.kernel_size
    total = 2 * 2.0 * B * cfg.latent_space_size * dims[0][0] * dims[0][1] * chans[0]
    for i in range(len(chans) - 1):
        (h, w), (uh, uw) = dims[i], dims[i + 1]
        P, U = (4, (k + 1) // 2) if (uh, uw) == (2 * h, 2 * w) else (1, k)
        total += 2.0 * P * U * U * chans[i] * B * h * w * (chans[i + 1] + 4 * -(-chans[i + 1] // 4))
    return total


def window(fn, torch, seconds):
    fn()
    torch.cuda.synchronize()
    n, t0 = 0, time.perf_counter()
    while True:
        for _ in range(4):
            fn()
        n += 4
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if dt >= seconds:
            return dt / n * 1e3, n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', type=int, nargs='+', default=[64, 256])
    ap.add_argument('--seconds', type=float, default=0.5)
    ap.add_argument('--runs', type=int, default=2)
    ap.add_argument('--out', default=None)
    ap.add_argument('--torch-batches', type=int, nargs='*', default=[64], help='batches at which torch autograd runs beside it (its first backward at B = 256 searches convolution algorithms for minutes)')
    args = ap.parse_args()
    import torch
    from augmentedautoencoder_amd.engine import DecoderEngine
    from augmentedautoencoder_amd.weights import DecoderConfig
    from oracle import decoder_cpu as dref
    assert torch.cuda.is_available(), 'bench_decoder_bwd.py measures on the GPU'
    cfg = DecoderConfig()
    w = dref.make_decoder_weights()
    if args.out:
        os.makedirs(args.out, exist_ok=True)
    sink = open(os.path.join(args.out, 'bench_decoder_bwd.jsonl'), 'w') if args.out else None

    def emit(row):
        print(json.dumps(row), flush=True)
        if sink:
            sink.write(json.dumps(row) + '\n')
            sink.flush()

    for B in args.batches:
        eng = DecoderEngine(cfg, w, max_batch=max(256, B))
        z = torch.from_numpy(np.random.default_rng(B).standard_normal((B, cfg.latent_space_size)).astype(np.float32)).cuda()
        x = eng.decode(z)
        dx = (torch.rand_like(x) - 0.5) / x.numel()
        grads, dz = eng.backward(z, x, dx)
        flops = executed_flops(cfg, B)
        for run in range(args.runs):
            fwd_ms, fwd_n = window(lambda: eng.decode(z, out=x), torch, args.seconds)
            bwd_ms, bwd_n = window(lambda: eng.backward(z, x, dx, out=grads), torch, args.seconds)
            emit({'what': 'decoder_backward', 'B': B, 'run': run, 'backward_ms': round(bwd_ms, 4), 'calls': bwd_n, 'forward_decode_ms': round(fwd_ms, 4), 'forward_calls': fwd_n,
                  'executed_gflop': round(flops / 1e9, 2), 'tflops': round(flops / bwd_ms / 1e9, 2), 'frac_of_f32_matrix_peak': round(flops / bwd_ms / 1e9 / PEAK_F32_TFLOPS, 4)})
        _, _, timed = eng.backward(z, x, dx, out=grads, timed=True)
        _, _, timed = eng.backward(z, x, dx, out=grads, timed=True)
        emit({'what': 'kernels', 'B': B, 'kernels': [{'label': l, 'ms': round(ms, 4)} for l, ms in timed], 'sum_ms': round(sum(ms for _, ms in timed), 4)})
        eng.close()
        if B not in args.torch_batches:
            emit({'what': 'torch_autograd', 'B': B, 'ran': False, 'error': 'not asked for (--torch-batches)'})
            continue
        try:
            import torch.nn.functional as F
            dense, convs, final, _ = cfg.variable_names(w)
            params = [torch.from_numpy(np.array(w[n + s])).cuda().requires_grad_(True) for n in [dense] + convs + [final] for s in ('/kernel', '/bias')]
            kernels = [p.detach().permute(3, 2, 0, 1).contiguous().requires_grad_(True) for p in params[2::2]]
            dims = cfg.layer_dimensions() + [list(cfg.shape[:2])]
            zt = z.clone().requires_grad_(True)
            gx = dx.permute(0, 3, 1, 2).contiguous()

            def step():
                h = torch.relu(zt @ params[0] + params[1]).reshape(B, dims[0][0], dims[0][1], cfg.num_filters[0]).permute(0, 3, 1, 2)
                for i, kk in enumerate(kernels):
                    h = F.conv2d(F.interpolate(h, size=tuple(dims[i + 1]), mode='nearest'), kk, params[3 + 2 * i], padding=cfg.kernel_size // 2)
                    h = torch.sigmoid(h) if i + 1 == len(kernels) else torch.relu(h)
                return h

            def fwd_bwd():
                torch.autograd.grad(step(), [zt, params[0], params[1]] + kernels + params[3::2], grad_outputs=gx)

            def fwd_only():
                with torch.no_grad():
                    step()
            for run in range(args.runs):
                f_ms, _ = window(fwd_only, torch, args.seconds)
                fb_ms, n = window(fwd_bwd, torch, args.seconds)
                emit({'what': 'torch_autograd', 'B': B, 'run': run, 'forward_plus_backward_ms': round(fb_ms, 4), 'forward_ms': round(f_ms, 4),
                      'backward_ms_by_difference': round(fb_ms - f_ms, 4), 'calls': n})
        except Exception as e:            # (said, not hidden: the comparison partner did not run here)
            emit({'what': 'torch_autograd', 'B': B, 'ran': False, 'error': '%s: %s' % (type(e).__name__, str(e)[:300])})
    if sink:
        sink.close()


if __name__ == '__main__':
    main()
