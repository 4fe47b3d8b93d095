#!/usr/bin/env python
"""The encoder's backward pass on the template network (128 x 128 x 3, filters 128-256-512-512, 5 x 5 stride 2, latent 128) at B = 64
and 256: the whole call in windows of at least 0.5 s (two runs each), the time per launch from the timed call, executed FLOP against
the fp32 matrix peak, the forward encode of the same batch beside it, and torch autograd over F.pad + conv2d on the same GPU, in a
child process with a time limit of its own (its first backward searches convolution algorithms; when that does not finish the row
says "not measured").  One JSON line per measurement; --out DIR also writes them to DIR/bench_encoder_bwd.jsonl and the register /
LDS use of every kernel of the translation unit to DIR/kernel_resources.txt.

Executed FLOP are what the kernels multiply (zero-padded tile edges not counted): per layer 2 KS^2 Cin Cout B Ho Wo for the weight
gradient, the same for the data gradient where it runs (selected taps: every (tap, output pixel) pair once; not for conv1, whose dx
nobody asks for), 2 B J U for each dense product."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK_F32_TFLOPS = 157.3


def executed_flops(cfg, B):
    total = 0.0
    for i, (h, w, ci, ho, wo, co) in enumerate(cfg.layer_shapes()):
        per = 2.0 * cfg.kernel_size ** 2 * ci * co * B * ho * wo
        total += per * (1 if i == 0 else 2)
    return total + 2 * 2.0 * B * cfg.flatten_size * cfg.latent_space_size


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


def torch_child(B, seconds, runs):
    """torch autograd of the same network: backward by difference of forward + backward and forward"""
    import torch
    import torch.nn.functional as F
    from augmentedautoencoder_amd import synth
    from augmentedautoencoder_amd.weights import EncoderConfig, conv_names
    from oracle import reference_cpu as ref
    cfg = EncoderConfig()
    w = synth.make_weights()
    names = conv_names(cfg.num_layers)
    kernels = [torch.from_numpy(np.array(w[n + '/kernel'])).cuda().permute(3, 2, 0, 1).contiguous().requires_grad_(True) for n in names]
    biases = [torch.from_numpy(np.array(w[n + '/bias'])).cuda().requires_grad_(True) for n in names]
    wd = torch.from_numpy(np.array(w['dense/kernel'])).cuda().requires_grad_(True)
    bd = torch.from_numpy(np.array(w['dense/bias'])).cuda().requires_grad_(True)
    x = torch.rand((B, cfg.shape[2]) + tuple(cfg.shape[:2]), device='cuda')
    gz = torch.randn((B, cfg.latent_space_size), device='cuda')
    pads = []
    for (h, wi, _, _, _, _), s in zip(cfg.layer_shapes(), cfg.strides):
        (_, pt, pb), (_, pl, pr) = ref.same_pad(h, cfg.kernel_size, s), ref.same_pad(wi, cfg.kernel_size, s)
        pads.append((pl, pr, pt, pb))

    def step():
        h = x
        for kk, bb, p, s in zip(kernels, biases, pads, cfg.strides):
            h = torch.relu(F.conv2d(F.pad(h, p), kk, bb, stride=s))
        return h.permute(0, 2, 3, 1).reshape(B, -1) @ wd + bd

    def fwd_bwd():
        torch.autograd.grad(step(), kernels + biases + [wd, bd], grad_outputs=gz)

    def fwd_only():
        with torch.no_grad():
            step()
    for run in range(runs):
        f_ms, _ = window(fwd_only, torch, seconds)
        fb_ms, n = window(fwd_bwd, torch, seconds)
        print(json.dumps({'what': 'torch_autograd', 'B': B, 'run': run, 'forward_plus_backward_ms': round(fb_ms, 4), 'forward_ms': round(f_ms, 4),
                          'backward_ms_by_difference': round(fb_ms - f_ms, 4), 'calls': n}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', type=int, nargs='+', default=[64, 256])
    ap.add_argument('--seconds', type=float, default=0.5)
    ap.add_argument('--runs', type=int, default=2)
    ap.add_argument('--out', default=None)
    ap.add_argument('--torch-limit', type=float, default=120.0, help='seconds the torch autograd child process may take per batch')
    ap.add_argument('--no-torch', action='store_true', help='skip the torch autograd child process')
    ap.add_argument('--torch-child', type=int, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.torch_child is not None:
        return torch_child(args.torch_child, args.seconds, args.runs)
    import torch
    from augmentedautoencoder_amd import synth
    from augmentedautoencoder_amd.engine import EncoderEngine
    from augmentedautoencoder_amd.weights import EncoderConfig
    assert torch.cuda.is_available(), 'bench_encoder_bwd.py measures on the GPU'
    cfg = EncoderConfig()
    w = synth.make_weights()
    if args.out:
        os.makedirs(args.out, exist_ok=True)
    sink = open(os.path.join(args.out, 'bench_encoder_bwd.jsonl'), 'w') if args.out else None

    def emit(row):
        print(json.dumps(row), flush=True)
        if sink:
            sink.write(json.dumps(row) + '\n')
            sink.flush()

    for B in args.batches:
        eng = EncoderEngine(cfg, w, max_batch=max(256, B))
        x = torch.from_numpy(synth.make_crops(B, seed=B)).cuda()
        z = eng.encode(x)
        dz = torch.from_numpy(np.random.default_rng(B).standard_normal(tuple(z.shape)).astype(np.float32)).cuda()
        grads, _ = eng.backward(x, dz)
        flops = executed_flops(cfg, B)
        for run in range(args.runs):
            fwd_ms, fwd_n = window(lambda: eng.encode(x), torch, args.seconds)
            bwd_ms, bwd_n = window(lambda: eng.backward(x, dz, out=grads), torch, args.seconds)
            emit({'what': 'encoder_backward', 'B': B, 'run': run, 'backward_ms': round(bwd_ms, 4), 'calls': bwd_n, 'forward_encode_ms': round(fwd_ms, 4), 'forward_calls': fwd_n,
                  'executed_gflop': round(flops / 1e9, 2), 'tflops': round(flops / bwd_ms / 1e9, 2), 'frac_of_f32_matrix_peak': round(flops / bwd_ms / 1e9 / PEAK_F32_TFLOPS, 4)})
        eng.backward(x, dz, out=grads, timed=True)
        _, _, timed = eng.backward(x, dz, out=grads, timed=True)
        emit({'what': 'kernels', 'B': B, 'kernels': [{'label': l, 'ms': round(ms, 4)} for l, ms in timed], 'sum_ms': round(sum(ms for _, ms in timed), 4)})
        eng.close()
        torch.cuda.synchronize()
        if args.no_torch:
            continue
        try:                                # a fresh process: its algorithm search may not finish, and must not take this one with it
            out = subprocess.run([sys.executable, os.path.abspath(__file__), '--torch-child', str(B), '--seconds', str(args.seconds), '--runs', str(args.runs)],
                                 stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=args.torch_limit)
            rows = [json.loads(l) for l in out.stdout.decode().splitlines() if l.startswith('{')]
            if out.returncode != 0 or not rows:
                emit({'what': 'torch_autograd', 'B': B, 'ran': False, 'error': 'not measured: exit status %d: %s' % (out.returncode, out.stderr.decode()[-300:])})
            for row in rows:
                emit(row)
        except subprocess.TimeoutExpired:
            emit({'what': 'torch_autograd', 'B': B, 'ran': False, 'error': 'not measured: no result within %.0f s' % args.torch_limit})
    if sink:
        sink.close()
    if args.out:
        res = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'kernel_resources.py'), '--unit', 'aae_encoder_bwd', '-o', os.path.join(args.out, '_resources_build.so')],
                             stdout=subprocess.PIPE)
        open(os.path.join(args.out, 'kernel_resources.txt'), 'wb').write(res.stdout)
        if os.path.exists(os.path.join(args.out, '_resources_build.so')):
            os.remove(os.path.join(args.out, '_resources_build.so'))


if __name__ == '__main__':
    main()
