"""The reconstruction loss at the template's shape (128x128x3, L2, BOOTSTRAP_RATIO 4) next to the same quantity written with torch:

    python tools/bench_loss.py [--batches 64 256] [--window 0.5] [--out profiles/r27_loss/bench_loss_run1.json]

Per batch size, on device-resident tensors (x a sigmoid of random numbers, the target uniform: errors that share a few exponents):

  launch            aae_recon_loss alone (the selecting kernel + the 1-block finish), as many calls as fill `window` seconds
                    between two device events, three passes, with dx and without; the bytes it must move (x and target read once,
                    dx written: 3 B n 4 bytes with dx, 2 B n 4 without) over that time.  At B = 64 a quarter of the 256 CUs have a
                    workgroup: the launch is latency-bound by design, the GB/s figure says how far from the traffic floor.
  launch_ratio_1    the same launch with bootstrap_ratio 1 (no radix pass, one sweep): the difference is what the selection costs;
  torch_topk        ((x - t)**2).flatten(1).topk(k).values.mean() and its backward for dx (autograd), the same timing;
                    torch_topk_forward the forward alone;
  reconstr_loss     Decoder.reconstr_loss_device from device-resident batches (encode, decode, loss; the default network with
                    seeded weights), host clock around calls that end in a synchronise;
  histogram         with AAE_EXPERIMENTS=1 (the experiments library): the launch with the histogram per lane group (the product's),
                    per wave and shared, alternating.

Prints one JSON line."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', type=int, nargs='+', default=[64, 256])
    ap.add_argument('--window', type=float, default=0.5, help='seconds each timed window must last')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()

    import torch
    from augmentedautoencoder_amd import _lib, loss as L, session as S, synth
    from augmentedautoencoder_amd.decoder import Decoder
    from augmentedautoencoder_amd.encoder import Encoder

    assert torch.cuda.is_available(), 'bench_loss needs the GPU'
    torch.cuda.set_device(0)
    lib = _lib.load()
    H, W, C, ratio = 128, 128, 3, 4
    n = H * W * C
    k = n // ratio

    def timed(fn, window):
        """ms per call: three passes of as many calls as fill `window` seconds, between device events"""
        for _ in range(3):
            fn()
        torch.cuda.synchronize()

        def one_pass(count):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(count):
                fn()
            t1.record()
            t1.synchronize()
            return t0.elapsed_time(t1) / count
        count = max(20, int(np.ceil(window * 1e3 / one_pass(20))))
        return [round(one_pass(count), 5) for _ in range(3)], count

    enc = Encoder(S.Placeholder((H, W, C)), synth.DEFAULT_LATENT, list(synth.DEFAULT_NUM_FILTER), synth.DEFAULT_KERNEL, list(synth.DEFAULT_STRIDES), False)
    dec = Decoder(S.Placeholder((H, W, C), 'reconst_target'), enc.z, list(reversed(synth.DEFAULT_NUM_FILTER)), synth.DEFAULT_KERNEL,
                  list(reversed(synth.DEFAULT_STRIDES)), loss='L2', bootstrap_ratio=ratio, encoder=enc)
    enc.load_weights(synth.make_weights(seed=2024))
    dec.load_weights(synth.make_decoder_weights_for(dec.config, seed=4242))

    res = {'tool': 'bench_loss', 'shape': [H, W, C], 'loss': 'L2', 'bootstrap_ratio': ratio, 'k': k, 'window_s': args.window,
           'experiments_library': bool(lib.aae_has_experiments()), 'batches': {}}
    gen = torch.Generator(device='cuda').manual_seed(27)
    for B in args.batches:
        x = torch.sigmoid(torch.randn((B, H, W, C), device='cuda', generator=gen))
        t = torch.rand((B, H, W, C), device='cuda', generator=gen)
        out = (torch.empty(1, device='cuda'), torch.empty(B, device='cuda'), torch.empty_like(x))
        ws = torch.empty(int(lib.aae_recon_loss_workspace_bytes(B, n)), dtype=torch.uint8, device='cuda')
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        p = lambda a: ctypes.c_void_p(a.data_ptr())

        def launch(with_dx=True, r=ratio):
            desc = _lib.ReconLossDesc(B, n, _lib.AAE_LOSS_L2, r)
            rc = lib.aae_recon_loss(ctypes.byref(desc), p(x), p(t), p(out[0]), p(out[1]), p(out[2]) if with_dx else None, p(ws), ws.numel(), stream)
            assert rc == 0, lib.aae_last_error()

        xg = x.clone().requires_grad_(True)

        def torch_topk(backward=True):
            loss = ((xg - t) ** 2).flatten(1).topk(k).values.mean()
            if backward:
                xg.grad = None
                loss.backward()
            return loss

        # the two formulations agree before they are timed
        launch()
        ref = torch_topk()
        torch.cuda.synchronize()
        assert abs(float(out[0][0]) - float(ref)) <= 1e-5 * float(ref), (float(out[0][0]), float(ref))
        assert float((out[2] - xg.grad).abs().max()) <= 1e-6 * float(xg.grad.abs().max())

        row = {}
        row['launch_ms'], row['launch_calls_per_pass'] = timed(lambda: launch(True), args.window)
        row['launch_no_dx_ms'], _ = timed(lambda: launch(False), args.window)
        row['launch_ratio_1_ms'], _ = timed(lambda: launch(True, 1), args.window)
        row['torch_topk_ms'], row['torch_calls_per_pass'] = timed(lambda: torch_topk(True), args.window)
        row['torch_topk_forward_ms'], _ = timed(lambda: torch_topk(False), args.window)
        best, best_no_dx = min(row['launch_ms']), min(row['launch_no_dx_ms'])
        row['floor_bytes_with_dx'], row['floor_bytes_no_dx'] = 3 * B * n * 4, 2 * B * n * 4
        row['launch_GB_per_s'] = round(3 * B * n * 4 / (best * 1e-3) / 1e9, 1)
        row['launch_no_dx_GB_per_s'] = round(2 * B * n * 4 / (best_no_dx * 1e-3) / 1e9, 1)
        row['selection_ms'] = round(best - min(row['launch_ratio_1_ms']), 5)
        row['torch_over_launch'] = round(min(row['torch_topk_ms']) / max(row['launch_ms']), 2)           # the ranges' near ends
        row['torch_forward_over_launch_no_dx'] = round(min(row['torch_topk_forward_ms']) / max(row['launch_no_dx_ms']), 2)
        row['workgroups_over_CUs'] = round(B / 256.0, 3)

        crops = (x * 255).to(torch.uint8)
        feed = {enc.x: crops, dec.reconstruction_target: t}

        def api():
            return dec.reconstr_loss_device(feed)[0]
        for _ in range(3):
            api()
        torch.cuda.synchronize()

        def api_pass(count):
            t0 = time.perf_counter()
            for _ in range(count):
                api()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / count * 1e3
        count = max(10, int(np.ceil(args.window * 1e3 / api_pass(10))))
        row['reconstr_loss_ms'] = [round(api_pass(count), 4) for _ in range(3)]
        row['reconstr_loss_calls_per_pass'] = count

        if lib.aae_has_experiments():
            modes = {'lane_groups': '0', 'per_wave': '1', 'shared': '2'}
            hist = {m: [] for m in modes}
            for _ in range(3):                                          # alternating
                for m, v in modes.items():
                    os.environ['AAE_LOSS_HIST'] = v
                    hist[m].append(min(timed(lambda: launch(True), args.window / 3)[0]))
            os.environ['AAE_LOSS_HIST'] = '0'
            row['histogram_ms'] = hist
        res['batches'][str(B)] = row
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
