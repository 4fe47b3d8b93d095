#!/usr/bin/env python
"""Top-k of per-detection batches on the default codebook (92 232 x 128 fp32) and the default network: the sorted lists inside
the stream scan, merged by the last block to arrive (AAE_SCAN_AUTO: one launch) against the earlier form (AAE_SCAN_AUTO_TOPK_ROWS:
the scan writes the [B,N] similarity rows, topk_chunks_kernel + topk_merge_kernel follow -- three launches), alternating in one
process, answers compared.

  * device period per query (aae_codebook_nn_timed: `reps` queries back to back between two events) for B in {1, 4} x k in
    {1, 2, 5, 8}, `rounds` times per form; k = 1 is the top-1 query of the same run, the same in both modes.  Two kinds of
    queries: "spread" (random latents: the k best rows lie in k different blocks, the finisher reads first pieces only) and
    "one_block" (eight planted neighbours of the query in ONE 128-row block: the finisher follows one list to its end, its
    longest chain of dependent loads);
  * host-synchronised time of the fused aae_encode_nn_topk call at B = 1, k = 8 against aae_encoder_forward + aae_codebook_nn on
    the earlier form.

Per point: the median over the rounds and the spread (max - min) of each form.  One JSON document on stdout (--out FILE: also there).
Usage: python tools/bench_topk_small.py [--reps 300] [--rounds 5] [--out profiles/.../topk_small.json]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from augmentedautoencoder_amd import _lib, synth
from augmentedautoencoder_amd.engine import CodebookEngine, EncoderEngine
from augmentedautoencoder_amd.weights import EncoderConfig

ap = argparse.ArgumentParser()
ap.add_argument('--reps', type=int, default=300)
ap.add_argument('--rounds', type=int, default=5)
ap.add_argument('--rows', type=int, default=92232)
ap.add_argument('--out', default=None)
args = ap.parse_args()
if args.reps < 200:
    sys.exit('--reps: at least 200 queries per timed window')

FORMS = (('lists_in_scan', _lib.AAE_SCAN_AUTO), ('similarity_rows', _lib.AAE_SCAN_AUTO_TOPK_ROWS))


def summary(us):
    return {'median_us': round(statistics.median(us), 3), 'spread_us': round(max(us) - min(us), 3), 'runs_us': [round(v, 3) for v in us]}


lib = _lib.load()
E = synth.make_codebook(args.rows, 128, seed=7, planted_duplicates=16)
rng = np.random.default_rng(99)
centre = rng.standard_normal(128)
centre /= np.linalg.norm(centre)
first = (args.rows // 2) // 128 * 128 + 40                         # eight neighbours of `centre` inside one block
for r in range(first, first + 8):
    v = centre + 0.3 * rng.standard_normal(128) / np.sqrt(128)
    E[r] = (v / np.linalg.norm(v)).astype(np.float32)
cb = CodebookEngine(E)
result = {'codebook_rows': args.rows, 'reps': args.reps, 'rounds': args.rounds, 'device': torch.cuda.get_device_name(0), 'scan': [], 'fused': None}
for kind, B in (('spread', 1), ('spread', 4), ('one_block', 1), ('one_block', 4)):
    z = torch.from_numpy(np.random.default_rng(1234 + B).standard_normal((B, 128)).astype(np.float32) * 3.0).cuda()
    if kind == 'one_block':
        z[:] = torch.from_numpy((5.0 * centre).astype(np.float32)).cuda()
    top1 = None
    for k in (1, 2, 5, 8):
        runs = {name: [] for name, _ in FORMS}
        answers, launches = {}, {}
        for name, mode in FORMS:                                     # warm-up: code objects, workspace growth
            cb.set_scan_mode(mode)
            cb.nn_timed(z, k, 1, reps=20)
        for _ in range(args.rounds):
            for name, mode in FORMS:
                cb.set_scan_mode(mode)
                idx, score, ms = cb.nn_timed(z, k, 1, reps=args.reps)
                runs[name].append(ms * 1e3)
                launches[name] = lib.aae_codebook_last_launches()
                answers[name] = (idx.cpu().numpy().copy(), score.cpu().numpy().copy())
        a, b = answers['lists_in_scan'], answers['similarity_rows']
        point = {'queries': kind, 'B': B, 'k': k, 'launches': launches, 'identical_answers': bool((a[0] == b[0]).all() and (a[1].view('uint32') == b[1].view('uint32')).all())}
        for name, _ in FORMS:
            point[name] = summary(runs[name])
        if k == 1:
            top1 = statistics.median(runs['lists_in_scan'] + runs['similarity_rows'])
        point['top1_period_us'] = round(top1, 3)
        for name, _ in FORMS:
            point[name]['ratio_to_top1'] = round(point[name]['median_us'] / top1, 3)
        result['scan'].append(point)
        print(json.dumps(point), file=sys.stderr, flush=True)

# the fused call at B = 1, k = 8: host clock around a call that ends in a stream synchronise
enc = EncoderEngine(EncoderConfig(), synth.make_weights(seed=2024), max_batch=4)
x = torch.from_numpy(synth.make_crops(1, seed=5)).cuda()


def fused():
    return enc.encode_nn(cb, x, topk=8)


def two_calls():
    z = enc.encode(x)
    idx, score = cb.nn(z, 8)
    return z, idx, score


def host_us(fn, reps):
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
        torch.cuda.current_stream().synchronize()
    return (time.perf_counter() - t0) / reps * 1e6


runs = {'fused_lists_in_scan': [], 'two_calls_similarity_rows': []}
out = {}
for _ in range(args.rounds):
    cb.set_scan_mode(_lib.AAE_SCAN_AUTO)
    runs['fused_lists_in_scan'].append(host_us(fused, args.reps))
    out['fused'] = fused()
    cb.set_scan_mode(_lib.AAE_SCAN_AUTO_TOPK_ROWS)
    runs['two_calls_similarity_rows'].append(host_us(two_calls, args.reps))
    out['two'] = two_calls()
cb.set_scan_mode(_lib.AAE_SCAN_AUTO)
result['fused'] = {'B': 1, 'k': 8, 'identical_answers': bool(all((p.cpu().numpy() == q.cpu().numpy()).all() for p, q in zip(out['fused'], out['two'])))}
for name, us in runs.items():
    result['fused'][name] = summary(us)
enc.close()
cb.close()
text = json.dumps(result, indent=1)
print(text)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text + '\n')
