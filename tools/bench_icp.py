#!/usr/bin/env python
"""Depth ICP refinement at n = 3000: per mode, one and eight problems per call -- wall time per refinement,
the icp_step period, iterations taken, the share of launches queued behind convergence -- and the same inputs through the
scikit-learn form of the reference's loop on this box's CPU.  Writes profiles/r21_icp/bench_icp.json.

    python tools/bench_icp.py [--reps 5] [--out profiles/r21_icp/bench_icp.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]


def clouds(seed, W=640, H=480, crop=240):
    """a synthetic frame and a crop with ~6000 points each: a tilted bumpy patch seen twice, the second moved a little"""
    r = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    syn = np.zeros((H, W), np.float32)
    m = (np.abs(xx - W // 2) < 45) & (np.abs(yy - H // 2) < 35)
    syn[m] = (700 + 0.3 * (xx - W // 2) + 12 * np.sin(xx / 7.0) * np.cos(yy / 5.0))[m]
    c = np.zeros((crop, crop), np.float32)
    y2, x2 = np.mgrid[0:crop, 0:crop]
    m2 = (np.abs(x2 - crop // 2 - 3) < 45) & (np.abs(y2 - crop // 2 + 2) < 35)
    c[m2] = (708 + 0.33 * (x2 - crop // 2) + 12 * np.sin((x2 - 2) / 7.0) * np.cos((y2 + 1) / 5.0) + r.randn(crop, crop))[m2]
    K = np.array([[572.4, 0, W / 2.0], [0, 573.6, H / 2.0], [0, 0, 1.0]])
    return K, syn, c


def cpu_icp(A, B, bits):
    """the reference's loop with its KD-tree (tests/icp_cases.py restates the rest)"""
    import icp_cases as ic
    from sklearn.neighbors import NearestNeighbors
    src = np.ones((4, len(A)))
    src[:3] = A.T
    prev = 0
    for i in range(100):
        neigh = NearestNeighbors(n_neighbors=1)
        neigh.fit(B)
        dist, idx = neigh.kneighbors(src[:3].T, return_distance=True)
        T = ic.best_fit_transform(src[:3].T, B[idx.ravel()], bits)
        src = np.dot(T, src)
        mean = np.mean(dist)
        if abs(prev - mean) < 1e-6:
            break
        prev = mean
    return ic.best_fit_transform(A, src[:3].T, bits), i


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r21_icp', 'bench_icp.json'))
    args = ap.parse_args()
    import torch
    import icp_cases as ic
    from augmentedautoencoder_amd import icp_engine
    eng = icp_engine.IcpEngine()
    K, syn, crop = clouds(1)
    syn_pts, _, _, real_all, keep, _ = ic.prepare(K, syn, crop, 2.0)
    real_pts = real_all[keep]
    n = min(len(real_pts), len(syn_pts), 3000)
    result = {'n_points': n, 'n_syn': len(syn_pts), 'n_real': len(real_pts), 'cpu_threads': torch.get_num_threads(), 'modes': {}}
    for mode in ic.MODES:
        bits = ic.mode_bits(mode, 'eval')
        row = {}
        for P in (1, 8):
            rs = np.random.RandomState(7)
            subs = [ic.draw(rs, len(real_pts), len(syn_pts)) for _ in range(P)]
            eng.prepare(np.stack([syn] * P), [crop] * P, K, 2.0)
            call = lambda **kw: eng.refine([n] * P, [s[1] for s in subs], [s[0] for s in subs], [bits] * P, **kw)
            out = call()
            walls = []
            for _ in range(args.reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = call()
                walls.append((time.perf_counter() - t0) * 1e3)
            ms = call(timed=True)['kernel_ms']
            its = (out['iterations'] + 1).tolist()
            live, steps = max(its), ms[1:-1]
            row['P%d' % P] = {'iterations': its, 'wall_ms_per_call': [round(w, 3) for w in walls], 'wall_ms_per_refinement': round(min(walls) / P, 3),
                              'step_us_live': round(1e3 * float(np.mean(steps[:live])), 2),
                              'step_us_empty': round(1e3 * float(np.mean(steps[live:])), 2) if live < len(steps) else None,
                              'live_ms': round(float(np.sum(steps[:live])), 3), 'empty_ms': round(float(np.sum(steps[live:])), 3),
                              'empty_launch_share': round(1.0 - live / float(len(steps)), 3), 'gather_us': round(1e3 * ms[0], 2), 'finish_us': round(1e3 * ms[-1], 2)}
        sub_real, sub_syn = subs[0]
        t0 = time.perf_counter()
        T_cpu, i_cpu = cpu_icp(syn_pts[sub_syn], real_pts[sub_real], bits)
        row['cpu_ms'] = round((time.perf_counter() - t0) * 1e3, 1)
        row['cpu_iterations'] = i_cpu + 1
        row['dT_vs_cpu'] = float(np.abs(out['T'][0] - T_cpu).max())
        result['modes'][mode] = row
        print(mode, json.dumps(row))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(result, f, indent=1)
    print('wrote', args.out)


if __name__ == '__main__':
    main()
