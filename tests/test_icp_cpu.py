"""The depth refinement without a GPU: csrc/kernels/icp_core.h compiled for the host and driven by tests/native/icp_host.cpp
(serial loops in place of the launches, the blocks of a step in forward, reverse and shuffled order) against NumPy, the
float64 restatement of tests/icp_cases.py and the golden recorded from the reference's own code
(tests/golden/make_icp_golden.py); and the same driver under -fsanitize=address,undefined."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import icp_cases as ic

HERE = os.path.dirname(os.path.abspath(__file__))
ORDERS = (0, 1, 2)                              # forward, reverse, shuffled


def _compiler():
    for c in ('g++', '/opt/rocm/lib/llvm/bin/clang++', 'clang++'):
        path = shutil.which(c) or (c if os.path.isabs(c) and os.path.exists(c) else None)
        if path:
            return path
    raise RuntimeError('no host C++ compiler (g++ or clang++) found')


def _build(out_dir, flags, name):
    exe = os.path.join(str(out_dir), name)
    subprocess.check_call([_compiler(), '-std=c++17', '-O2', '-ffp-contract=off', '-Wall'] + flags +
                          [os.path.join(HERE, 'native', 'icp_host.cpp'), '-o', exe])
    return exe


@pytest.fixture(scope='module')
def host_exe(tmp_path_factory):
    return _build(tmp_path_factory.mktemp('icp_host'), [], 'icp_host')


@pytest.fixture(scope='module')
def golden():
    return dict(np.load(ic.GOLDEN))


def _run(exe, tmp_path, K, syn, crop, factor, **kw):
    prob, out = str(tmp_path / 'problem.bin'), str(tmp_path / 'out.bin')
    ic.write_problem(prob, K, syn, crop, factor, **kw)
    subprocess.check_call([exe, prob, out])
    return ic.read_result(out, len(kw.get('sub_syn', ())))


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


# ---- points ----------------------------------------------------------------------------------------------------------
def test_points_equal_numpy_bit_for_bit(host_exe, tmp_path):
    K = ic.K_test()
    r = np.random.RandomState(5)
    full = (700 + 50 * r.rand(120, 160)).astype(np.float32)
    full[r.rand(120, 160) < 0.6] = 0
    full[0, 0], full[-1, -1] = 655.5, 733.25                       # first and last pixel are points
    odd = (690 + 30 * r.rand(37, 53)).astype(np.float32)
    odd[r.rand(37, 53) < 0.3] = 0
    odd[3, 3] = -2.0
    for syn, crop in ((full, odd), (np.zeros((120, 160), np.float32), odd), (full, np.zeros((37, 53), np.float32))):
        got = _run(host_exe, tmp_path, K, syn, crop, 1e9)           # a filter that keeps everything
        want_syn = ic.point_cloud(K, syn)
        assert got['n_syn'] == len(want_syn) and _same_bits(got['syn'], want_syn)
        if len(want_syn):
            want_real = ic.point_cloud(ic.crop_K(K, crop), crop)
            assert got['n_real'] == len(want_real) and _same_bits(got['real'], want_real)
            assert np.abs(got['stats'][:3] - want_syn.mean(axis=0)).max() < 1e-9
        else:
            assert got['n_real'] == 0                              # no centroid: nothing passes


def test_filter_keeps_what_the_reference_keeps(host_exe, tmp_path, golden):
    K = golden['K']
    for k in range(len(ic.CASES)):
        for variant, (factor, _, _) in ic.VARIANTS.items():
            syn_pts, centroid, radius, real_all, keep, dist = ic.prepare(K, golden['syn_%d' % k], golden['crop_%d' % k], factor)
            assert np.abs(dist - factor * radius).min() > 1e-6     # (the reference alone: nothing sits on the threshold)
            assert 0 < keep.sum() < len(real_all)                  # the strip and the negative pixel are there and go
            got = _run(host_exe, tmp_path, K, golden['syn_%d' % k], golden['crop_%d' % k], factor)
            assert got['n_syn'] == int(golden['n_syn_%d_%s' % (k, variant)]) and got['n_real'] == int(golden['n_real_%d_%s' % (k, variant)])
            assert _same_bits(got['real'], real_all[keep])
            assert abs(got['stats'][3] - radius) < 1e-9 and np.abs(got['stats'][:3] - centroid).max() < 1e-9


# ---- one step --------------------------------------------------------------------------------------------------------
def _check_step(got, syn_pts, real_pts, sub_syn, sub_real, label):
    A, B = syn_pts[sub_syn], real_pts[sub_real]
    d2, idx = ic.nearest(A, B)
    assert np.array_equal(got['idx'], idx), label                  # the lowest index of every tie
    assert _same_bits(got['d2'], d2), label
    assert _same_bits(B[got['idx']], B[idx]), label
    assert got['i'] == 0 and got['error'] == 0
    assert abs(got['mean_error'] - np.mean(np.sqrt(d2))) < 1e-12 * max(1.0, np.mean(np.sqrt(d2)))


@pytest.mark.parametrize('n', [3, 63, 64, 65, 257, 1000])
def test_single_step_matches_brute_force(host_exe, tmp_path, n):
    K = ic.K_test()
    syn, crop = ic.random_images(n, 1200, 1100)
    syn_pts, _, _, real_all, keep, _ = ic.prepare(K, syn, crop, 2.0)
    real_pts = real_all[keep]
    r = np.random.RandomState(n)
    sub_syn, sub_real = r.choice(len(syn_pts), n), r.choice(len(real_pts), n)
    sub_real[-1] = sub_real[0]                                     # a planted duplicate target, besides the drawn ones
    outs = [_run(host_exe, tmp_path, K, syn, crop, 2.0, sub_syn=sub_syn, sub_real=sub_real, max_iterations=1, order=o) for o in ORDERS]
    _check_step(outs[0], syn_pts, real_pts, sub_syn, sub_real, 'n = %d' % n)
    A, B = syn_pts[sub_syn], real_pts[sub_real][outs[0]['idx']]
    S = np.linalg.svd(np.dot((A - A.mean(axis=0)).T, B - B.mean(axis=0)))[1]
    R = outs[0]['T'][:3, :3]
    assert np.abs(R.dot(R.T) - np.eye(3)).max() < 1e-12 and abs(np.linalg.det(R) - 1) < 1e-12
    if S[1] - S[2] > 1e-6 * S[0]:                                  # the rotation is unique (not so for three points on two targets)
        assert np.abs(outs[0]['T'] - ic.best_fit_transform(A, B, 0)).max() < 1e-8
    else:
        assert n == 3
    for o in outs[1:]:                                             # whichever block finishes: the same bits
        for key in ('T', 'd2', 'src'):
            assert _same_bits(o[key], outs[0][key])
        assert np.array_equal(o['idx'], outs[0]['idx']) and o['mean_error'] == outs[0]['mean_error']


def test_exact_ties_take_the_lowest_index(host_exe, tmp_path):
    K, syn, crop = ic.tie_images()
    syn_pts, _, _, real_all, keep, _ = ic.prepare(K, syn, crop, 2.0)
    assert keep.all() and len(syn_pts) == 4 and len(real_all) == 8
    sub_syn = np.array([0, 1, 2, 3, 0, 2, 3, 1])
    sub_real = np.array([1, 0, 4, 3, 7, 6, 2, 5])                  # the mirror pairs (0, 1), (3, 4), (6, 7), the higher index first
    d2 = ic.dist2(syn_pts[sub_syn][:, None, :], real_all[sub_real][None, :, :])
    ties = (d2 == d2.min(axis=1, keepdims=True)).sum(axis=1)
    assert (ties >= 2).sum() >= 2                                  # the plant took: bit-identical distances to two targets
    got = _run(host_exe, tmp_path, K, syn, crop, 2.0, sub_syn=sub_syn, sub_real=sub_real, max_iterations=1)
    _check_step(got, syn_pts, real_all, sub_syn, sub_real, 'ties')


# ---- the rotation solve ----------------------------------------------------------------------------------------------
def test_rotation_solve_against_numpy_svd(tmp_path):
    """icp_rotation_from_H through a three-line program: random, rank-2 and reflection matrices against np.linalg.svd."""
    src = tmp_path / 'solve.cpp'
    src.write_text('#include <stdio.h>\n#include "%s"\nint main() { double H[9], R[9]; while (fread(H, 8, 9, stdin) == 9) { '
                   'aae_icp::icp_rotation_from_H(H, R); fwrite(R, 8, 9, stdout); } return 0; }\n'
                   % os.path.join(os.path.dirname(HERE), 'augmentedautoencoder_amd', 'csrc', 'kernels', 'icp_core.h'))
    exe = str(tmp_path / 'solve')
    subprocess.check_call([_compiler(), '-std=c++17', '-O2', '-ffp-contract=off', '-Wall', str(src), '-o', exe])
    r = np.random.RandomState(3)
    Hs = [r.randn(3, 3) * 10 ** r.uniform(-3, 5) for _ in range(40)]
    for _ in range(10):                                            # rank 2: coplanar clouds
        a, b = r.randn(50, 3), r.randn(50, 3)
        a[:, 2] = 0
        Hs.append(a.T.dot(b.dot(ic._axis_rotation(r.randn(3), 0.7))))
    for _ in range(10):                                            # reflection: det(V U^T) < 0
        U, _, Vt = np.linalg.svd(r.randn(3, 3))
        if np.linalg.det(Vt.T.dot(U.T)) > 0:
            U[:, 0] *= -1
        Hs.append(U.dot(np.diag([5.0, 2.0, 0.5])).dot(Vt))
    Hs.append(np.zeros((3, 3)))
    Hs.append(np.outer([1., 2., 3.], [3., -1., 2.]))               # rank 1: any rotation will do, but it must be one
    raw = subprocess.run([exe], input=np.array(Hs).tobytes(), stdout=subprocess.PIPE, check=True).stdout
    Rs = np.frombuffer(raw, np.float64).reshape(-1, 3, 3)
    assert len(Rs) == len(Hs)
    checked = 0
    for H, R in zip(Hs, Rs):
        assert np.abs(R.dot(R.T) - np.eye(3)).max() < 1e-12 and abs(np.linalg.det(R) - 1) < 1e-12
        U, S, Vt = np.linalg.svd(H)
        if S[0] == 0 or (S[1] - S[2]) < 1e-3 * S[0] or (S[0] - S[1]) < 1e-3 * S[0]:
            continue                                               # a repeated singular value: the rotation is not unique
        want = Vt.T.dot(U.T)
        if np.linalg.det(want) < 0:
            Vt[2] *= -1
            want = Vt.T.dot(U.T)
        assert np.abs(R - want).max() < 1e-12
        checked += 1
    assert checked >= 50


# ---- full refinements ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('variant', list(ic.VARIANTS))
@pytest.mark.parametrize('k', range(len(ic.CASES)))
def test_refinement_matches_golden_and_restatement(host_exe, tmp_path, golden, k, variant):
    K = golden['K']
    syn, crop = golden['syn_%d' % k], golden['crop_%d' % k]
    factor = ic.VARIANTS[variant][0]
    syn_pts, _, _, real_all, keep, _ = ic.prepare(K, syn, crop, factor)
    real_pts = real_all[keep]
    assert not len(real_pts) < len(syn_pts) / 8.
    rs = np.random.RandomState(int(golden['seed_%d' % k]))
    sub_real, sub_syn = ic.draw(rs, len(real_pts), len(syn_pts))
    assert np.array_equal(sub_real, golden['sub_real_%d_%s' % (k, variant)]) and np.array_equal(sub_syn, golden['sub_syn_%d_%s' % (k, variant)])
    for mode in ic.MODES:
        key = '%d_%s_%s' % (k, variant, mode)
        bits = ic.mode_bits(mode, variant)
        T, d2, idx, i, mean_error, margin = ic.icp(syn_pts[sub_syn], real_pts[sub_real], bits)
        assert margin > 1e-9                                       # (the reference alone: no iteration sits on the stop test)
        assert i == int(golden['iterations_' + key]) and np.abs(T - golden['T_' + key]).max() <= 1e-8
        pa, pb = np.random.RandomState(1).permutation(len(sub_syn)), np.random.RandomState(2).permutation(len(sub_syn))
        T_perm = ic.icp(syn_pts[sub_syn][pa], real_pts[sub_real][pb], bits)
        assert T_perm[3] == i and np.abs(T_perm[0] - T).max() < 1e-10       # (the reference alone: sums in another order do not move it)
        outs = [_run(host_exe, tmp_path, K, syn, crop, factor, bits=bits, sub_syn=sub_syn, sub_real=sub_real, order=o) for o in ORDERS]
        got = outs[0]
        print('%s: i = %d, |dT| vs golden %.3e, vs restatement %.3e' % (key, got['i'], np.abs(got['T'] - golden['T_' + key]).max(), np.abs(got['T'] - T).max()))
        assert got['i'] == int(golden['iterations_' + key]) == i
        assert np.abs(got['T'] - golden['T_' + key]).max() <= 1e-8
        assert np.abs(got['T'] - T).max() <= 1e-8
        assert abs(got['mean_error'] - float(golden['mean_error_' + key])) <= 1e-8
        R_ref, t_ref = ic.compose(got['T'], golden['R_est_%d' % k], golden['t_est_%d' % k], mode, variant)
        assert np.abs(R_ref - golden['R_refined_' + key]).max() <= 1e-8 and np.abs(t_ref - golden['t_refined_' + key]).max() <= 1e-6
        for o in outs[1:]:
            assert _same_bits(o['T'], got['T']) and o['i'] == got['i'] and _same_bits(o['src'], got['src'])


def test_too_few_points_is_decided_like_the_reference(host_exe, tmp_path, golden):
    K = golden['K']
    got = _run(host_exe, tmp_path, K, golden['syn_0'], golden['few_crop'], 2.0)
    syn_pts, _, _, real_all, keep, _ = ic.prepare(K, golden['syn_0'], golden['few_crop'], 2.0)
    assert got['n_real'] == int(keep.sum()) and got['n_syn'] == len(syn_pts)
    assert got['n_real'] < got['n_syn'] / 8.                       # icp_utils.py:264: the pose comes back unchanged


def test_bad_index_is_clamped_and_flagged(host_exe, tmp_path, golden):
    K = golden['K']
    sub = np.arange(10)
    bad = sub.copy()
    bad[4] = 10 ** 6
    got = _run(host_exe, tmp_path, K, golden['syn_0'], golden['crop_0'], 2.0, sub_syn=sub, sub_real=bad, max_iterations=2)
    assert got['error'] == 1 and np.isfinite(got['T']).all()
    got = _run(host_exe, tmp_path, K, golden['syn_0'], golden['crop_0'], 2.0, sub_syn=-bad, sub_real=sub, max_iterations=2)
    assert got['error'] == 1 and np.isfinite(got['T']).all()


def test_host_driver_under_sanitizers(tmp_path, golden):
    """address + undefined-behaviour sanitizers on the stand-alone driver: a full refinement per mode, an empty frame, a
    three-point problem, a clamped index, every block order."""
    exe = _build(tmp_path, ['-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all'], 'icp_host_san')
    K = golden['K']
    sub_real, sub_syn = golden['sub_real_1_eval'], golden['sub_syn_1_eval']
    for mode, order in zip(ic.MODES, ORDERS):
        got = _run(exe, tmp_path, K, golden['syn_1'], golden['crop_1'], 2.0, bits=ic.mode_bits(mode, 'm3'), sub_syn=sub_syn, sub_real=sub_real, order=order)
        assert np.isfinite(got['T']).all()
    _run(exe, tmp_path, K, np.zeros((120, 160), np.float32), golden['crop_1'], 2.0)
    _run(exe, tmp_path, K, golden['syn_1'], golden['crop_1'], 2.0, sub_syn=[0, 5, 9], sub_real=[1, 10 ** 7, -4], max_iterations=3)
