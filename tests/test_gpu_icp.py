"""The depth refinement on the GPU (aae_icp_* through icp_engine.IcpEngine, icp_utils and icp) against NumPy, the float64
restatement of tests/icp_cases.py and the golden recorded from the reference's own code.  tests/test_icp_cpu.py makes the
same assertions on the host driver of the same arithmetic, so "equal to NumPy bit for bit" here is parity with that driver.

Bounds.  Integers (counts, matched indices, iteration counts) and squared distances: bitwise.  T: 1e-8 per entry against the
golden and the restatement (sums in another order move it by <= 2e-11 on these inputs; the stop test resolves 1e-6).  The mean
error is a mean of n square roots, each within 1 ulp, summed in another order: n * 2^-52 relative."""
import numpy as np
import pytest

import icp_cases as ic
import render_cases as rc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def engine():
    from augmentedautoencoder_amd import icp_engine
    return icp_engine.IcpEngine()


@pytest.fixture(scope='module')
def golden():
    return dict(np.load(ic.GOLDEN))


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def test_points_equal_numpy_bit_for_bit(engine):
    K = ic.K_test()
    r = np.random.RandomState(5)
    full = (700 + 50 * r.rand(120, 160)).astype(np.float32)
    full[r.rand(120, 160) < 0.6] = 0
    full[0, 0], full[-1, -1] = 655.5, 733.25
    odd = (690 + 30 * r.rand(37, 53)).astype(np.float32)
    odd[r.rand(37, 53) < 0.3] = 0
    odd[3, 3] = -2.0
    syns = np.stack([full, np.zeros_like(full), full])
    crops = [odd, odd, np.zeros((5, 9), np.float32)]                # three problems of different crop sizes in one call
    counts = engine.prepare(syns, crops, K, 1e9, fill=0xA5)
    want_syn = ic.point_cloud(K, full)
    want_real = ic.point_cloud(ic.crop_K(K, odd), odd)
    assert counts.tolist() == [[len(want_syn), len(want_real)], [0, 0], [len(want_syn), 0]]
    for p in (0, 2):
        assert _same_bits(engine.cloud(p, 0)[:len(want_syn)], want_syn)
        st = engine.cloud(p, 2)
        assert np.abs(st[:3] - want_syn.mean(axis=0)).max() < 1e-9
        assert abs(st[3] - np.linalg.norm(want_syn - want_syn.mean(axis=0), axis=1).max()) < 1e-9
    assert _same_bits(engine.cloud(0, 1)[:len(want_real)], want_real)


def test_filter_keeps_what_the_reference_keeps(engine, golden):
    K = golden['K']
    for variant, (factor, _, _) in ic.VARIANTS.items():
        counts = engine.prepare(np.stack([golden['syn_0'], golden['syn_1'], golden['syn_0']]), [golden['crop_0'], golden['crop_1'], golden['few_crop']],
                                K, factor)
        for p, k in ((0, 0), (1, 1)):
            _, _, _, real_all, keep, _ = ic.prepare(K, golden['syn_%d' % k], golden['crop_%d' % k], factor)
            assert counts[p].tolist() == [int(golden['n_syn_%d_%s' % (k, variant)]), int(golden['n_real_%d_%s' % (k, variant)])]
            assert _same_bits(engine.cloud(p, 1)[:counts[p, 1]], real_all[keep])
        assert counts[2, 1] < counts[2, 0] / 8.                     # the too-few-points decision (icp_utils.py:264)


def _one_step(engine, K, syn, crop, sub_syn, sub_real):
    counts = engine.prepare(syn[None], [crop], K, 2.0, max_points=max(3, len(sub_syn)))
    syn_pts, _, _, real_all, keep, _ = ic.prepare(K, syn, crop, 2.0)
    assert counts[0].tolist() == [len(syn_pts), int(keep.sum())]
    n = len(sub_syn)
    out = engine.refine([n], [sub_syn], [sub_real], [0], max_iterations=1, matches=True)
    A, B = syn_pts[sub_syn], real_all[keep][sub_real]
    d2, idx = ic.nearest(A, B)
    assert np.array_equal(out['idx'][0, :n], idx)                   # the lowest index of every tie
    assert _same_bits(out['d2'][0, :n], d2)
    assert int(out['iterations'][0]) == 0
    mean = np.mean(np.sqrt(d2))
    assert abs(out['mean_error'][0] - mean) <= n * 2.0 ** -52 * mean
    R = out['T'][0][:3, :3]
    assert np.abs(R.dot(R.T) - np.eye(3)).max() < 1e-12
    S = np.linalg.svd(np.dot((A - A.mean(axis=0)).T, B[idx] - B[idx].mean(axis=0)))[1]
    if S[1] - S[2] > 1e-6 * S[0]:
        assert np.abs(out['T'][0] - ic.best_fit_transform(A, B[idx], 0)).max() < 1e-8
    return out, d2


@pytest.mark.parametrize('n', [3, 63, 64, 65, 257, 1000, 3000])
def test_single_step_matches_brute_force(engine, n):
    """3000: the targets of one problem fill 72 KB of LDS and 47 blocks take tickets in two levels"""
    syn, crop = ic.random_images(n, 3500 if n > 1000 else 1200, 3400 if n > 1000 else 1100)
    r = np.random.RandomState(n)
    sub_syn, sub_real = r.choice(int((syn != 0).sum()), n), r.choice(int((crop != 0).sum()), n)
    sub_real[-1] = sub_real[0]
    _one_step(engine, ic.K_test(), syn, crop, sub_syn, sub_real)


def test_exact_ties_take_the_lowest_index(engine):
    K, syn, crop = ic.tie_images()
    sub_syn = np.array([0, 1, 2, 3, 0, 2, 3, 1])
    sub_real = np.array([1, 0, 4, 3, 7, 6, 2, 5])
    _, d2 = _one_step(engine, K, syn, crop, sub_syn, sub_real)


def _refine_case(engine, golden, k, variant, modes, fill=None):
    K = golden['K']
    factor = ic.VARIANTS[variant][0]
    P = len(modes)
    engine.prepare(np.stack([golden['syn_%d' % k]] * P), [golden['crop_%d' % k]] * P, K, factor, fill=fill)
    sub_syn, sub_real = golden['sub_syn_%d_%s' % (k, variant)], golden['sub_real_%d_%s' % (k, variant)]
    return engine.refine([len(sub_syn)] * P, [sub_syn] * P, [sub_real] * P, [ic.mode_bits(m, variant) for m in modes])


@pytest.mark.parametrize('variant', list(ic.VARIANTS))
@pytest.mark.parametrize('k', range(len(ic.CASES)))
def test_refinement_matches_golden(engine, golden, k, variant):
    out = _refine_case(engine, golden, k, variant, ic.MODES)
    for p, mode in enumerate(ic.MODES):
        key = '%d_%s_%s' % (k, variant, mode)
        print('%s: i = %d (golden %d), |dT| %.3e' % (key, out['iterations'][p], golden['iterations_' + key], np.abs(out['T'][p] - golden['T_' + key]).max()))
        assert int(out['iterations'][p]) == int(golden['iterations_' + key])
        assert np.abs(out['T'][p] - golden['T_' + key]).max() <= 1e-8
        n = len(golden['sub_syn_%d_%s' % (k, variant)])
        assert abs(out['mean_error'][p] - float(golden['mean_error_' + key])) <= 1e-8 + n * 2.0 ** -52 * float(golden['mean_error_' + key])


def test_batch_equals_single_calls_garbage_and_twice(engine, golden):
    """P = 3 problems of different n and iteration counts (12, 13 and 99) in one call: the bits of the three single calls;
    the same into a workspace filled with 0xA5; the same again."""
    K = golden['K']
    specs = [(0, 'eval', 'depth_only'), (1, 'eval', 'depth_only'), (0, 'm3', 'no_depth')]
    singles = [_refine_case(engine, golden, k, v, [m]) for k, v, m in specs[:2]]
    # one factor per prepare call: the m3 problem runs on its own indices but is prepared with the batch's factor
    syns = np.stack([golden['syn_%d' % k] for k, _, _ in specs])
    crops = [golden['crop_%d' % k] for k, _, _ in specs]
    sub_syn = [golden['sub_syn_%d_eval' % k] for k, _, _ in specs]
    sub_real = [golden['sub_real_%d_eval' % k] for k, _, _ in specs]
    modes = [ic.mode_bits(m, v) for _, v, m in specs]
    n = [len(s) for s in sub_syn]
    engine.prepare(syns[2:], crops[2:], K, 2.0)
    singles.append(engine.refine(n[2:], sub_syn[2:], sub_real[2:], modes[2:]))
    assert len(set(n)) > 1 and sorted(int(s['iterations'][0]) for s in singles) == [12, 13, 99]
    runs = []
    for fill in (None, 0xA5, None):
        engine.prepare(syns, crops, K, 2.0, fill=fill)
        runs.append(engine.refine(n, sub_syn, sub_real, modes, matches=True))
    for run in runs:
        for p, single in enumerate(singles):
            assert _same_bits(run['T'][p], single['T'][0]) and run['iterations'][p] == single['iterations'][0]
            assert _same_bits(run['mean_error'][p], single['mean_error'][0])
        assert _same_bits(run['d2'], runs[0]['d2']) and np.array_equal(run['idx'], runs[0]['idx'])


def test_left_out_problem_and_bad_arguments(engine, golden):
    K = golden['K']
    engine.prepare(np.stack([golden['syn_0'], golden['syn_1']]), [golden['crop_0'], golden['crop_1']], K, 2.0)
    sub = np.arange(50)
    out = engine.refine([0, 50], [(), sub], [(), sub], [0, 0], max_iterations=3)
    assert np.array_equal(out['T'][0], np.eye(4)) and out['iterations'].tolist() == [-1, 2]
    with pytest.raises(ValueError):
        engine.refine([2, 50], [sub, sub], [sub, sub], [0, 0])      # n < 3
    with pytest.raises(ValueError):
        engine.refine([50, 50], [sub, sub], [sub, sub], [0, 64])    # unknown mode bit


def test_bad_index_raises_and_reads_nothing_out_of_range(engine, golden):
    K = golden['K']
    engine.prepare(golden['syn_0'][None], [golden['crop_0']], K, 2.0)
    sub = np.arange(40)
    for bad in (10 ** 6, -1, int(golden['n_real_0_eval'])):
        idx = sub.copy()
        idx[7] = bad
        with pytest.raises(ValueError, match='outside its point list'):
            engine.refine([40], [sub], [idx], [0], max_iterations=2)
    out = engine.refine([40], [sub], [sub], [0], max_iterations=2)   # the run ends clean: the next call is fine
    assert np.isfinite(out['T']).all()


# ---- end to end: the public functions through the GPU rasteriser -----------------------------------------------------------
def _expected(K, syn_depth, crop, R_est, t_est, mode, variant, seed):
    factor = ic.VARIANTS[variant][0]
    syn_pts, _, _, real_all, keep, _ = ic.prepare(K, syn_depth, crop, factor)
    sub_real, sub_syn = ic.draw(np.random.RandomState(seed), int(keep.sum()), len(syn_pts))
    T = ic.icp(syn_pts[sub_syn], real_all[keep][sub_real], ic.mode_bits(mode, variant))[0]
    return ic.compose(T, R_est, t_est, mode, variant)


def test_public_functions_end_to_end(golden):
    """icp_utils.icp_refinement and ICP.icp_refinement with a seeded rng.  The synthetic depth is the GPU rasteriser's: where
    it equals the golden's frame bit for bit the golden's poses are the expectation, and in any case the restatement run on
    the depth the rasteriser gave."""
    from augmentedautoencoder_amd import icp as icp_m3, icp_utils
    K, dims = golden['K'], tuple(int(v) for v in golden['dims'])
    model = rc.model_dict('torus')
    ev = icp_utils.SynRenderer(model_path=model)
    m3 = icp_m3.ICP(syn_renderer=icp_m3.SynRenderer(model_paths=[model], vertex_scale=1))
    k = 1
    R_est, t_est, crop, seed = golden['R_est_%d' % k], golden['t_est_%d' % k], golden['crop_%d' % k], int(golden['seed_%d' % k])
    depth = ev.renderer.render(0, dims[0], dims[1], K, R_est, np.array([0, 0, t_est[2]]), 10, 10000)[1]
    same_frame = np.array_equal(depth, golden['syn_%d' % k])
    print('GPU synthetic depth equals the golden frame: %s' % same_frame)
    pts = ev.generate_synthetic_depth(K, R_est, t_est, dims)
    assert _same_bits(pts, ic.point_cloud(K, depth))
    for mode in ic.MODES:
        flags = dict(depth_only=(mode == 'depth_only'), no_depth=(mode == 'no_depth'))
        for variant, call in (('eval', lambda rng: icp_utils.icp_refinement(crop, ev, R_est, t_est, K, dims, rng=rng, **flags)),
                              ('m3', lambda rng: m3.icp_refinement(crop, R_est, t_est, K, dims, rng=rng, **flags))):
            R_ref, t_ref = call(np.random.RandomState(seed))
            R_want, t_want = _expected(K, depth, crop, R_est, t_est, mode, variant, seed)
            assert np.abs(R_ref - R_want).max() <= 1e-8 and np.abs(t_ref - t_want).max() <= 1e-6, (mode, variant)
            if same_frame:
                key = '%d_%s_%s' % (k, variant, mode)
                assert np.abs(R_ref - golden['R_refined_' + key]).max() <= 1e-8 and np.abs(t_ref - golden['t_refined_' + key]).max() <= 1e-6
    # the global generator is the default, drawn in the reference's order
    np.random.seed(seed)
    R_ref, t_ref = icp_utils.icp_refinement(crop, ev, R_est, t_est, K, dims)
    R_want, t_want = _expected(K, depth, crop, R_est, t_est, 'plain', 'eval', seed)
    assert np.abs(R_ref - R_want).max() <= 1e-8 and np.abs(t_ref - t_want).max() <= 1e-6
    # too few points: the inputs come back and no random number is drawn
    rng = np.random.RandomState(9)
    before = rng.get_state()[1].copy()
    R0, t0 = golden['R_est_0'], golden['t_est_0']
    R_ref, t_ref = icp_utils.icp_refinement(golden['few_crop'], ev, R0, t0, K, dims, rng=rng)
    assert R_ref is R0 and t_ref is t0 and np.array_equal(before, rng.get_state()[1])
    # the batched form: the single calls, in order, on one generator
    rng_a, rng_b = np.random.RandomState(3), np.random.RandomState(3)
    crops = [golden['crop_0'], golden['few_crop'], golden['crop_1']]
    Rs, ts = [R0, R0, R_est], [t0, t0, t_est]
    batch = icp_utils.icp_refinement_batch(crops, ev, Rs, ts, K, dims, depth_only=True, rng=rng_a)
    for (Rb, tb), c, R, t in zip(batch, crops, Rs, ts):
        Rs1, ts1 = icp_utils.icp_refinement(c, ev, R, t, K, dims, depth_only=True, rng=rng_b)
        assert _same_bits(Rb, Rs1) and _same_bits(tb, ts1)


class _StoredDepth(object):
    """stands where meshrenderer.Renderer stands: hands out a stored synthetic depth frame for every requested view"""

    def __init__(self, depth):
        self.depth = depth

    def render_batch(self, obj_id, W, H, K, Rs, ts, near, far, **kw):
        assert (H, W) == self.depth.shape and (near, far) == (10, 10000)
        return None, np.stack([self.depth] * len(Rs))


@pytest.mark.parametrize('k', range(len(ic.CASES)))
def test_public_functions_against_the_golden(golden, k):
    """The golden's R_refined / t_refined for every variant and mode, always: the public functions run on the golden's own
    synthetic frame (a stored-depth renderer), with the global generator seeded as the recording seeded it."""
    from augmentedautoencoder_amd import icp as icp_m3, icp_utils
    K, dims = golden['K'], tuple(int(v) for v in golden['dims'])
    model = rc.model_dict('torus')
    ev = icp_utils.SynRenderer(model_path=model)
    m3r = icp_m3.SynRenderer(model_paths=[model], vertex_scale=1)
    ev.__dict__['renderer'] = m3r.__dict__['renderer'] = _StoredDepth(golden['syn_%d' % k])
    m3 = icp_m3.ICP(syn_renderer=m3r)
    R_est, t_est, crop, seed = golden['R_est_%d' % k], golden['t_est_%d' % k], golden['crop_%d' % k], int(golden['seed_%d' % k])
    for mode in ic.MODES:
        flags = dict(depth_only=(mode == 'depth_only'), no_depth=(mode == 'no_depth'))
        for variant in ic.VARIANTS:
            np.random.seed(seed)
            if variant == 'eval':
                R_ref, t_ref = icp_utils.icp_refinement(crop, ev, R_est, t_est, K, dims, **flags)
            else:
                R_ref, t_ref = m3.icp_refinement(crop, R_est, t_est, K, dims, **flags)
            key = '%d_%s_%s' % (k, variant, mode)
            assert np.abs(R_ref - golden['R_refined_' + key]).max() <= 1e-8, key
            assert np.abs(t_ref - golden['t_refined_' + key]).max() <= 1e-6, key     # (t in mm: 1e-8 of the rotation times |t| < 1000, rounded up)


# ---- the estimator: icp=True is the per-detection sequence of public calls ----------------------------------------------------
def test_estimator_with_icp_equals_the_public_sequence():
    """Two classes x (1, 2) boxes.  process(..., depth_img) of an estimator built with icp= takes, per class, ICP along z ->
    the translation again with depth_pred -> rotation ICP (eval/ae_eval.py:192-210); the expectation is that sequence written
    with the public per-detection calls, the class's first steps before its second ones (the order the random draws take).
    With icp=False (the default) depth_img changes nothing."""
    import configparser

    import torch

    import test_pose_estimator as tpe
    from augmentedautoencoder_amd import icp as icp_m3, session as S
    from augmentedautoencoder_amd.codebook import Codebook
    from augmentedautoencoder_amd.dataset import Dataset
    from augmentedautoencoder_amd.encoder import Encoder
    from augmentedautoencoder_amd.pose_estimator import AePoseEstimator, BoundingBox
    from oracle import synth

    S.reset_default_graph()
    targs = configparser.ConfigParser()
    targs.read_string(tpe.TRAIN_CFG.format(h=128, w=128).replace('MIN_N_VIEWS: 12', 'MIN_N_VIEWS: 162').replace('NUM_CYCLO: 6', 'NUM_CYCLO: 36'))
    codebooks, train_args = {}, {}
    for k, name in enumerate(['obj_a', 'obj_b']):
        ds = Dataset('', h=128, w=128, c=3, min_n_views=162, radius=700, num_cyclo=36)
        with S.variable_scope(name):
            enc = Encoder(S.Placeholder((128, 128, 3)), 128, synth.DEFAULT_NUM_FILTER, 5, [2, 2, 2, 2], False)
            cb = Codebook(enc, ds, True)
        enc.load_weights(synth.make_weights(seed=50 + k))
        E = synth.make_codebook(ds.embedding_size, 128, seed=60 + k, planted_duplicates=8)
        cb.assign_embedding(E)
        rng = np.random.default_rng(70 + k)
        cb.assign_obj_bbs(np.stack([rng.integers(250, 350, len(E)), rng.integers(180, 260, len(E)), rng.integers(80, 200, len(E)), rng.integers(80, 200, len(E))], 1))
        codebooks[name], train_args[name] = cb, targs
    handle = icp_m3.ICP(syn_renderer=icp_m3.SynRenderer(model_paths=[rc.model_dict('torus'), rc.model_dict('box')], vertex_scale=1))
    plain = AePoseEstimator(codebooks=codebooks, train_args=train_args)
    est = AePoseEstimator(codebooks=codebooks, train_args=train_args, icp=handle)
    assert 'depth_img' in est.query_process_requirements() and 'depth_img' not in plain.query_process_requirements()

    W, H = 640, 480
    img = tpe._scene(9, H, W)
    camK = np.array([[1075.65, 0, 320.0], [0, 1073.9, 240.0], [0, 0, 1]])
    raw = [('obj_a', [60.0, 50.0, 150.0, 140.0]), ('obj_b', [300.5, 40.25, 160.0, 150.0]), ('obj_b', [330.0, 260.0, 170.5, 160.0])]
    dets = [BoundingBox(xmin=x / W, xmax=(x + w) / W, ymin=y / H, ymax=(y + h) / H, classes={c: 1.0}) for c, (x, y, w, h) in raw]
    bbs = [[b.xmin * W, b.ymin * H, (b.xmax - b.xmin) * W, (b.ymax - b.ymin) * H] for b in dets]
    rgb = plain.process(dets, img, camK, mm=True)
    assert len(rgb) == 3

    # a depth frame that shows, in every box's window, the class's model at the RGB rotation, 6 mm behind the RGB depth,
    # centred where the refinement puts the window's principal point
    order = ['obj_a', 'obj_b']
    depth = np.zeros((H, W), dtype=np.float32)
    for (c, _), bb, pose in zip(raw, bbs, rgb):
        size = int(np.maximum(bb[3], bb[2]) * 1.2)
        left, top = int(max(bb[0] + bb[2] / 2. - size // 2, 0)), int(max(bb[1] + bb[3] / 2. - size // 2, 0))
        win = AePoseEstimator.depth_crop(depth, bb, 1.2)
        Kw = camK.copy()
        Kw[0, 2], Kw[1, 2] = left + win.shape[0] // 2, top + win.shape[1] // 2
        frame = handle.syn_renderer.renderer.render(order.index(c), W, H, Kw, pose.trafo[:3, :3], np.array([0, 0, pose.trafo[2, 3] + 6.0]), 10, 10000)[1]
        depth[top:top + win.shape[0], left:left + win.shape[1]] = frame[top:top + win.shape[0], left:left + win.shape[1]]

    np.random.seed(11)
    got = est.process(dets, img, camK, depth_img=depth, mm=True)
    assert [g.name for g in got] == [c for c, _ in raw]

    np.random.seed(11)
    img_dev = torch.from_numpy(img).cuda()
    want = {}
    for ci, clas in enumerate(order):
        cb = codebooks[clas]
        members = [j for j, (c, _) in enumerate(raw) if c == clas]
        crops = {j: est.extract_square_patches(img_dev, [bbs[j]], 1.2, resize=(128, 128)) for j in members}
        first = {}
        for j in members:
            R, t = cb.auto_pose6d(None, crops[j], bbs[j], camK, 1, targs)
            assert np.array_equal(R.squeeze(), rgb[j].trafo[:3, :3])
            first[j] = handle.icp_refinement(AePoseEstimator.depth_crop(depth, bbs[j], 1.2), R.squeeze(), t.squeeze(), camK, (W, H), depth_only=True, clas_idx=ci)
        for j in members:
            _, ts = cb.auto_pose6d(None, crops[j], bbs[j], camK, 1, targs, depth_pred=first[j][1][2])
            R2, _ = handle.icp_refinement(AePoseEstimator.depth_crop(depth, bbs[j], 1.2), first[j][0], ts.squeeze(), camK, (W, H), no_depth=True, clas_idx=ci)
            want[j] = (R2, ts.squeeze())
    moved = 0
    for j, g in enumerate(got):
        assert _same_bits(g.trafo[:3, :3], want[j][0]) and _same_bits(g.trafo[:3, 3], want[j][1])
        moved += int(not np.array_equal(g.trafo, rgb[j].trafo))
    print('%d of 3 detections moved by the refinement' % moved)
    assert moved >= 1                                               # the refinement ran on real points

    # off by default: the depth image is not looked at
    off = plain.process(dets, img, camK, depth_img=depth, mm=True)
    assert all(a.name == b.name and np.array_equal(a.trafo, b.trafo) for a, b in zip(off, rgb))
    assert AePoseEstimator.depth_crop(depth, [630.0, 470.0, 20.0, 20.0], 1.2).shape == (12, 12)      # the padded square (24), clipped to the image
