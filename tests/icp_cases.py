"""The cases of the depth-refinement tests, shared by the CPU test (icp_core.h through tests/native/icp_host.cpp), the GPU
test (the kernels) and tests/golden/make_icp_golden.py: the depth images, the NumPy float64 restatement of the reference's
icp_refinement (eval/icp_utils.py and icp/icp.py, nearest neighbours by brute force with the lowest index on ties), and the
file format of the host driver."""
import functools
import os

import numpy as np

import render_cases as rc
import render_reference as rr

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'icp_golden.npz')

DEPTH_ONLY, NO_DEPTH, NO_DEPTH_ZERO_T = 1, 2, 4
MODES = ('plain', 'depth_only', 'no_depth')
# (max_mean_dist_factor, angle_change_limit, flag bits of no_depth): eval/icp_utils.py:17-18,60-61,248 and icp/icp.py:10-11,58-61
VARIANTS = {'eval': (2.0, 20 * np.pi / 180., NO_DEPTH), 'm3': (4.0, 0.35, NO_DEPTH | NO_DEPTH_ZERO_T)}
N_SUB = 3000                                    # icp_utils.py:14
TOLERANCE = 1e-6                                # icp_utils.py:273
MAX_ITERATIONS = 100                            # icp_utils.py:96
CROP_ROWS, CROP_COLS = 101, 117                 # odd and not square: shape[0] // 2 is the x centre, shape[1] // 2 the y centre
# Chosen so that the reference reproduces itself in every mode: with the points in another order its T moves by < 1e-10 (the
# test asserts it).  icp/icp.py's no_depth (rotation about the camera, no translation) never converges and on some views
# wanders chaotically -- T then moves by O(1) under a reordering, and nothing can be compared at 1e-8.
# (view of rc.rotations('torus'), t_z of the estimate, rotation of the "real" object about (1, 2, 3), its t, RandomState seed)
CASES = ((0, 700.0, 0.10, (4.0, -3.0, 712.0), 101), (2, 890.0, 0.06, (1.0, 1.0, 880.0), 202))


def mode_bits(mode, variant):
    return {'plain': 0, 'depth_only': DEPTH_ONLY, 'no_depth': VARIANTS[variant][2]}[mode]


def K_test():
    return np.asarray(rr.scaled_K(*rc.DIMS), dtype=np.float64)


def _axis_rotation(axis, angle):
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * Kx.dot(Kx)


def _render_depth(R, t):
    W, H = rc.DIMS
    return rr.render(rr.mesh_dict(rc.arrays('torus', 'cad')), 'cad', rr.scaled_K(W, H), R, np.asarray(t, dtype=np.float64), W, H, rc.NEAR, rc.FAR,
                     shade=False)['depth'].astype(np.float32)


@functools.lru_cache(maxsize=None)
def make_case(k):
    """(R_est, t_est, synthetic depth [H,W] f32, depth crop [101,117] f32) of case k, rendered by the float64 restatement of the
    rasteriser.  The crop is a window of a frame that shows the object turned and moved a little, cut so that the crop's
    principal point (rows // 2, cols // 2) lands on the frame's; it carries a far background strip and one negative pixel."""
    view, tz, angle, t_real, _ = CASES[k]
    R_est = rc.rotations('torus')[view]
    t_est = np.array([12.0, -7.0, tz])
    syn = _render_depth(R_est, (0.0, 0.0, tz))
    real = _render_depth(_axis_rotation((1, 2, 3), angle).dot(R_est), t_real)
    K = K_test()
    left, top = int(K[0, 2]) - CROP_ROWS // 2, int(K[1, 2]) - CROP_COLS // 2
    crop = np.ascontiguousarray(real[top:top + CROP_ROWS, left:left + CROP_COLS]).copy()
    assert crop.shape == (CROP_ROWS, CROP_COLS)
    crop[:, -3:] = 3000.0                                            # background the filter must remove
    crop[0, 0] = -5.0                                                # a negative pixel is a point too (depth != 0)
    return R_est, t_est, syn, crop


# ---- the reference, restated in NumPy float64 --------------------------------------------------------------------------
def point_cloud(K, depth):
    """misc.py:65-70"""
    vs, us = depth.nonzero()
    zs = depth[vs, us]
    xs = ((us - K[0, 2]) * zs) / float(K[0, 0])
    ys = ((vs - K[1, 2]) * zs) / float(K[1, 1])
    return np.array([xs, ys, zs]).T.astype(np.float64).reshape(-1, 3)


def crop_K(K, crop):
    Kc = np.array(K, dtype=np.float64)
    Kc[0, 2] = crop.shape[0] // 2                                    # icp_utils.py:256-257 (Python 2 division)
    Kc[1, 2] = crop.shape[1] // 2
    return Kc


def prepare(K, syn_depth, crop, factor):
    """icp_utils.py:249-261 -> (syn points, centroid, max_mean_dist, real points before the filter, kept mask, distances)"""
    syn = point_cloud(K, syn_depth)
    centroid = np.mean(syn, axis=0)
    radius = np.max(np.linalg.norm(syn - centroid, axis=1))
    real_all = point_cloud(crop_K(K, crop), crop)
    dist = np.linalg.norm(real_all - centroid, axis=1)
    return syn, centroid, radius, real_all, dist < factor * radius, dist


def dist2(a, b):
    d = a - b
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def nearest(src, dst):
    """brute force with icp_core.h's formula and key: (d2 [n], lowest index of the smallest d2 [n])"""
    d2 = dist2(src[:, None, :], dst[None, :, :])
    idx = np.argmin(d2, axis=1)                                      # first occurrence = lowest index
    return d2[np.arange(len(src)), idx], idx


def best_fit_transform(A, B, bits):
    """icp_utils.py:21-74 / icp/icp.py:18-69"""
    cA, cB = np.mean(A, axis=0), np.mean(B, axis=0)
    if bits & DEPTH_ONLY:
        R = np.eye(3)
        t = np.array([0, 0, (cB - cA)[2]])
    else:
        H = np.dot((A - cA).T, B - cB)
        U, S, Vt = np.linalg.svd(H)
        R = np.dot(Vt.T, U.T)
        if np.linalg.det(R) < 0:
            Vt[2, :] *= -1
            R = np.dot(Vt.T, U.T)
        t = cB - np.dot(R, cA)
        if bits & NO_DEPTH:
            t = np.array([0., 0., 0.]) if bits & NO_DEPTH_ZERO_T else np.array([t[0], t[1], 0.])
    T = np.identity(4)
    T[:3, :3] = R
    T[:3, 3] = t
    return T


def icp(A, B, bits, max_iterations=MAX_ITERATIONS, tolerance=TOLERANCE):
    """icp_utils.py:96-175 -> (T, d2 of the last iteration, indices of the last iteration, i, mean error, stop margins)"""
    src = np.ones((4, len(A)))
    src[:3] = A.T
    prev, margins = 0, []
    for i in range(max_iterations):
        d2, idx = nearest(src[:3].T, B)
        T = best_fit_transform(src[:3].T, B[idx], bits)
        src = np.dot(T, src)
        mean_error = np.mean(np.sqrt(d2))
        margins.append(abs(abs(prev - mean_error) - tolerance))
        if abs(prev - mean_error) < tolerance:
            break
        prev = mean_error
    return best_fit_transform(A, src[:3].T, bits), d2, idx, i, mean_error, min(margins)


def rotation_angle(T):
    """|angle| of transform.rotation_from_matrix(T): atan2(|sin|, cos) with cos from the trace"""
    R = T[:3, :3]
    cosa = (np.trace(R) - 1.0) / 2.0
    sina = 0.5 * np.sqrt((R[2, 1] - R[1, 2]) ** 2 + (R[0, 2] - R[2, 0]) ** 2 + (R[1, 0] - R[0, 1]) ** 2)
    return abs(np.arctan2(sina, cosa))


def compose(T, R_est, t_est, mode, variant):
    """icp_utils.py:289-303"""
    if mode == 'no_depth' and rotation_angle(T) > VARIANTS[variant][1]:
        T = np.eye(4)
    H = np.eye(4)
    H[:3, :3] = R_est
    H[:3, 3] = t_est
    Hr = np.dot(T, H)
    return Hr[:3, :3], Hr[:3, 3]


def draw(rng, n_real, n_syn):
    """icp_utils.py:269-270: the real indices first"""
    n = int(np.min([n_real, n_syn, N_SUB]))
    return rng.choice(n_real, n), rng.choice(n_syn, n)


# ---- tests/native/icp_host.cpp: problem file in, results out ----------------------------------------------------------------
def write_problem(path, K, syn, crop, factor, bits=0, sub_syn=(), sub_real=(), max_iterations=MAX_ITERATIONS, tolerance=TOLERANCE, order=0):
    H, W = syn.shape
    with open(path, 'wb') as f:
        f.write(np.array([W, H, crop.shape[0], crop.shape[1], bits, max_iterations, len(sub_syn), order], dtype=np.int32).tobytes())
        f.write(np.asarray(K, dtype=np.float64).reshape(9).tobytes())
        f.write(np.array([factor, tolerance], dtype=np.float64).tobytes())
        f.write(np.ascontiguousarray(syn, dtype=np.float32).tobytes())
        f.write(np.ascontiguousarray(crop, dtype=np.float32).tobytes())
        f.write(np.asarray(sub_syn, dtype=np.int32).tobytes())
        f.write(np.asarray(sub_real, dtype=np.int32).tobytes())


def read_result(path, n):
    raw = open(path, 'rb').read()
    out, o = {}, 0
    out['n_syn'], out['n_real'] = (int(v) for v in np.frombuffer(raw, np.int32, 2, o)); o += 8
    out['stats'] = np.frombuffer(raw, np.float64, 5, o); o += 40
    out['syn'] = np.frombuffer(raw, np.float64, out['n_syn'] * 3, o).reshape(-1, 3); o += out['n_syn'] * 24
    out['real'] = np.frombuffer(raw, np.float64, out['n_real'] * 3, o).reshape(-1, 3); o += out['n_real'] * 24
    if n:
        out['error'], out['i'] = (int(v) for v in np.frombuffer(raw, np.int32, 2, o)); o += 8
        out['mean_error'] = float(np.frombuffer(raw, np.float64, 1, o)[0]); o += 8
        out['T'] = np.frombuffer(raw, np.float64, 16, o).reshape(4, 4); o += 128
        out['d2'] = np.frombuffer(raw, np.float64, n, o); o += 8 * n
        out['idx'] = np.frombuffer(raw, np.int32, n, o); o += 4 * n
        out['src'] = np.frombuffer(raw, np.float64, 3 * n, o).reshape(-1, 3); o += 24 * n
    assert o == len(raw)
    return out


# ---- images whose point clouds are what a test wants ---------------------------------------------------------------------
def random_images(seed, n_pixels_syn, n_pixels_real, dims=rc.DIMS, crop_shape=(CROP_ROWS, CROP_COLS)):
    """A synthetic frame and a crop with that many nonzero pixels at random places, depths around 700: two clouds of the same
    size and place, so every real point passes the filter."""
    r = np.random.RandomState(seed)
    W, H = dims
    syn = np.zeros(H * W, dtype=np.float32)
    syn[r.choice(H * W, n_pixels_syn, replace=False)] = (700 + 40 * r.rand(n_pixels_syn)).astype(np.float32)
    crop = np.zeros(crop_shape[0] * crop_shape[1], dtype=np.float32)
    crop[r.choice(crop.size, n_pixels_real, replace=False)] = (705 + 40 * r.rand(n_pixels_real)).astype(np.float32)
    return syn.reshape(H, W), crop.reshape(crop_shape)


def tie_images():
    """Exact ties by symmetry: with K = (f, 0, 4; 0, f, 4) the synthetic frame and the crop (9 x 9: centre 4, 4) share their
    pixel grid; the sources sit on the middle column and row, the targets are mirror pairs at the same depth, so each source
    has two targets at bit-identical distance (squares of +-dx are equal)."""
    K = np.array([[500., 0., 4.], [0., 500., 4.], [0., 0., 1.]])
    syn = np.zeros((9, 9), dtype=np.float32)
    crop = np.zeros((9, 9), dtype=np.float32)
    syn[1, 4] = syn[4, 4] = syn[7, 4] = 640.0
    syn[4, 1] = 640.0
    for v in (1, 4, 7):
        crop[v, 2] = crop[v, 6] = 641.0                              # mirror pair about the column of the sources
    crop[2, 1] = crop[6, 1] = 641.0                                  # ... and about the row of the source at (4, 1)
    return K, syn, crop
