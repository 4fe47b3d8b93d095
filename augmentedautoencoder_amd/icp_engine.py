"""The depth ICP refinement behind ``icp.py`` (the reference's ``auto_pose/icp/icp.py``) and ``icp_utils.py``
(``auto_pose/eval/icp_utils.py``): one implementation over libaae_hip.so's ``aae_icp_*`` (csrc/kernels/icp_core.h states
what is computed).  The device does the point clouds, the filter and the ICP loop in float64; the host keeps what the
reference does with random numbers and 4x4 matrices: the too-few-points decision, the subsample draws (the real indices
first, then the synthetic ones, icp_utils.py:269-270) and the rejection and composition of the result (:289-303).

Deviations from the reference: among equidistant targets the nearest neighbour is the one with the lowest index (the
KD-tree answers any); a refinement that would run on fewer than 3 points returns the pose unchanged."""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib

N_SUB = 3000                                    # icp_utils.py:14 / icp.py:8
MAX_ITERATIONS = 100                            # icp_utils.py:96
TOLERANCE = 0.000001                            # icp_utils.py:273
NEAR, FAR = 10, 10000                           # icp_utils.py:206-207


class IcpEngine(object):
    """Workspace and calls of one device.  ``prepare`` then ``refine`` work on the same batch of up to 16 problems."""

    def __init__(self, device=None):
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError('the depth refinement needs the GPU (libaae_hip.so): there is no CPU fallback')
        self.lib = _lib.load()
        self._device = device if device is not None else torch.device('cuda', torch.cuda.current_device())
        self._ws = None
        self._shape = None
        self._counts = torch.empty((_lib.AAE_ICP_MAX_PROBLEMS, 2), dtype=torch.int32).pin_memory()

    def _stream(self):
        import torch
        return ctypes.c_void_p(torch.cuda.current_stream(self._device).cuda_stream)

    def _workspace(self, shape, fill=None):
        import torch
        need = int(self.lib.aae_icp_workspace_bytes(shape.n_problems, shape.max_points, shape.W, shape.H, shape.crop_w, shape.crop_h))
        if need == 0:
            raise ValueError('aae_icp_workspace_bytes: %d problems, %d points, frame %dx%d, crop %dx%d are outside what the kernels cover'
                             % (shape.n_problems, shape.max_points, shape.W, shape.H, shape.crop_w, shape.crop_h))
        if self._ws is None or self._ws.numel() - (-self._ws.data_ptr()) % 256 < need:
            self._ws = None
            self._ws = torch.empty(need + 256, dtype=torch.uint8, device=self._device)
        if fill is not None:
            self._ws.fill_(fill)
        return self._ws.data_ptr() + (-self._ws.data_ptr()) % 256, need

    def prepare(self, syn_depth, crops, K, factor, max_points=N_SUB, fill=None):
        """Steps 1-3 for P problems: syn_depth [P,H,W] float32 (device tensor or array), crops a list of P 2-d arrays ->
        counts int [P,2] (synthetic points, real points inside the filter).  Synchronises once, to read the counts."""
        import torch
        syn = torch.as_tensor(syn_depth).to(device=self._device, dtype=torch.float32).contiguous()
        if syn.dim() != 3 or len(crops) != syn.shape[0]:
            raise ValueError('%d crops for synthetic depth of shape %s' % (len(crops), tuple(syn.shape)))
        P, H, W = (int(v) for v in syn.shape)
        crops = [np.ascontiguousarray(c, dtype=np.float32) for c in crops]
        if any(c.ndim != 2 or c.size == 0 for c in crops):
            raise ValueError('a depth crop must be a non-empty 2-d array')
        crop_h, crop_w = max(c.shape[0] for c in crops), max(c.shape[1] for c in crops)
        slot = crop_h * crop_w                                         # every crop fits, dense, at the front of its slot
        shape = _lib.IcpShape(P, int(max_points), W, H, crop_w, crop_h)
        packed = np.zeros((P, slot), dtype=np.float32)
        for p, c in enumerate(crops):
            packed[p, :c.size] = c.reshape(-1)
        dims = np.array([c.shape for c in crops], dtype=np.int32)
        Kh = np.ascontiguousarray(np.asarray(K, dtype=np.float64).reshape(9))
        with torch.cuda.device(self._device):
            crop_dev = torch.as_tensor(packed, device=self._device)
            ws_ptr, ws_bytes = self._workspace(shape, fill)
            rc = self.lib.aae_icp_prepare(ctypes.byref(shape), ctypes.c_void_p(syn.data_ptr()), ctypes.c_void_p(crop_dev.data_ptr()),
                                          ctypes.c_void_p(dims.ctypes.data), ctypes.c_void_p(Kh.ctypes.data), float(factor),
                                          ctypes.c_void_p(self._counts.data_ptr()), ctypes.c_void_p(ws_ptr), ws_bytes, self._stream())
            _lib.check(self.lib, rc, 'aae_icp_prepare')
            torch.cuda.current_stream(self._device).synchronize()
        self._shape = shape
        return self._counts[:P].numpy().copy()

    def cloud(self, problem, what):
        """What prepare left for one problem: what = 0 synthetic points [n,3], 1 real points [n,3] (both up to capacity: cut
        them with the counts), 2 (centroid[3], largest distance, threshold)."""
        off, cap = ctypes.c_size_t(), ctypes.c_size_t()
        _lib.check(self.lib, self.lib.aae_icp_workspace_info(ctypes.byref(self._shape), int(problem), int(what), ctypes.byref(off), ctypes.byref(cap)),
                   'aae_icp_workspace_info')
        base = (-self._ws.data_ptr()) % 256 + off.value
        n = cap.value * (3 if what < 2 else 1)
        flat = self._ws[base:base + 8 * n].cpu().numpy().copy().view(np.float64)
        return flat.reshape(-1, 3) if what < 2 else flat

    def refine(self, n_points, sub_syn, sub_real, modes, max_iterations=MAX_ITERATIONS, tolerance=TOLERANCE, matches=False, timed=False):
        """Steps 5-6 on the prepared batch: n_points [P] (0 = leave the problem out), sub_syn / sub_real lists of index arrays,
        modes [P] AAE_ICP_* bits -> dict(T [P,4,4], iterations [P], mean_error [P]) and, with matches=True, the last iteration's
        d2 and idx [P,max_points]; timed=True adds kernel_ms (gather, the steps, finish).  An index outside its list raises
        ValueError (the device clamps it: nothing is read out of range)."""
        import torch
        shape = self._shape
        if shape is None:
            raise RuntimeError('refine() needs a prepare()d batch')
        P, M = shape.n_problems, shape.max_points
        n_points = np.ascontiguousarray(n_points, dtype=np.int32)
        modes_a = np.ascontiguousarray(modes, dtype=np.int32)
        if len(n_points) != P or len(modes_a) != P or len(sub_syn) != P or len(sub_real) != P:
            raise ValueError('refine(): %d problems were prepared' % P)
        idx = np.zeros((2, P, M), dtype=np.int32)
        for p in range(P):
            n = int(n_points[p])
            if n > M or len(sub_syn[p]) < n or len(sub_real[p]) < n:
                raise ValueError('problem %d: %d points, %d / %d indices, at most %d' % (p, n, len(sub_syn[p]), len(sub_real[p]), M))
            idx[0, p, :n] = np.clip(np.asarray(sub_syn[p][:n], dtype=np.int64), -1, 2 ** 31 - 1)     # (out of range stays out of range)
            idx[1, p, :n] = np.clip(np.asarray(sub_real[p][:n], dtype=np.int64), -1, 2 ** 31 - 1)
        with torch.cuda.device(self._device):
            idx_dev = torch.as_tensor(idx, device=self._device)
            T = torch.empty((P, 16), dtype=torch.float64, device=self._device)
            its = torch.empty((P,), dtype=torch.int32, device=self._device)
            err = torch.empty((P,), dtype=torch.float64, device=self._device)
            bad = torch.empty((P,), dtype=torch.int32, device=self._device)
            d2 = torch.zeros((P, M), dtype=torch.float64, device=self._device) if matches else None
            nn = torch.zeros((P, M), dtype=torch.int32, device=self._device) if matches else None
            ws_ptr = self._ws.data_ptr() + (-self._ws.data_ptr()) % 256
            ws_bytes = int(self.lib.aae_icp_workspace_bytes(P, M, shape.W, shape.H, shape.crop_w, shape.crop_h))
            args = (ctypes.byref(shape), ctypes.c_void_p(n_points.ctypes.data), ctypes.c_void_p(idx_dev[0].data_ptr()), ctypes.c_void_p(idx_dev[1].data_ptr()),
                    ctypes.c_void_p(modes_a.ctypes.data), int(max_iterations), float(tolerance), ctypes.c_void_p(T.data_ptr()), ctypes.c_void_p(its.data_ptr()),
                    ctypes.c_void_p(err.data_ptr()), ctypes.c_void_p(bad.data_ptr()), ctypes.c_void_p(d2.data_ptr()) if matches else None,
                    ctypes.c_void_p(nn.data_ptr()) if matches else None, ctypes.c_void_p(ws_ptr), ws_bytes, self._stream())
            out = {}
            if timed:
                ms = (ctypes.c_float * (int(max_iterations) + 2))()
                _lib.check(self.lib, self.lib.aae_icp_refine_timed(*(args + (ms,))), 'aae_icp_refine_timed')
                out['kernel_ms'] = list(ms)
            else:
                _lib.check(self.lib, self.lib.aae_icp_refine(*args), 'aae_icp_refine')
            bad_h = bad.cpu().numpy()
        if bad_h.any():
            raise ValueError('a subsample index of problem(s) %s lies outside its point list' % np.nonzero(bad_h)[0].tolist())
        out.update(T=T.cpu().numpy().reshape(P, 4, 4), iterations=its.cpu().numpy(), mean_error=err.cpu().numpy())
        if matches:
            out.update(d2=d2.cpu().numpy(), idx=nn.cpu().numpy())
        return out


def mode_bits(depth_only, no_depth, zero_translation):
    if depth_only:
        return _lib.AAE_ICP_DEPTH_ONLY                              # best_fit_transform tests depth_only first
    if no_depth:
        return _lib.AAE_ICP_NO_DEPTH | (_lib.AAE_ICP_NO_DEPTH_ZERO_T if zero_translation else 0)
    return 0


def rotation_angle(T):
    """|angle| of transform.rotation_from_matrix(T) (icp_utils.py:290): the cosine from the trace, the sine from the skew part"""
    R = np.asarray(T, dtype=np.float64)[:3, :3]
    cosa = (np.trace(R) - 1.0) / 2.0
    sina = 0.5 * np.sqrt((R[2, 1] - R[1, 2]) ** 2 + (R[0, 2] - R[2, 0]) ** 2 + (R[1, 0] - R[0, 1]) ** 2)
    return abs(np.arctan2(sina, cosa))


def icp_refinement_batch(engine, renderer, obj_id, depth_crops, R_ests, t_ests, K_test, test_render_dims, depth_only=False, no_depth=False,
                         max_mean_dist_factor=2.0, angle_change_limit=20 * np.pi / 180., zero_translation=False, rng=None):
    """icp_refinement for a list of detections of one object, 16 per call: [(R_refined, t_refined)].  rng: a RandomState
    (default: the global np.random), drawn per detection in order, and not at all for a detection with too few points."""
    rng = np.random if rng is None else rng
    W, H = (int(v) for v in test_render_dims[:2])
    bits = mode_bits(depth_only, no_depth, zero_translation)
    out = []
    for a in range(0, len(depth_crops), _lib.AAE_ICP_MAX_PROBLEMS):
        crops = depth_crops[a:a + _lib.AAE_ICP_MAX_PROBLEMS]
        Rs = [np.asarray(R, dtype=np.float64).reshape(3, 3) for R in R_ests[a:a + len(crops)]]
        ts = [np.asarray(t, dtype=np.float64).reshape(3) for t in t_ests[a:a + len(crops)]]
        # icp_utils.py:199-209: the model at R_est, t = (0, 0, t_z)
        syn = renderer.render_batch(obj_id, W, H, K_test, np.array(Rs), np.array([[0.0, 0.0, t[2]] for t in ts]), NEAR, FAR)[1]
        counts = engine.prepare(syn, crops, K_test, max_mean_dist_factor)
        n_points, sub_syn, sub_real = [], [], []
        for n_syn, n_real in counts:
            n = int(np.min([n_real, n_syn, N_SUB]))
            if n_real < n_syn / 8. or n < 3:                        # icp_utils.py:264 (and the stated deviation)
                n_points.append(0); sub_syn.append(()); sub_real.append(())
                continue
            sub_real.append(rng.choice(int(n_real), n))
            sub_syn.append(rng.choice(int(n_syn), n))
            n_points.append(n)
        if not any(n_points):
            out += list(zip(R_ests[a:a + len(crops)], t_ests[a:a + len(crops)]))
            continue
        res = engine.refine(n_points, sub_syn, sub_real, [bits] * len(crops))
        for p in range(len(crops)):
            if n_points[p] == 0:
                out.append((R_ests[a + p], t_ests[a + p]))
                continue
            T = res['T'][p]
            if no_depth and rotation_angle(T) > angle_change_limit:  # icp_utils.py:289-292
                T = np.eye(4)
            H_est = np.eye(4)
            H_est[:3, 3] = ts[p]
            H_est[:3, :3] = Rs[p]
            H_ref = np.dot(T, H_est)
            out.append((H_ref[:3, :3], H_ref[:3, 3]))
    return out
