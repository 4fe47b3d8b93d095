"""``ICP`` and ``SynRenderer`` with the signatures and constants of the reference's ``auto_pose/icp/icp.py`` and
``auto_pose/icp/renderer.py`` (the refinement of the m3 estimator, m3_interface/ae_pose_estimator.py:175-198), backed by the
HIP rasteriser and the HIP ICP kernels (icp_engine.py).  Against ``icp_utils``: factor 4.0, angle limit 0.35 rad, and
``no_depth`` drops the whole translation (icp.py:58-61)."""
from __future__ import annotations

import numpy as np

from . import icp_engine, meshrenderer
from .utils import lazy_property

N = icp_engine.N_SUB                                  # icp.py:8
max_mean_dist_factor = 4.0                            # icp.py:10
angle_change_limit = 0.35                             # icp.py:11


class SynRenderer(object):
    """icp/renderer.py:9-69.  all_train_args: one training cfg per class ([Paths] model_path, [Dataset] vertex_scale of the
    first); ``model_paths`` / ``vertex_scale`` may also be given directly."""

    def __init__(self, test_args=None, all_train_args=None, has_vertex_color=False, model_paths=None, vertex_scale=None):
        if model_paths is None:
            model_paths = [train_args.get('Paths', 'model_path') for train_args in all_train_args]
            vertex_scale = all_train_args[0].getint('Dataset', 'vertex_scale')
        self.model_paths = list(model_paths)
        self.has_vertex_color = has_vertex_color
        self.vertex_scale = 1 if vertex_scale is None else vertex_scale
        self.renderer

    @lazy_property
    def renderer(self):
        return meshrenderer.Renderer(self.model_paths, 1, '.', vertex_scale=self.vertex_scale, model='reconst' if self.has_vertex_color else 'cad')

    @lazy_property
    def engine(self):
        return icp_engine.IcpEngine()

    def generate_synthetic_depth(self, K_test, R_est, t_est, test_shape, clas_idx=0):
        """renderer.py:33-53: the point cloud of class clas_idx rendered at R_est, t = (0, 0, t_z), as float64 [n,3]"""
        W_test, H_test = test_shape[:2]
        depth = self.renderer.render_batch(clas_idx, W_test, H_test, K_test, np.asarray(R_est, dtype=np.float64).reshape(1, 3, 3),
                                           np.array([0, 0, t_est[2]], dtype=np.float64), icp_engine.NEAR, icp_engine.FAR)[1]
        n_syn = int(self.engine.prepare(depth, [np.ones((1, 1), np.float32)], K_test, 1.0)[0, 0])
        return self.engine.cloud(0, 0)[:n_syn]

    def render_trafo(self, K_test, R_est, t_est, test_shape, clas_idx=0):
        """renderer.py:55-69: (bgr, depth)"""
        W_test, H_test = test_shape[:2]
        return self.renderer.render(obj_id=clas_idx, W=W_test, H=H_test, K=K_test, R=R_est, t=t_est, near=icp_engine.NEAR, far=icp_engine.FAR,
                                    random_light=False)


class ICP(object):
    def __init__(self, test_args=None, all_train_args=None, syn_renderer=None):
        self.syn_renderer = syn_renderer if syn_renderer is not None else SynRenderer(test_args, all_train_args)

    def icp_refinement_batch(self, depth_crops, R_ests, t_ests, K_test, test_render_dims, depth_only=False, no_depth=False, clas_idx=0, rng=None):
        """icp_refinement for lists of crops and poses of one class, 16 per call: [(R_refined, t_refined)]"""
        return icp_engine.icp_refinement_batch(self.syn_renderer.engine, self.syn_renderer.renderer, clas_idx, depth_crops, R_ests, t_ests, K_test,
                                               test_render_dims, depth_only, no_depth, max_mean_dist_factor, angle_change_limit, True, rng)

    def icp_refinement(self, depth_crop, R_est, t_est, K_test, test_render_dims, depth_only=False, no_depth=False, clas_idx=0, rng=None):
        """icp.py:162-212.  rng: a RandomState for the subsample (default: the global np.random, drawn in the reference's order
        and not at all when there are too few points)."""
        return self.icp_refinement_batch([depth_crop], [R_est], [t_est], K_test, test_render_dims, depth_only, no_depth, clas_idx, rng)[0]
