"""``SynRenderer`` and ``icp_refinement`` with the signatures and constants of the reference's
``auto_pose/eval/icp_utils.py`` (the refinement ``eval/ae_eval.py:192-210`` runs per detection), backed by the HIP
rasteriser and the HIP ICP kernels (icp_engine.py)."""
from __future__ import annotations

import numpy as np

from . import icp_engine, meshrenderer
from .utils import lazy_property

N = icp_engine.N_SUB                                  # icp_utils.py:14
angle_change_limit = 20 * np.pi / 180.                # icp_utils.py:18


class SynRenderer(object):
    """icp_utils.py:178-234.  train_args: the training cfg; the model is [Paths] MODEL_PATH with [Dataset] MODEL replaced by
    'cad', rendered by the cad renderer.  ``model_path`` may also be given directly (a PLY path or a loaded model)."""

    def __init__(self, train_args=None, model_path=None):
        if model_path is None:
            MODEL_PATH = train_args.get('Paths', 'MODEL_PATH')
            self.model = train_args.get('Dataset', 'MODEL')
            model_path = MODEL_PATH.replace(self.model, 'cad')
        self.model_path = model_path
        self.renderer

    @lazy_property
    def renderer(self):
        return meshrenderer.Renderer([self.model_path], 1, '.', 1, model='cad')

    @lazy_property
    def engine(self):
        return icp_engine.IcpEngine()

    def generate_synthetic_depth(self, K_test, R_est, t_est, test_shape):
        """icp_utils.py:194-218: the point cloud of the model rendered at R_est, t = (0, 0, t_z), as float64 [n,3]"""
        W_test, H_test = test_shape[:2]
        depth = self.renderer.render_batch(0, W_test, H_test, K_test, np.asarray(R_est, dtype=np.float64).reshape(1, 3, 3),
                                           np.array([0, 0, t_est[2]], dtype=np.float64), icp_engine.NEAR, icp_engine.FAR)[1]
        n_syn = int(self.engine.prepare(depth, [np.ones((1, 1), np.float32)], K_test, 1.0)[0, 0])
        return self.engine.cloud(0, 0)[:n_syn]

    def render_trafo(self, K_test, R_est, t_est, test_shape, downSample=1):
        """icp_utils.py:220-234"""
        W_test, H_test = test_shape[:2]
        return self.renderer.render(obj_id=0, W=W_test, H=H_test, K=K_test, R=R_est, t=np.array(t_est), near=icp_engine.NEAR, far=icp_engine.FAR,
                                    random_light=False)[0]


def icp_refinement_batch(depth_crops, icp_renderer, R_ests, t_ests, K_test, test_render_dims, depth_only=False, no_depth=False,
                         max_mean_dist_factor=2.0, rng=None):
    """icp_refinement for lists of crops and poses of one object, 16 per call: [(R_refined, t_refined)]"""
    return icp_engine.icp_refinement_batch(icp_renderer.engine, icp_renderer.renderer, 0, depth_crops, R_ests, t_ests, K_test, test_render_dims,
                                           depth_only, no_depth, max_mean_dist_factor, angle_change_limit, False, rng)


def icp_refinement(depth_crop, icp_renderer, R_est, t_est, K_test, test_render_dims, depth_only=False, no_depth=False, max_mean_dist_factor=2.0,
                   rng=None):
    """icp_utils.py:248-305.  rng: a RandomState for the subsample (default: the global np.random, drawn in the reference's
    order and not at all when there are too few points)."""
    return icp_refinement_batch([depth_crop], icp_renderer, [R_est], [t_est], K_test, test_render_dims, depth_only, no_depth,
                                max_mean_dist_factor, rng)[0]
