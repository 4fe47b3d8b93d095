"""PoseVisualizer and Renderer.render_many without a GPU: what is read from the estimator, the arguments that are refused or
ignored, and the absence of a CPU fallback."""
import numpy as np
import pytest
import torch

import render_cases as rc
import render_reference as rr
from augmentedautoencoder_amd import meshrenderer as mr
from augmentedautoencoder_amd.pose_estimator import PoseEstimate
from augmentedautoencoder_amd.visualization import PoseVisualizer
from scene_cases import Estimator


def _models(tmp_path):
    out = []
    for name in ('box', 'torus'):
        path = str(tmp_path / (name + '.ply'))
        rr.write_ply(path, rc.model_dict(name))
        out.append((name, path))
    return out


def test_classes_paths_and_scale_are_read_as_the_reference_reads_them(tmp_path):
    models = _models(tmp_path)
    vis = PoseVisualizer(Estimator(models, vertex_scale=1000))
    assert vis.classes == ['box', 'torus'] and vis.ply_model_paths == [p for _, p in models]
    assert vis.vertex_scale == [1000] and vis.downsample == 1
    assert vis._renderer is None                                           # lazy: nothing is loaded yet
    r = vis.renderer
    assert r is vis.renderer and r.model == 'cad' and r.vertex_scale == 1000.0 and len(r._arrays) == 2
    assert len(r._arrays[0][3]) == 12 and r._meshes is None                 # the box's soup; no device state without a call


def test_refused_and_ignored_arguments(tmp_path):
    est = Estimator(_models(tmp_path))
    image = np.zeros((120, 160, 3), np.uint8)
    K = rr.scaled_K(160, 120)
    with pytest.raises(NotImplementedError, match='downsample'):
        PoseVisualizer(est, downsample=2).render_poses(image, K, [], [])
    with pytest.raises(NotImplementedError, match='all_pose_estimates_rgb'):
        PoseVisualizer(est).render_poses(image, K, [], [], all_pose_estimates_rgb=[])
    with pytest.raises(NotImplementedError, match='downsample'):
        PoseVisualizer(est, downsample=2).render_poses_batch([image], K, [[]])
    # nothing to draw: no renderer is needed; waitKey, vis_mask and depth_image change nothing, no window is opened
    vis = PoseVisualizer(est)
    image[:] = np.random.RandomState(3).randint(0, 256, image.shape)
    for kw in (dict(), dict(waitKey=False), dict(vis_mask=True), dict(depth_image=np.ones((120, 160), np.float32))):
        out = vis.render_poses(image, K, [], [], **kw)
        assert out is not image and out.dtype == np.uint8 and np.array_equal(out, image)
    assert vis._renderer is None
    with pytest.raises(ValueError, match='uint8'):
        vis.render_poses(image.astype(np.float32), K, [], [])
    with pytest.raises(ValueError, match='2 images'):
        vis.render_poses_batch([image, image], K, [[]])


def test_rendering_needs_the_gpu(tmp_path):
    if torch.cuda.is_available():
        pytest.skip('GPU present')
    models = _models(tmp_path)
    r = mr.Renderer([p for _, p in models], model='cad')
    with pytest.raises(RuntimeError, match='needs the GPU'):
        r.render_many([0, 1], 160, 120, rr.scaled_K(160, 120), [np.eye(3)] * 2, [np.array(rc.T0)] * 2, rc.NEAR, rc.FAR)
    with pytest.raises(RuntimeError, match='needs the GPU'):
        r.render_scenes([0], [0], 1, 160, 120, rr.scaled_K(160, 120), np.eye(3)[None], np.array([rc.T0]), rc.NEAR, rc.FAR)
    pose = PoseEstimate(name='torus', trafo=np.eye(4))
    with pytest.raises(RuntimeError, match='needs the GPU'):
        PoseVisualizer(Estimator(models)).render_poses(np.zeros((120, 160, 3), np.uint8), rr.scaled_K(160, 120), [pose], [])
