"""The estimator's opt-in depth refinement without a GPU: the switch (argument and [auto_pose] icp), what it asks its caller
for, and the depth window of a box (eval/eval_utils.py:104-117)."""
import configparser

import numpy as np

import test_pose_estimator as tpe
from augmentedautoencoder_amd.pose_estimator import AePoseEstimator


def _targs():
    targs = configparser.ConfigParser()
    targs.read_string(tpe.TRAIN_CFG.format(h=16, w=16))
    return targs


def test_icp_is_off_by_default_and_asks_for_depth_when_on():
    off = AePoseEstimator(codebooks={'a': object()}, train_args={'a': _targs()})
    assert 'depth_img' not in off.query_process_requirements() and off._icp is None
    handle = object()
    on = AePoseEstimator(codebooks={'a': object()}, train_args={'a': _targs()}, icp=handle)
    assert on.query_process_requirements()[-1] == 'depth_img' and on.icp_handle is handle


def test_depth_window_is_the_padded_square_clipped_to_the_image():
    depth = np.arange(480 * 640, dtype=np.float32).reshape(480, 640)
    for bb, pad in (([60.0, 50.0, 150.0, 140.0], 1.2), ([300.5, 40.25, 160.0, 150.0], 1.2), ([630.0, 470.0, 20.0, 20.0], 1.2), ([0.0, 0.0, 33.0, 71.5], 1.5)):
        x, y, w, h = bb
        size = int(np.maximum(h, w) * pad)                          # eval_utils.py:106-110, size / 2 as Python 2 divides an int
        left, right = int(np.max([x + w / 2 - size // 2, 0])), int(np.min([x + w / 2 + size // 2, 640]))
        top, bottom = int(np.max([y + h / 2 - size // 2, 0])), int(np.min([y + h / 2 + size // 2, 480]))
        got = AePoseEstimator.depth_crop(depth, bb, pad)
        assert np.array_equal(got, depth[top:bottom, left:right]) and got.size > 0
    assert AePoseEstimator.depth_crop(depth, [630.0, 470.0, 20.0, 20.0], 1.2).shape == (12, 12)
