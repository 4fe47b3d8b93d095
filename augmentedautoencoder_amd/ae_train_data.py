"""``ae_train_data <group/experiment> [--seed N] [--batch 256]`` -- render the training set of an experiment on the GPU and
write it where the reference's ``ae_train`` looks for it first (auto_pose/ae/ae_train.py:60-76 ->
dataset.py:82-95: ``<workspace>/tmp_datasets/<md5 of the cfg's [Dataset] and [Paths] items>.npz`` with train_x, mask_x,
train_y).  Nothing is trained.  The images are the HIP rasteriser's (meshrenderer.py), not an OpenGL driver's."""
from __future__ import annotations

import argparse
import configparser
import os
import time

import numpy as np

from . import ae_factory as factory
from . import utils as u


def _parse(argv):
    ap = argparse.ArgumentParser(prog='ae_train_data')
    ap.add_argument('experiment_name', help='<group>/<name> or <name>')
    ap.add_argument('--seed', type=int, default=None, help='seed of np.random (rotations, lights, offsets); default: unseeded, as the reference')
    ap.add_argument('--batch', type=int, default=256, help='training pairs per GPU call')
    opts = ap.parse_args(argv)
    if opts.batch < 1:
        ap.error('--batch must be at least 1')
    return opts


def main(argv=None):
    workspace = os.environ.get('AE_WORKSPACE_PATH')
    if workspace is None:
        raise SystemExit('Please define a workspace path:\nexport AE_WORKSPACE_PATH=/path/to/workspace')
    opts = _parse(argv)
    group, _, name = opts.experiment_name.rpartition('/')
    group = group.rsplit('/', 1)[-1]

    cfg_path = u.get_config_file_path(workspace, name, group)
    if not os.path.exists(cfg_path):
        raise SystemExit('Could not find config file:\n%s' % cfg_path)
    args = configparser.ConfigParser()
    args.read(cfg_path)
    dataset_path = u.get_dataset_path(workspace)
    os.makedirs(dataset_path, exist_ok=True)

    dataset = factory.build_dataset(dataset_path, args)
    if opts.seed is not None:
        np.random.seed(opts.seed)
    t0 = time.perf_counter()
    try:
        path = dataset.get_training_images(dataset_path, args, batch=opts.batch)
    except FileNotFoundError as e:
        raise SystemExit('ae_train_data: %s' % e)
    dt = time.perf_counter() - t0
    print('%s: %d training images, %.1f images/s' % (path, len(dataset.train_x), len(dataset.train_x) / dt))
    return path


if __name__ == '__main__':
    main()
