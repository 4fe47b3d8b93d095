"""Records, from the reference's own code, what the rasteriser tests compare the PLY reader and the camera with:

  render_ascii.ply / render_binary.ply   a small torus (24 vertices, 48 faces) written by tests/render_reference.write_ply
  render_golden.npz                      gl_utils/inout.load_ply on both files; Camera.realCamera's T_view_world /
                                         T_proj_view for three poses

Run on a machine that has the reference checkout:  python tests/golden/make_render_golden.py /path/to/reference
inout.py (it imports only numpy, struct and itertools) is executed as it stands, with two shims for today's interpreter:
``np.float`` (removed from NumPy) is ``float``, and ``open`` hands it a file whose ``readline`` returns text and whose
``read`` returns bytes (it opens binary PLYs in text mode, which Python 3 cannot struct.unpack).  camera.py is imported with
``OpenGL.GL`` stubbed, the way the other generators stub TensorFlow."""
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import render_reference as rr  # noqa: E402


class _TextAndBytes(object):
    def __init__(self, path):
        self.f = open(path, 'rb')

    def readline(self):
        return self.f.readline().decode('ascii')

    def read(self, n):
        return self.f.read(n)

    def close(self):
        self.f.close()


def _load_inout(ref):
    if not hasattr(np, 'float'):
        np.float = float
    src = open(os.path.join(ref, 'auto_pose', 'meshrenderer', 'gl_utils', 'inout.py')).read()
    ns = {'open': lambda path, mode='r': _TextAndBytes(path), '__name__': 'inout'}
    exec(compile(src, 'inout.py', 'exec'), ns)
    return ns['load_ply']


def _load_camera(ref):
    gl = types.ModuleType('OpenGL.GL')
    pkg = types.ModuleType('OpenGL')
    pkg.GL = gl
    sys.modules['OpenGL'], sys.modules['OpenGL.GL'] = pkg, gl
    spec = importlib.util.spec_from_file_location('ref_camera', os.path.join(ref, 'auto_pose', 'meshrenderer', 'gl_utils', 'camera.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.Camera


def main(ref):
    model = rr.torus_model(R=60.0, r=25.0, nu=6, nv=4)
    out = {}
    load_ply = _load_inout(ref)
    for fmt in ('ascii', 'binary'):
        path = os.path.join(HERE, 'render_%s.ply' % fmt)
        rr.write_ply(path, model, binary=(fmt == 'binary'))
        got = load_ply(path)
        assert sorted(got) == ['colors', 'faces', 'normals', 'pts']
        for key, val in got.items():
            out['%s_%s' % (fmt, key)] = val

    Camera = _load_camera(ref)
    poses = [((720, 540), rr.TEMPLATE_K, rr.random_rotations(1, 1)[0], np.array([0., 0., 700.]), (10., 10000.)),
             ((160, 120), rr.scaled_K(160, 120), rr.random_rotations(1, 2)[0], np.array([200., -150., 700.]), (10., 10000.)),
             ((640, 480), np.array([[572.4, 0.3, 325.3], [0, 573.6, 242.0], [0, 0, 1]]), rr.random_rotations(1, 3)[0], np.array([-30., 40., 450.]), (5., 2000.))]
    for key in ('cam_dims', 'cam_K', 'cam_R', 'cam_t', 'cam_near_far', 'cam_T_view_world', 'cam_T_proj_view'):
        out[key] = []
    for (W, H), K, R, t, (near, far) in poses:
        cam = Camera()
        cam.realCamera(W, H, K, R, t, near, far)
        out['cam_dims'].append([W, H]); out['cam_K'].append(K); out['cam_R'].append(R); out['cam_t'].append(t)
        out['cam_near_far'].append([near, far])
        out['cam_T_view_world'].append(cam.T_view_world.copy())
        out['cam_T_proj_view'].append(cam.T_proj_view.copy())
    np.savez(os.path.join(HERE, 'render_golden.npz'), **{k: np.asarray(v) for k, v in out.items()})
    print('wrote render_ascii.ply, render_binary.ply, render_golden.npz')


if __name__ == '__main__':
    main(sys.argv[1] if len(sys.argv) > 1 else os.environ.get('AAE_REFERENCE', ''))
