"""Records, from the reference's own code, what the depth-refinement tests compare with: icp_golden.npz.

Run on a machine that has the reference checkout and scikit-learn:  python tests/golden/make_icp_golden.py /path/to/reference

Neither auto_pose/eval/icp_utils.py nor auto_pose/icp/icp.py imports under today's interpreter (print statements, imports of
the OpenGL renderer), so their text is executed in memory: from ``# Constants`` on, with the lines that are print
statements dropped, ``depth_crop.shape[k]/2`` written ``//2`` (the reference runs under Python 2, where that division
floors) and, for icp/icp.py, the unreachable imports replaced by names in the namespace.  What runs is the
reference's best_fit_transform, nearest_neighbor (scikit-learn's KD-tree), icp and icp_refinement, both variants.
misc.rgbd_to_point_cloud is executed the same way with its ``rgb != np.array([])`` test (an error in today's NumPy) given a
``None`` default; transform.py imports as it stands.  The renderer is a stub that hands out the synthetic depth of
tests/icp_cases.make_case (rendered by the float64 restatement of the rasteriser), so the file holds data only:

  per case k:   syn_k, crop_k (float32 depth), R_est_k, t_est_k, seed_k, sub_real_k, sub_syn_k, n_syn_k, n_real_k
  per case, variant (eval: eval/icp_utils.py, m3: icp/icp.py) and mode (plain, depth_only, no_depth):
                T, iterations (icp's i), mean_error (np.mean of the last distances), R_refined, t_refined
  few_*:        a crop with too few points: the refinement returns its inputs and draws nothing"""
import importlib.util
import os
import re
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))]
import icp_cases as ic  # noqa: E402


def _drop_prints(text):
    text = '\n'.join(line for line in text.split('\n') if not re.match(r'\s*print\s', line))
    assert text.count('.shape[0]/2') == 1 and text.count('.shape[1]/2') == 1
    return text.replace('.shape[0]/2', '.shape[0]//2').replace('.shape[1]/2', '.shape[1]//2')       # Python 2's int / int


def _load(ref):
    spec = importlib.util.spec_from_file_location('ref_transform', os.path.join(ref, 'auto_pose', 'ae', 'pysixd_stuff', 'transform.py'))
    transform = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(transform)
    msrc = open(os.path.join(ref, 'auto_pose', 'ae', 'pysixd_stuff', 'misc.py')).read()
    a = msrc.index('def rgbd_to_point_cloud')
    fn = msrc[a:msrc.index('\ndef ', a + 1)].replace('rgb=np.array([])', 'rgb=None').replace('if rgb != np.array([]):', 'if rgb is not None:')
    misc = types.ModuleType('misc')
    misc.np = np
    exec(compile(fn, 'misc.py', 'exec'), misc.__dict__)
    from sklearn.neighbors import NearestNeighbors
    import time

    src = open(os.path.join(ref, 'auto_pose', 'eval', 'icp_utils.py')).read()
    src = _drop_prints(src[src.index('# Constants'):])
    src = src[:src.index('class SynRenderer')] + src[src.index('def icp_refinement'):]
    ev = {'np': np, 'time': time, 'NearestNeighbors': NearestNeighbors, 'transform': transform, 'misc': misc, 'plt': None}
    exec(compile(src, 'icp_utils.py', 'exec'), ev)

    src = open(os.path.join(ref, 'auto_pose', 'icp', 'icp.py')).read()
    src = _drop_prints(src[src.index('# Constants'):])
    m3 = {'np': np, 'NearestNeighbors': NearestNeighbors, 'transform': transform, 'misc': misc, 'SynRenderer': lambda *a: None}
    exec(compile(src, 'icp.py', 'exec'), m3)
    return ev, m3


class _Stub(object):
    """SynRenderer.generate_synthetic_depth with the render replaced by a stored depth image"""

    def __init__(self, misc, syn):
        self.misc, self.syn = misc, syn

    def generate_synthetic_depth(self, K_test, R_est, t_est, test_shape, clas_idx=0):
        return self.misc.rgbd_to_point_cloud(K_test, self.syn)[0]


def main(ref):
    ev, m3 = _load(ref)
    K = ic.K_test()
    out = {'K': K, 'dims': np.array(ic.rc.DIMS)}
    for k in range(len(ic.CASES)):
        R_est, t_est, syn, crop = ic.make_case(k)
        seed = ic.CASES[k][4]
        out.update({'syn_%d' % k: syn, 'crop_%d' % k: crop, 'R_est_%d' % k: R_est, 't_est_%d' % k: t_est, 'seed_%d' % k: np.array(seed)})
        for variant in ic.VARIANTS:
            factor = ic.VARIANTS[variant][0]
            syn_pts, centroid, radius, real_all, keep, dist = ic.prepare(K, syn, crop, factor)
            rs = np.random.RandomState(seed)
            sub_real, sub_syn = ic.draw(rs, int(keep.sum()), len(syn_pts))
            out.update({'sub_real_%d_%s' % (k, variant): sub_real, 'sub_syn_%d_%s' % (k, variant): sub_syn,
                        'n_syn_%d_%s' % (k, variant): np.array(len(syn_pts)), 'n_real_%d_%s' % (k, variant): np.array(int(keep.sum()))})
            for mode in ic.MODES:
                flags = dict(depth_only=(mode == 'depth_only'), no_depth=(mode == 'no_depth'))
                stub = _Stub(ev['misc'], syn)
                # the pieces, for T / i / mean error ...
                A, B = syn_pts[sub_syn], real_all[keep][sub_real]
                if variant == 'eval':
                    T, distances, i = ev['icp'](A, B, tolerance=0.000001, **flags)
                else:
                    obj = m3['ICP'](None, None)
                    obj.syn_renderer = stub
                    T, distances, i = obj.icp(A, B, tolerance=0.000001, **flags)
                # ... and the whole function, with the global generator seeded as the tests seed theirs
                np.random.seed(seed)
                if variant == 'eval':
                    R_ref, t_ref = ev['icp_refinement'](crop, stub, R_est, t_est, K, ic.rc.DIMS, max_mean_dist_factor=factor, **flags)
                else:
                    R_ref, t_ref = obj.icp_refinement(crop, R_est, t_est, K, ic.rc.DIMS, **flags)
                key = '%d_%s_%s' % (k, variant, mode)
                out.update({'T_' + key: T, 'iterations_' + key: np.array(i), 'mean_error_' + key: np.array(np.mean(distances)),
                            'R_refined_' + key: np.array(R_ref), 't_refined_' + key: np.array(t_ref)})
                print('%s: n = %d, i = %d, mean error %.6f, |t_refined - t_est| = %.3f' % (key, len(A), i, np.mean(distances), np.linalg.norm(t_ref - t_est)))
    # too few points: most of the object masked out of the crop
    R_est, t_est, syn, crop = ic.make_case(0)
    few = crop.copy()
    few[:, 12:] = 0
    np.random.seed(7)
    before = np.random.get_state()[1].copy()
    R_ref, t_ref = ev['icp_refinement'](few, _Stub(ev['misc'], syn), R_est, t_est, K, ic.rc.DIMS)
    assert np.array_equal(before, np.random.get_state()[1]) and R_ref is R_est and t_ref is t_est
    out['few_crop'] = few
    np.savez_compressed(ic.GOLDEN, **out)
    print('wrote %s (%d bytes)' % (ic.GOLDEN, os.path.getsize(ic.GOLDEN)))


if __name__ == '__main__':
    main(sys.argv[1] if len(sys.argv) > 1 else os.environ.get('AAE_REFERENCE', ''))
