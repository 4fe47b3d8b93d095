"""The timed twins of the mesh rasteriser on the MI355X (aae_render_embedding_views_timed, aae_render_scenes_timed: six
milliseconds, the bytes of the untimed call) and the order in which the single-mesh calls refuse bad arguments: view count,
camera, workspace size, workspace alignment, each refusal naming its entry point, all of them before any launch."""
import ctypes
import math

import numpy as np
import pytest

import render_cases as rc
import render_reference as rr
import scene_cases as sc

pytestmark = pytest.mark.gpu

W, H = rc.DIMS
K = rr.scaled_K(W, H)
CROP = 32


@pytest.fixture(scope='module')
def renderers(tmp_path_factory):
    from augmentedautoencoder_amd.meshrenderer import Renderer
    d = tmp_path_factory.mktemp('timed_ply')
    paths = []
    for k, name in enumerate(sc.SET):
        paths.append(str(d / (name + '.ply')))
        rr.write_ply(paths[-1], rc.model_dict(name), binary=(k % 2 == 1))
    out = {'torus': Renderer([paths[sc.SET.index('torus')]], model='reconst'), 'set': Renderer(paths, model='reconst')}
    yield out
    for r in out.values():
        r.close()


def _check_ms(ms):
    assert len(ms) == 6 and all(isinstance(v, float) and math.isfinite(v) and v >= 0 for v in ms), ms


def test_embedding_views_timed_gives_the_untimed_bytes(renderers):
    r = renderers['torus']
    call = lambda **kw: r.render_embedding_views(0, W, H, K, rc.rotations('torus'), rc.T0, rc.NEAR, rc.FAR, rc.PAD, CROP, **kw)
    plain, timed = call(), call(timed=True)
    assert len(plain) == 3 and len(timed) == 4
    _check_ms(timed[3])
    assert plain[0].shape == (rc.N_ROT, CROP, CROP, 3) and plain[0].cpu().numpy().any() and plain[2].cpu().numpy().all()
    for a, b in zip(plain, timed[:3]):
        assert a.dtype == b.dtype and a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


def test_scenes_timed_gives_the_untimed_bytes(renderers):
    r = renderers['set']
    Rs, ts = sc.poses(sc.SCENE_A)
    call = lambda **kw: r.render_scenes(sc.obj_ids(sc.SCENE_A), [0] * len(sc.SCENE_A), 1, W, H, K, Rs, ts, rc.NEAR, rc.FAR, return_ids=True, **kw)
    plain, timed = call(), call(timed=True)
    assert len(plain) == 6 and len(timed) == 7
    _check_ms(timed[6])
    assert plain[0].cpu().numpy().any() and plain[3].cpu().numpy().tolist() == sc.FLAGS_A
    for a, b in zip(plain, timed[:6]):
        assert a.dtype == b.dtype and a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


# ---- refusal order of the single-mesh calls -------------------------------------------
# every pointer is a live device buffer of the size a valid call needs (the workspace with 256 spare bytes), so a check that
# failed to fire could not send a launch anywhere else; the calls below must all return before any launch

BAD = {                                       # item -> (return code, what aae_last_error() names), in the order the checks fire
    'n': (-2, b'0 views outside'),
    'K': (-1, b'K[1,0]'),
    'near_far': (-1, b'need 0 < near < far'),
    'short': (-4, b' needed'),
    'misaligned': (-4, b'256-byte aligned'),
}
ORDER = list(BAD)
CALLS = ('aae_render_embedding_views', 'aae_render_frames', 'aae_render_training_views')


def _raw_call(r, name, bad):
    import torch
    from augmentedautoencoder_amd.meshrenderer import render_params
    dev = lambda *shape, dtype=torch.uint8: torch.zeros(shape, dtype=dtype, device='cuda')
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    n = rc.N_ROT
    mesh = r._meshes[0]
    Kb = np.array(K, dtype=np.float64)
    if 'K' in bad:
        Kb[1, 0] = 0.5
    near, far = (rc.FAR, rc.NEAR) if 'near_far' in bad else (rc.NEAR, rc.FAR)
    p = render_params(W, H, Kb, rc.T0, near, far, rc.PAD)
    need = int((r.lib.aae_render_training_workspace_bytes if name == 'aae_render_training_views' else r.lib.aae_render_workspace_bytes)(mesh, n, W, H))
    ws = dev(need + 512)
    ws_ptr = ws.data_ptr() + (-ws.data_ptr()) % 256 + (8 if 'misaligned' in bad else 0)
    ws_bytes = need - 1 if 'short' in bad else need
    Rd = torch.as_tensor(rc.rotations('torus').reshape(-1, 9), device='cuda')
    bbs, vis = dev(n, 4, dtype=torch.int32), dev(n, dtype=torch.int32)
    n_arg = 0 if 'n' in bad else n
    tail = (ptr(bbs), ptr(vis), ctypes.c_void_p(ws_ptr), ws_bytes, None)
    if name == 'aae_render_embedding_views':
        keep = [dev(n, CROP, CROP, 3)]
        args = (mesh, ptr(Rd), n_arg, ctypes.byref(p), CROP, ptr(keep[0])) + tail
    elif name == 'aae_render_frames':
        keep = [dev(n, H, W, 3), dev(n, H, W, dtype=torch.float32)]
        args = (mesh, ptr(Rd), None, n_arg, ctypes.byref(p), ptr(keep[0]), ptr(keep[1]), None) + tail
    else:
        keep = [dev(n, 6, dtype=torch.float32), dev(n, 2, dtype=torch.float64), dev(n, CROP, CROP, 3), dev(n, CROP, CROP), dev(n, CROP, CROP, 3)]
        args = (mesh, ptr(Rd), ptr(keep[0]), ptr(keep[1]), n_arg, ctypes.byref(p), CROP, ptr(keep[2]), ptr(keep[3]), ptr(keep[4])) + tail
    code = getattr(r.lib, name)(*args)
    torch.cuda.synchronize()
    return code, r.lib.aae_last_error()


@pytest.mark.parametrize('name', CALLS)
def test_single_mesh_refusals_name_the_call_in_order(renderers, name):
    r = renderers['torus']
    r._open()
    assert _raw_call(r, name, ())[0] == 0                                      # the arguments are good before one is spoiled
    for item in ORDER:                                                         # one at a time
        code, msg = _raw_call(r, name, (item,))
        assert code == BAD[item][0] and msg.startswith(name.encode() + b': ') and BAD[item][1] in msg, (item, code, msg)
    for first, second in zip(ORDER, ORDER[1:]):                                # two at once: the earlier check answers
        code, msg = _raw_call(r, name, (first, second))
        assert code == BAD[first][0] and msg.startswith(name.encode() + b': ') and BAD[first][1] in msg, (first, second, code, msg)
        assert BAD[second][1] not in msg
    code, msg = _raw_call(r, name, ORDER)                                      # all at once: the view count
    assert code == -2 and BAD['n'][1] in msg
