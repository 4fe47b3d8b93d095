"""``Renderer`` with the signature of the reference's two OpenGL renderers
(/root/reference/auto_pose/meshrenderer/meshrenderer_phong.py for ``model='reconst'``, meshrenderer.py for
``model='cad'``), backed by the HIP software rasteriser of libaae_hip.so (csrc/kernels/render_core.h states what is
computed and how exactly), plus the PLY reader the reference loads its models with.

No OpenGL, EGL or pyassimp: the mesh is uploaded once (``aae_mesh_create``) and every call renders a batch of views
in six launches; ``render_many`` / ``render_scenes`` draw several models into one frame (``aae_render_scenes``);
``render_training_views`` renders training pairs (``aae_render_training_views``: random light and shifted box next to default
light and true box, the geometry done once).  Parity with a real OpenGL driver is unpinned; the geometry is reproducible bit for bit against the
float64 restatement of the tests."""
from __future__ import annotations

import ctypes
import math
import struct

import numpy as np

from . import _lib

MODEL_KINDS = {'reconst': _lib.AAE_MODEL_RECONST, 'cad': _lib.AAE_MODEL_CAD}
DEFAULT_LIGHT = (400., 400., 400.)                                   # meshrenderer_phong.py:126
DEFAULT_PHONG = {'ambient': 0.4, 'diffuse': 0.8, 'specular': 0.3}    # meshrenderer_phong.py:101

_PLY_FORMATS = {'float': ('f', 4), 'double': ('d', 8), 'int': ('i', 4), 'uchar': ('B', 1)}      # inout.py:82-87


def load_ply(path):
    """gl_utils/inout.py:8-155: ``pts`` [n,3], and where the file has them ``normals`` [n,3], ``colors`` [n,3],
    ``texture_uv`` [n,2] and ``faces`` [m,3], all float64 as the reference returns them; ascii and
    binary_little_endian; only the scalar types of inout.py:82-87 and triangular faces."""
    with open(path, 'rb') as f:
        n_pts = n_faces = 0
        pt_props, face_props = [], []
        is_binary = False
        section = None
        while True:
            raw = f.readline()
            if not raw:
                raise ValueError('%s: no end_header' % path)
            line = raw.decode('ascii', 'replace').rstrip('\n').rstrip('\r')
            if line.startswith('element vertex'):
                n_pts = int(line.split()[-1])
                section = 'vertex'
            elif line.startswith('element face'):
                n_faces = int(line.split()[-1])
                section = 'face'
            elif line.startswith('element'):
                section = None
            elif line.startswith('property') and section == 'vertex':
                pt_props.append((line.split()[-1], line.split()[-2]))
            elif line.startswith('property list') and section == 'face':
                elems = line.split()
                if elems[-1] == 'vertex_indices':
                    face_props.append(('n_corners', elems[2]))
                    face_props += [('ind_%d' % i, elems[3]) for i in range(3)]
            elif line.startswith('format'):
                if 'binary_big_endian' in line:
                    raise ValueError('%s: binary_big_endian PLY is not supported' % path)
                is_binary = 'binary' in line
            elif line.startswith('end_header'):
                break
        names = [p[0] for p in pt_props]
        model = {'pts': np.zeros((n_pts, 3), np.float64)}
        if n_faces > 0:
            model['faces'] = np.zeros((n_faces, 3), np.float64)
        groups = [('pts', ('x', 'y', 'z'))]
        if {'nx', 'ny', 'nz'}.issubset(names):
            model['normals'] = np.zeros((n_pts, 3), np.float64)
            groups.append(('normals', ('nx', 'ny', 'nz')))
        if {'red', 'green', 'blue'}.issubset(names):
            model['colors'] = np.zeros((n_pts, 3), np.float64)
            groups.append(('colors', ('red', 'green', 'blue')))
        if {'texture_u', 'texture_v'}.issubset(names):
            model['texture_uv'] = np.zeros((n_pts, 2), np.float64)
            groups.append(('texture_uv', ('texture_u', 'texture_v')))
        for kind in [p[1] for p in pt_props + face_props]:
            if is_binary and kind not in _PLY_FORMATS:
                raise ValueError('%s: property type %r is not supported' % (path, kind))

        if is_binary:
            vfmt = '<' + ''.join(_PLY_FORMATS[p[1]][0] for p in pt_props)
            vsize = struct.calcsize(vfmt)
            rows = [struct.unpack(vfmt, f.read(vsize)) for _ in range(n_pts)]
        else:
            rows = [f.readline().decode('ascii').split() for _ in range(n_pts)]
        col = {name: k for k, name in enumerate(names)}
        for key, props in groups:
            for j, prop in enumerate(props):
                model[key][:, j] = [float(r[col[prop]]) for r in rows]

        if n_faces > 0:
            if is_binary:
                ffmt = '<' + ''.join(_PLY_FORMATS[p[1]][0] for p in face_props)
                fsize = struct.calcsize(ffmt)
                frows = [struct.unpack(ffmt, f.read(fsize)) for _ in range(n_faces)]
            else:
                frows = [f.readline().decode('ascii').split() for _ in range(n_faces)]
            fcol = {p[0]: k for k, p in enumerate(face_props)}
            for i, r in enumerate(frows):
                if int(r[fcol['n_corners']]) != 3:
                    raise ValueError('%s: only triangular faces are supported (face %d has %d corners)' % (path, i, int(r[fcol['n_corners']])))
                model['faces'][i] = [int(r[fcol['ind_0']]), int(r[fcol['ind_1']]), int(r[fcol['ind_2']])]
    return model


def calc_normals(vertices):
    """gl_utils/geometry.py:67-80 for a whole triangle soup at once: the face normal, repeated for its three vertices,
    zero for a zero-area face; float32 arithmetic as the reference's float32 vertices give it."""
    v = np.asarray(vertices, dtype=np.float32).reshape(-1, 3, 3)
    normal = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
    norm = np.sqrt((normal * normal).sum(axis=1, dtype=np.float32))
    safe = np.where(norm == 0, np.float32(1), norm)
    normal = np.where((norm == 0)[:, None], np.float32(0), normal / safe[:, None]).astype(np.float32)
    return np.repeat(normal, 3, axis=0)


def mesh_arrays(model, kind):
    """The vertex buffer of a loaded model: (verts f32 [V,3] unscaled, normals f32 [V,3], colors f32 [V,3] rgb in [0,1],
    faces int32 [F,3]).  reconst: load_meshes_sixd + meshrenderer_phong.py:41-55 (indexed, the file's normals, colours
    through uint32, 160 without).  cad: meshrenderer.py:37-42, a non-indexed triangle soup with recalculated per-face
    normals (the reference reads it through pyassimp; here the soup is built from the PLY's faces)."""
    if kind not in MODEL_KINDS:
        raise ValueError("model must be 'reconst' or 'cad', got %r" % (kind,))
    if 'faces' not in model:
        raise ValueError('the model has no faces')
    pts = np.asarray(model['pts']).astype(np.float32)
    faces = np.asarray(model['faces']).astype(np.uint32).astype(np.int64)
    if faces.size and (faces.min() < 0 or faces.max() >= len(pts)):
        raise ValueError('a face names vertex %d of %d' % (faces.max(), len(pts)))
    if kind == 'cad':
        verts = np.ascontiguousarray(pts[faces.reshape(-1)])
        normals = calc_normals(verts)
        colors = np.empty_like(verts)
        colors[:] = np.array([223., 214., 205.], dtype=np.float32) / np.float32(255)
        faces = np.arange(len(verts), dtype=np.int32).reshape(-1, 3)
        return verts, normals, colors, faces
    if 'normals' not in model:
        raise ValueError("model='reconst' needs per-vertex normals in the PLY (nx, ny, nz)")
    normals = np.asarray(model['normals']).astype(np.float32)
    if 'colors' in model:
        colors = (np.asarray(model['colors']).astype(np.uint32) / 255.0).astype(np.float32)
    else:
        colors = ((np.ones_like(pts) * 160.0) / 255.0).astype(np.float32)
    return np.ascontiguousarray(pts), np.ascontiguousarray(normals), np.ascontiguousarray(colors), np.ascontiguousarray(faces.astype(np.int32))


def draw_light(random_light, phong, kind):
    """(light position, ambient, diffuse, specular) of one render call; random_light draws them with the reference's
    np.random calls in the reference's order (meshrenderer_phong.py:117-129, meshrenderer.py:97-109)."""
    phong = DEFAULT_PHONG if phong is None else phong
    if not random_light:
        return DEFAULT_LIGHT, phong['ambient'], phong['diffuse'], phong['specular']
    light = 1000. * np.random.random(3)
    ambient = phong['ambient'] + (0.1 * (2 * np.random.rand() - 1) if kind == 'cad' else 0.0)
    diffuse = phong['diffuse'] + 0.1 * (2 * np.random.rand() - 1)
    specular = phong['specular'] + 0.1 * (2 * np.random.rand() - 1)
    return tuple(light), ambient, diffuse, specular


def random_rotation_matrix(rand=None):
    """pysixd_stuff/transform.py:1463-1503 (random_quaternion + quaternion_matrix): a uniform random rotation as a homogeneous
    4x4 matrix from three uniforms in [0, 1), drawn with np.random.rand(3) when not given; the reference's float64 operations in
    the reference's order, so the same seed gives the same bits."""
    if rand is None:
        rand = np.random.rand(3)
    else:
        assert len(rand) == 3
    r1 = np.sqrt(1.0 - rand[0])
    r2 = np.sqrt(rand[0])
    pi2 = math.pi * 2.0
    t1 = pi2 * rand[1]
    t2 = pi2 * rand[2]
    q = np.array([np.cos(t2) * r2, np.sin(t1) * r1, np.cos(t1) * r1, np.sin(t2) * r2], dtype=np.float64)
    n = np.dot(q, q)
    if n < np.finfo(float).eps * 4.0:
        return np.identity(4)
    q *= math.sqrt(2.0 / n)
    q = np.outer(q, q)
    return np.array([
        [1.0 - q[2, 2] - q[3, 3], q[1, 2] - q[3, 0], q[1, 3] + q[2, 0], 0.0],
        [q[1, 2] + q[3, 0], 1.0 - q[1, 1] - q[3, 3], q[2, 3] - q[1, 0], 0.0],
        [q[1, 3] - q[2, 0], q[2, 3] + q[1, 0], 1.0 - q[1, 1] - q[2, 2], 0.0],
        [0.0, 0.0, 0.0, 1.0]])


def draw_training_params(n, max_rel_offset, kind, phong=None):
    """The random numbers of n passes of the loop of dataset.py:238-285, drawn from np.random in the loop's order -- per image
    rand(3) for the rotation, the light of the train_x render (draw_light(True, ...)), uniform(-m, m) for x, then for y -- as
    (Rs float64 [n,3,3], lights float64 [n,6]: position, ambient, diffuse, specular, offsets float64 [n,2]).  The reference
    multiplies the offsets by the box's width and height afterwards, so every draw can precede the rendering."""
    Rs, lights, offsets = np.empty((n, 3, 3)), np.empty((n, 6)), np.empty((n, 2))
    for i in range(n):
        Rs[i] = random_rotation_matrix()[:3, :3]
        light, a, d, s = draw_light(True, phong, kind)
        lights[i] = light + (a, d, s)
        offsets[i, 0] = np.random.uniform(-max_rel_offset, max_rel_offset)
        offsets[i, 1] = np.random.uniform(-max_rel_offset, max_rel_offset)
    return Rs, lights, offsets


def render_params(W, H, K, t, near, far, pad_factor=1.0, light=DEFAULT_LIGHT, ambient=0.4, diffuse=0.8, specular=0.3):
    p = _lib.RenderParams()
    K = np.asarray(K, dtype=np.float64).reshape(3, 3)
    p.K[:] = K.reshape(-1).tolist()
    p.t[:] = np.asarray(t, dtype=np.float64).reshape(-1)[:3].tolist() if t is not None else [0.0, 0.0, 0.0]
    p.W, p.H = int(W), int(H)
    p.clip_near, p.clip_far, p.pad_factor = float(near), float(far), float(pad_factor)
    p.light[:] = [float(v) for v in light]
    p.ambient, p.diffuse, p.specular = float(ambient), float(diffuse), float(specular)
    return p


class Renderer(object):

    MAX_FBO_WIDTH = 2000
    MAX_FBO_HEIGHT = 2000

    def __init__(self, models_cad_files, samples=1, vertex_tmp_store_folder='.', vertex_scale=1.0, model='reconst', device=None):
        if int(samples) > 1:
            raise NotImplementedError('ANTIALIASING = %d: multisampling is not implemented (the MSAA resolve is driver-defined); use 1' % int(samples))
        if model not in MODEL_KINDS:
            raise ValueError("model must be 'reconst' or 'cad', got %r" % (model,))
        self.model = model
        self.vertex_scale = float(vertex_scale)
        self._samples = int(samples)
        # a model is a PLY path or an already loaded dict (load_ply's keys); no vertex cache file: loading is not the cost here
        self._arrays = [mesh_arrays(p if isinstance(p, dict) else load_ply(p), model) for p in models_cad_files]
        self._device = device
        self._meshes = None
        self._set = None
        self._ws = None
        self.lib = None
        self._torch = None

    # ---- device state, created at first use ---------------------------------------
    def _open(self):
        if self._meshes is not None:
            return
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError('the mesh rasteriser needs the GPU (libaae_hip.so): there is no CPU fallback')
        self.lib = _lib.load()
        self._torch = torch                                      # for the per-call helpers: an import statement each would cost a call microseconds
        if self._device is None:
            self._device = torch.device('cuda', torch.cuda.current_device())
        meshes = []
        with torch.cuda.device(self._device):
            for verts, normals, colors, faces in self._arrays:
                h = ctypes.c_void_p()
                rc = self.lib.aae_mesh_create(verts.ctypes.data, normals.ctypes.data, colors.ctypes.data, len(verts), faces.ctypes.data, len(faces),
                                              MODEL_KINDS[self.model], self.vertex_scale, ctypes.byref(h))
                _lib.check(self.lib, rc, 'aae_mesh_create')
                meshes.append(h)
            self._meshes = meshes
            # the set of all models (render_scenes / render_many): a device table of the mesh descriptors, written once
            handles = (ctypes.c_void_p * len(meshes))(*[h.value for h in meshes])
            mesh_set = ctypes.c_void_p()
            rc = self.lib.aae_mesh_set_create(handles, len(meshes), ctypes.byref(mesh_set))
            if rc != _lib.AAE_OK:
                self.close()
            _lib.check(self.lib, rc, 'aae_mesh_set_create')
            self._set = mesh_set

    def _workspace(self, need):
        import torch
        need = int(need)
        if self._ws is None or self._ws.numel() - (-self._ws.data_ptr()) % 256 < need:
            self._ws = None
            self._ws = torch.empty(need + 256, dtype=torch.uint8, device=self._device)
        return self._ws.data_ptr() + (-self._ws.data_ptr()) % 256, need

    def _upload(self, a, cols):
        import torch
        if isinstance(a, torch.Tensor):
            return a.to(device=self._device, dtype=torch.float64).reshape(-1, cols).contiguous()
        return torch.as_tensor(np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(-1, cols)), device=self._device)

    def _stream(self):
        return ctypes.c_void_p(self._torch.cuda.current_stream(self._device).cuda_stream)

    # ---- the parts every render call has ----------------------------------------------
    def _begin(self, W, H, *sizes):
        """the device state is open; the frame size and the call's further sizes as ints"""
        self._open()
        assert W <= Renderer.MAX_FBO_WIDTH and H <= Renderer.MAX_FBO_HEIGHT
        return [int(v) for v in (W, H) + sizes]

    def _out(self, shape, dtype):
        return self._torch.empty(shape, dtype=dtype, device=self._device)

    @staticmethod
    def _ptr(t):
        return None if t is None else ctypes.c_void_p(t.data_ptr())

    def _pick_workspace(self, workspace, need):
        """the caller's (pointer, bytes), or the renderer's own buffer of need bytes: the two workspace arguments of a call"""
        ptr, nbytes = workspace if workspace is not None else self._workspace(need)
        return ctypes.c_void_p(ptr), nbytes

    def _call(self, name, args, timed=False):
        """lib.<name>(*args) on the renderer's device and stream, or its _timed twin: the milliseconds of the six launches, else None"""
        ms = (ctypes.c_float * 6)() if timed else None
        name, args = (name + '_timed', args + (self._stream(), ms)) if timed else (name, args + (self._stream(),))
        with self._torch.cuda.device(self._device):
            _lib.check(self.lib, getattr(self.lib, name)(*args), name)
        return list(ms) if timed else None

    # ---- rendering ------------------------------------------------------------------
    def render_batch(self, obj_id, W, H, K, Rs, ts, near, far, random_light=False, phong=None, workspace=None, return_tri=False, light=None):
        """n views in one call: Rs [n,3,3], ts [n,3] or one [3] for all -> (bgr uint8 [n,H,W,3], depth float32 [n,H,W],
        obj_bbs int32 [n,4], visible int32 [n]) as device tensors, with return_tri=True also the index of the visible face
        per pixel (int32 [n,H,W], -1 = background).  One light for the batch, as one render call has: draw_light's, or the
        explicit light = (position, ambient, diffuse, specular)."""
        import torch
        W, H = self._begin(W, H)
        mesh = self._meshes[obj_id]
        Rd = self._upload(Rs, 9)
        n = Rd.shape[0]
        t_arr = np.asarray(ts.cpu() if isinstance(ts, torch.Tensor) else ts, dtype=np.float64)
        td = None if t_arr.size == 3 else self._upload(t_arr, 3)
        if td is not None and td.shape[0] != n:
            raise ValueError('%d rotations, %d translations' % (n, td.shape[0]))
        light, a, d, s = draw_light(random_light, phong, self.model) if light is None else light
        p = render_params(W, H, K, t_arr if td is None else None, near, far, 1.0, light, a, d, s)
        bgr, depth = self._out((n, H, W, 3), torch.uint8), self._out((n, H, W), torch.float32)
        bbs, vis = self._out((n, 4), torch.int32), self._out((n,), torch.int32)
        tri = self._out((n, H, W), torch.int32) if return_tri else None
        ptr = self._ptr
        self._call('aae_render_frames', (mesh, ptr(Rd), ptr(td), n, ctypes.byref(p), ptr(bgr), ptr(depth), ptr(tri), ptr(bbs), ptr(vis))
                   + self._pick_workspace(workspace, self.lib.aae_render_workspace_bytes(mesh, n, W, H)))
        if return_tri:
            return bgr, depth, bbs, vis, tri
        return bgr, depth, bbs, vis

    def render_embedding_views(self, obj_id, W, H, K, Rs, t, near, far, pad_factor, crop, random_light=False, phong=None, workspace=None,
                               timed=False):
        """Renderer.render + calc_2d_bbox + extract_square_patch(INTER_NEAREST) of dataset.py:326-347 for n rotations at one
        translation: (crops uint8 [n,crop,crop,3] BGR, obj_bbs int32 [n,4], visible int32 [n]) as device tensors; with
        timed=True also the milliseconds of the six launches."""
        import torch
        W, H, crop = self._begin(W, H, crop)
        mesh = self._meshes[obj_id]
        Rd = self._upload(Rs, 9)
        n = Rd.shape[0]
        light, a, d, s = draw_light(random_light, phong, self.model)
        p = render_params(W, H, K, t, near, far, pad_factor, light, a, d, s)
        crops, bbs, vis = self._out((n, crop, crop, 3), torch.uint8), self._out((n, 4), torch.int32), self._out((n,), torch.int32)
        ptr = self._ptr
        ms = self._call('aae_render_embedding_views', (mesh, ptr(Rd), n, ctypes.byref(p), crop, ptr(crops), ptr(bbs), ptr(vis))
                        + self._pick_workspace(workspace, self.lib.aae_render_workspace_bytes(mesh, n, W, H)), timed)
        return (crops, bbs, vis, ms) if timed else (crops, bbs, vis)

    def render_training_views(self, obj_id, W, H, K, Rs, t, near, far, pad_factor, crop, lights, offsets, phong=None, workspace=None, timed=False):
        """n passes of the loop of dataset.py:238-303 at one translation, the geometry of a pair rendered once: lights [n,6]
        (position, ambient, diffuse, specular of the train_x render), offsets [n,2] (the shift of train_x's box in units of its
        width and height) -> (train_x uint8 [n,crop,crop,3] BGR, mask_x bool [n,crop,crop], train_y uint8 [n,crop,crop,3],
        obj_bbs int32 [n,4], visible int32 [n]) as device tensors; with timed=True also the milliseconds of the six launches.
        train_y has the default light with phong's constants.  A view that covers no pixel has flag 0, zero crops and a mask
        of all ones."""
        import torch
        W, H, crop = self._begin(W, H, crop)
        mesh = self._meshes[obj_id]
        Rd = self._upload(Rs, 9)
        n = Rd.shape[0]
        Ld = self._upload(lights, 6).to(torch.float32)
        Od = self._upload(offsets, 2)
        if Ld.shape[0] != n or Od.shape[0] != n:
            raise ValueError('%d rotations, %d lights, %d offsets' % (n, Ld.shape[0], Od.shape[0]))
        light, a, d, s = draw_light(False, phong, self.model)
        p = render_params(W, H, K, t, near, far, pad_factor, light, a, d, s)
        train_x, train_y = self._out((n, crop, crop, 3), torch.uint8), self._out((n, crop, crop, 3), torch.uint8)
        mask_x, bbs, vis = self._out((n, crop, crop), torch.uint8), self._out((n, 4), torch.int32), self._out((n,), torch.int32)
        ptr = self._ptr
        ms = self._call('aae_render_training_views', (mesh, ptr(Rd), ptr(Ld), ptr(Od), n, ctypes.byref(p), crop, ptr(train_x), ptr(mask_x), ptr(train_y),
                                                      ptr(bbs), ptr(vis))
                        + self._pick_workspace(workspace, self.lib.aae_render_training_workspace_bytes(mesh, n, W, H)), timed)
        out = (train_x, mask_x.view(torch.bool), train_y, bbs, vis)
        return out + (ms,) if timed else out

    def render(self, obj_id, W, H, K, R, t, near, far, random_light=False, phong=None):
        """meshrenderer_phong.py:101-168 / meshrenderer.py:84-137: (bgr uint8 [H,W,3], depth float32 [H,W]) on the host."""
        bgr, depth, _, _ = self.render_batch(obj_id, W, H, K, np.asarray(R, dtype=np.float64).reshape(1, 3, 3),
                                             np.asarray(t, dtype=np.float64).reshape(3), near, far, random_light, phong)
        return bgr[0].cpu().numpy(), depth[0].cpu().numpy()

    def render_scenes(self, obj_ids, scene_ids, n_scenes, W, H, K, Rs, ts, near, far, random_light=False, phong=None, workspace=None,
                      return_ids=False, timed=False):
        """Several models into one frame, several frames in one call: draw d is model obj_ids[d] at (Rs[d], ts[d]) in scene
        scene_ids[d] -> (bgr uint8 [S,H,W,3], depth float32 [S,H,W], obj_bbs int32 [D,4], visible int32 [D]) as device tensors,
        with return_ids=True also the winning draw and its face per pixel (int32 [S,H,W], -1 = background); with timed=True also
        the milliseconds of the six launches.  The draws of a scene share one depth buffer: the nearest fp32 depth wins, at
        equal depth the earlier draw.  obj_bbs[d] is the box of draw d rendered alone (render_many's), visible[d] = 0 when it
        covers no pixel.  One light for the call.  At most 256 draws a call: split by scene."""
        import torch
        W, H, S = self._begin(W, H, n_scenes)
        obj = np.ascontiguousarray(np.asarray(obj_ids, dtype=np.int32).reshape(-1))
        scn = np.ascontiguousarray(np.asarray(scene_ids, dtype=np.int32).reshape(-1))
        D = len(obj)
        if D > _lib.AAE_SCENE_MAX_DRAWS:
            raise ValueError('aae_render_scenes: %d draws, at most %d per call (split by scene)' % (D, _lib.AAE_SCENE_MAX_DRAWS))
        if D < 1 or len(scn) != D:
            raise ValueError('aae_render_scenes: %d obj_ids, %d scene_ids' % (D, len(scn)))
        if S < 1:
            raise ValueError('aae_render_scenes: %d scenes' % S)
        Rd, td = self._upload(Rs, 9), self._upload(ts, 3)
        if Rd.shape[0] != D or td.shape[0] != D:
            raise ValueError('aae_render_scenes: %d draws, %d rotations, %d translations' % (D, Rd.shape[0], td.shape[0]))
        light, a, d, s = draw_light(random_light, phong, self.model)
        p = render_params(W, H, K, None, near, far, 1.0, light, a, d, s)
        bgr, depth = self._out((S, H, W, 3), torch.uint8), self._out((S, H, W), torch.float32)
        bbs, vis = self._out((D, 4), torch.int32), self._out((D,), torch.int32)
        draw, tri = (self._out((S, H, W), torch.int32), self._out((S, H, W), torch.int32)) if return_ids else (None, None)
        ptr = self._ptr
        ms = self._call('aae_render_scenes', (self._set, obj.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), scn.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                              ptr(Rd), ptr(td), D, S, ctypes.byref(p), ptr(bgr), ptr(depth), ptr(draw), ptr(tri), ptr(bbs), ptr(vis))
                        + self._pick_workspace(workspace, self.lib.aae_render_scenes_workspace_bytes(self._set, D, S, W, H)), timed)
        out = (bgr, depth, bbs, vis) + ((draw, tri) if return_ids else ())
        return out + (ms,) if timed else out

    def render_many(self, obj_ids, W, H, K, Rs, ts, near, far, random_light=None, phong=None):
        """meshrenderer.py:140-194 / meshrenderer_phong.py:170-224: the models obj_ids at the poses (Rs[i], ts[i]) in one frame with
        one depth buffer -> (bgr uint8 [H,W,3], depth float32 [H,W], bbs: one [x, y, w, h] per object, of the object rendered
        alone) on the host.  random_light=None is the reference's default for the kind (True for 'reconst', False for 'cad');
        the light is drawn once per call.  A draw that covers no pixel raises ValueError (the reference: from calc_2d_bbox)."""
        if random_light is None:
            random_light = self.model == 'reconst'
        n = len(obj_ids)
        bgr, depth, bbs, vis = self.render_scenes(obj_ids, [0] * n, 1, W, H, K, np.asarray([np.asarray(R, dtype=np.float64).reshape(3, 3) for R in Rs]),
                                                  np.asarray([np.asarray(t, dtype=np.float64).reshape(3) for t in ts]), near, far, random_light, phong)
        vis = vis.cpu().numpy()
        for i in range(n):
            if not vis[i]:
                raise ValueError('render_many: draw %d (obj_id %d) covers no pixel of the %dx%d frame' % (i, int(obj_ids[i]), int(W), int(H)))
        return bgr[0].cpu().numpy(), depth[0].cpu().numpy(), [[int(v) for v in bb] for bb in bbs.cpu().numpy()]

    def overlay_blend(self, image, render, channel=1, out=None):
        """aae_overlay_blend on device uint8 tensors of one shape [..., 3]: where render > 0, two thirds of the render's `channel`
        over one third of the image (visualization/render_pose.py:44-46); out may be image itself."""
        import torch
        self._open()
        if image.shape != render.shape or image.dtype != torch.uint8 or render.dtype != torch.uint8 or image.shape[-1] != 3:
            raise ValueError('aae_overlay_blend: image %s %s, render %s %s' % (tuple(image.shape), image.dtype, tuple(render.shape), render.dtype))
        image, render = image.contiguous(), render.contiguous()
        out = torch.empty_like(image) if out is None else out
        if not out.is_contiguous() or out.shape != image.shape or out.dtype != torch.uint8:
            raise ValueError('aae_overlay_blend: out must be a contiguous uint8 tensor of the image\'s shape')
        with torch.cuda.device(self._device):
            rc = self.lib.aae_overlay_blend(ctypes.c_void_p(image.data_ptr()), ctypes.c_void_p(render.data_ptr()), image.numel() // 3, int(channel),
                                            ctypes.c_void_p(out.data_ptr()), self._stream())
        _lib.check(self.lib, rc, 'aae_overlay_blend')
        return out

    def close(self):
        if self._set is not None:
            self.lib.aae_mesh_set_destroy(self._set)
        self._set = None
        if self._meshes is not None:
            for h in self._meshes:
                self.lib.aae_mesh_destroy(h)
        self._meshes = None
        self._ws = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
