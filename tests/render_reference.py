"""NumPy float64 restatement of what the reference's renderer, calc_2d_bbox and extract_square_patch yield for one view --
the reference of the rasteriser tests (CPU: tests/native/render_host.cpp drives render_core.h; GPU: the kernels).

Written from the reference's Python and shader text (paths relative to auto_pose/meshrenderer/), not from the kernels:
  camera        gl_utils/camera.py:86-98 (realCamera), :139-166 (setIntrinsic), :195-205 (__glOrtho__)
  reconst       shader/depth_shader_phong.vs:21-32, shader/depth_shader_phong.frag:18-38, meshrenderer_phong.py:101-168
  cad           shader/cad_shader.vs:22-34, shader/cad_shader.frag:16-42, meshrenderer.py:84-137
  bbox / crop   pysixd/view_sampler.py:10-15, auto_pose/ae/dataset.py:354-373

What a GL driver leaves open is fixed by the rule the project documents: pixel coordinates in float64 snapped
to 1/256 pixel, int64 edge functions with the top-left fill rule, both windings, z interpolated perspective-correctly in
float64 and rounded once to fp32, GL_LESS with the first-drawn triangle winning a tie, a triangle with a vertex in front
of the near plane dropped whole.  Colour is float64 throughout here (the kernels shade in fp32).

Also the meshes of the tests and a PLY writer."""
import struct

import numpy as np

SUB = 256
HALF = 128
MAX_PIXEL = 4194304.0


# ---- the view and projection matrices of the reference, for the shader's varyings -------------------------------
def view_matrix(R, t):
    """camera.py:88-93: T_view_world of realCamera (float64 here, the reference stores float32)."""
    T_world_view = np.eye(4)
    T_world_view[:3, :3] = R.T
    T_world_view[:3, 3] = -R.T.dot(np.asarray(t, dtype=np.float64).reshape(3))
    z_flip = np.eye(4)
    z_flip[2, 2] = -1
    T_world_view = T_world_view.dot(z_flip)
    return np.linalg.inv(T_world_view)


def projection_matrix(K, W, H, near, far):
    """camera.py:139-166 (setIntrinsic, originIsInTopLeft=True) with :195-205 (__glOrtho__(0, W, H, 0, near, far)), float64."""
    persp = np.array([[K[0, 0], K[0, 1], -K[0, 2], 0],
                      [0, K[1, 1], -K[1, 2], 0],
                      [0, 0, near + far, near * far],
                      [0, 0, -1, 0]], dtype=np.float64)
    left, right, bottom, top = 0.0, float(W), float(H), 0.0
    ortho = np.array([[2. / (right - left), 0, 0, -(right + left) / (right - left)],
                      [0, 2. / (top - bottom), 0, -(top + bottom) / (top - bottom)],
                      [0, 0, -2. / (far - near), -(far + near) / (far - near)],
                      [0, 0, 0, 1]], dtype=np.float64)
    return ortho.dot(persp)


def pixel_coordinates(K, R, t, X):
    """The image pixel (u, v) and camera depth z_c of points X [n,3] (float64), in the one order of operations the
    project fixes: X_c = R X + t, u = (K00 x_c + K01 y_c) / z_c + K02, v = K11 y_c / z_c + K12."""
    X = np.asarray(X, dtype=np.float64)
    x, y, z = X[:, 0], X[:, 1], X[:, 2]
    xc = ((R[0, 0] * x + R[0, 1] * y) + R[0, 2] * z) + t[0]
    yc = ((R[1, 0] * x + R[1, 1] * y) + R[1, 2] * z) + t[1]
    zc = ((R[2, 0] * x + R[2, 1] * y) + R[2, 2] * z) + t[2]
    with np.errstate(all='ignore'):
        u = (K[0, 0] * xc + K[0, 1] * yc) / zc + K[0, 2]
        v = (K[1, 1] * yc) / zc + K[1, 2]
    return u, v, zc


def _topleft(A, B):
    return A > 0 or (A == 0 and B > 0)


def render(mesh, model, K, R, t, W, H, near, far, light=(400., 400., 400.), ambient=0.4, diffuse=0.8, specular=0.3, shade=True):
    """One view.  mesh: dict(verts f32 [V,3] already scaled, normals f32 [V,3], colors f32 [V,3] in [0,1], faces [F,3]).
    Returns dict(bgr uint8 [H,W,3], depth float32 [H,W], tri int64 [H,W] (-1: background), bb [x,y,w,h] or None);
    shade=False leaves bgr black (geometry and box only)."""
    K = np.asarray(K, dtype=np.float64).reshape(3, 3)
    R = np.asarray(R, dtype=np.float64).reshape(3, 3)
    t = np.asarray(t, dtype=np.float64).reshape(3)
    verts = np.asarray(mesh['verts'], dtype=np.float32).astype(np.float64)
    faces = np.asarray(mesh['faces']).astype(np.int64)
    u, v, zc = pixel_coordinates(K, R, t, verts)
    with np.errstate(all='ignore'):
        usable = (zc >= near) & (np.abs(u) <= MAX_PIXEL) & (np.abs(v) <= MAX_PIXEL)
        xs = np.where(usable, np.floor(u * SUB + 0.5), 0).astype(np.int64)
        ys = np.where(usable, np.floor(v * SUB + 0.5), 0).astype(np.int64)

    key = np.full((H, W), np.iinfo(np.uint64).max, dtype=np.uint64)
    setups = {}
    for f, (i0, i1, i2) in enumerate(faces):
        if not (usable[i0] and usable[i1] and usable[i2]):
            continue
        idx = (i0, i1, i2)
        px = [int(xs[i]) for i in idx]
        py = [int(ys[i]) for i in idx]
        area2 = (px[2] - px[1]) * (py[0] - py[1]) - (py[2] - py[1]) * (px[0] - px[1])
        if area2 == 0:
            continue
        s = 1 if area2 > 0 else -1
        # pixel j is sampled at 256 j + 128: the columns / rows whose sample can lie inside the vertex box
        x0 = max(-((-(min(px) - HALF)) // SUB), 0)
        x1 = min((max(px) - HALF) // SUB, W - 1)
        y0 = max(-((-(min(py) - HALF)) // SUB), 0)
        y1 = min((max(py) - HALF) // SUB, H - 1)
        if x0 > x1 or y0 > y1:
            continue
        sx = (np.arange(x0, x1 + 1, dtype=np.int64) * SUB + HALF)[None, :]
        sy = (np.arange(y0, y1 + 1, dtype=np.int64) * SUB + HALF)[:, None]
        e = []
        inside = np.ones((y1 - y0 + 1, x1 - x0 + 1), dtype=bool)
        edges = []
        for i in range(3):
            a, b = (i + 1) % 3, (i + 2) % 3
            A = -(py[b] - py[a]) * s
            B = (px[b] - px[a]) * s
            ei = A * (sx - px[a]) + B * (sy - py[a])
            inside &= (ei > 0) | ((ei == 0) & _topleft(A, B))
            e.append(ei)
            edges.append((A, B, px[a], py[a]))
        if not inside.any():
            continue
        z = [float(zc[i]) for i in idx]
        with np.errstate(all='ignore'):
            den = (e[0].astype(np.float64) / z[0] + e[1].astype(np.float64) / z[1]) + e[2].astype(np.float64) / z[2]
            zf = (e[0] + e[1] + e[2]).astype(np.float64) / den
            keep = inside & (zf <= far)
            k = (zf.astype(np.float32).view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.uint64(f)
        sub = key[y0:y1 + 1, x0:x1 + 1]
        win = keep & (k < sub)
        sub[win] = k[win]
        setups[f] = (edges, z, idx)

    covered = key != np.iinfo(np.uint64).max
    tri = np.where(covered, (key & np.uint64(0xFFFFFFFF)).astype(np.int64), -1)
    depth = np.where(covered, (key >> np.uint64(32)).astype(np.uint32).view(np.float32), np.float32(0)).astype(np.float32)

    # ---- shading, float64 ----
    view = view_matrix(R, t)
    u_nm = np.linalg.inv(view).T                                           # .vs: transpose(inverse(view))
    Vh = np.concatenate([verts, np.ones((len(verts), 1))], axis=1)
    P = Vh.dot(view.T)[:, :3]                                              # P = view * vec4(position, 1)
    v_view = -P
    L = np.asarray(light, dtype=np.float64)[None, :] - P
    if model == 'reconst':
        L = L / np.linalg.norm(L, axis=1, keepdims=True)                   # depth_shader_phong.vs:30
    n4 = np.concatenate([np.asarray(mesh['normals'], dtype=np.float32).astype(np.float64), np.ones((len(verts), 1))], axis=1).dot(u_nm.T)
    with np.errstate(all='ignore'):
        v_normal = (n4 / np.linalg.norm(n4, axis=1, keepdims=True))[:, :3]  # normalize(vec4).xyz
    colors = np.asarray(mesh['colors'], dtype=np.float32).astype(np.float64)
    material = np.array([223. / 255, 214. / 255, 205. / 255])

    bgr = np.zeros((H, W, 3), dtype=np.uint8)
    for f in (np.unique(tri[covered]) if shade else []):
        edges, z, idx = setups[int(f)]
        yy, xx = np.nonzero(tri == f)
        sx = xx.astype(np.int64) * SUB + HALF
        sy = yy.astype(np.int64) * SUB + HALF
        w = []
        for i in range(3):
            A, B, ox, oy = edges[i]
            w.append((A * (sx - ox) + B * (sy - oy)).astype(np.float64) / z[i])
        den = (w[0] + w[1]) + w[2]
        b = [wi / den for wi in w]
        interp = lambda a: b[0][:, None] * a[idx[0]][None, :] + b[1][:, None] * a[idx[1]][None, :] + b[2][:, None] * a[idx[2]][None, :]
        with np.errstate(all='ignore'):
            N = interp(v_normal)
            N = N / np.linalg.norm(N, axis=1, keepdims=True)
            Ld = interp(L)
            Ld = Ld / np.linalg.norm(Ld, axis=1, keepdims=True)
            Vd = interp(v_view)
            Vd = Vd / np.linalg.norm(Vd, axis=1, keepdims=True)
            color = interp(colors) if model == 'reconst' else np.broadcast_to(material, (len(xx), 3))
            ndl = (N * Ld).sum(axis=1)
            diff = np.fmax(ndl, 0.0)[:, None] * color
            Rv = 2.0 * ndl[:, None] * N - Ld                                # reflect(-LightDir, Normal)
            spec = np.fmax((Rv * Vd).sum(axis=1), 0.0)[:, None] * color
            rgb = np.fmin(ambient * color + diffuse * diff + specular * spec, 1.0)
            rgb = np.fmax(rgb, 0.0)
        bgr[yy, xx] = np.floor(rgb[:, ::-1] * 255.0 + 0.5).astype(np.uint8)

    bb = None
    if covered.any():
        yy, xx = np.nonzero(depth > 0)
        bb = calc_2d_bbox(xx, yy, (W, H))
    return dict(bgr=bgr, depth=depth, tri=tri, bb=bb)


def calc_2d_bbox(xs, ys, im_size):
    """pysixd/view_sampler.py:10-15."""
    bbTL = (max(xs.min() - 1, 0), max(ys.min() - 1, 0))
    bbBR = (min(xs.max() + 1, im_size[0] - 1), min(ys.max() + 1, im_size[1] - 1))
    return [int(bbTL[0]), int(bbTL[1]), int(bbBR[0] - bbTL[0]), int(bbBR[1] - bbTL[1])]


def resize_nearest(img, dst_w, dst_h):
    """cv2.resize(img, (dst_w, dst_h), interpolation=INTER_NEAREST): OpenCV imgproc resize.cpp resizeNN,
    source column min(floor(dx * (1 / (dst_w / src_w))), src_w - 1), rows alike."""
    src_h, src_w = img.shape[:2]
    ifx = 1.0 / (float(dst_w) / src_w)
    ify = 1.0 / (float(dst_h) / src_h)
    cols = np.minimum(np.floor(np.arange(dst_w) * ifx).astype(np.int64), src_w - 1)
    rows = np.minimum(np.floor(np.arange(dst_h) * ify).astype(np.int64), src_h - 1)
    return img[rows][:, cols]


def extract_square_patch(scene_img, bb_xywh, pad_factor, resize=(128, 128)):
    """dataset.py:354-373 with interpolation = INTER_NEAREST, black_borders = False."""
    x, y, w, h = np.array(bb_xywh).astype(np.int32)
    size = int(np.maximum(h, w) * pad_factor)
    left = int(np.maximum(x + w / 2 - size / 2, 0))
    right = int(np.minimum(x + w / 2 + size / 2, scene_img.shape[1]))
    top = int(np.maximum(y + h / 2 - size / 2, 0))
    bottom = int(np.minimum(y + h / 2 + size / 2, scene_img.shape[0]))
    scene_crop = scene_img[top:bottom, left:right].copy()
    return resize_nearest(scene_crop, resize[0], resize[1])


# ---- meshes of the tests ------------------------------------------------------------------------------------------
def torus_model(R=60.0, r=25.0, nu=24, nv=12):
    """A torus as load_ply would return it: 288 vertices, 576 faces, analytic normals, smoothly varying colours."""
    a = np.arange(nu) * 2 * np.pi / nu
    b = np.arange(nv) * 2 * np.pi / nv
    A, B = np.meshgrid(a, b, indexing='ij')
    pts = np.stack([(R + r * np.cos(B)) * np.cos(A), (R + r * np.cos(B)) * np.sin(A), r * np.sin(B)], axis=-1).reshape(-1, 3)
    normals = np.stack([np.cos(B) * np.cos(A), np.cos(B) * np.sin(A), np.sin(B)], axis=-1).reshape(-1, 3)
    colors = np.stack([140 + 100 * np.cos(A), 120 + 90 * np.sin(B), 130 + 80 * np.sin(A + B)], axis=-1).reshape(-1, 3)
    faces = []
    for i in range(nu):
        for j in range(nv):
            p00, p10 = i * nv + j, ((i + 1) % nu) * nv + j
            p01, p11 = i * nv + (j + 1) % nv, ((i + 1) % nu) * nv + (j + 1) % nv
            faces += [[p00, p10, p11], [p00, p11, p01]]
    return dict(pts=np.float32(pts).astype(np.float64), normals=np.float32(normals).astype(np.float64), colors=np.floor(colors),
                faces=np.array(faces, dtype=np.float64))


def box_model(sx=80.0, sy=60.0, sz=40.0):
    """A box of 12 large triangles with split vertices (24) and one colour per face."""
    h = np.array([sx, sy, sz]) / 2
    pts, normals, colors, faces = [], [], [], []
    palette = [(230, 60, 50), (60, 200, 80), (70, 90, 220), (220, 210, 60), (200, 70, 200), (60, 210, 210)]
    for axis in range(3):
        for sign in (-1, 1):
            n = np.zeros(3)
            n[axis] = sign
            u_ax, v_ax = (axis + 1) % 3, (axis + 2) % 3
            corners = []
            for cu, cv in ((-1, -1), (1, -1), (1, 1), (-1, 1)):
                p = np.zeros(3)
                p[axis] = sign * h[axis]
                p[u_ax] = cu * h[u_ax]
                p[v_ax] = cv * h[v_ax]
                corners.append(p)
            base = len(pts)
            pts += corners
            normals += [n] * 4
            colors += [palette[len(faces) // 2]] * 4
            quad = [0, 1, 2, 3] if sign > 0 else [0, 3, 2, 1]
            faces += [[base + quad[0], base + quad[1], base + quad[2]], [base + quad[0], base + quad[2], base + quad[3]]]
    return dict(pts=np.array(pts, dtype=np.float64), normals=np.array(normals, dtype=np.float64), colors=np.array(colors, dtype=np.float64),
                faces=np.array(faces, dtype=np.float64))


def degenerate_model():
    """The torus plus two zero-area faces (a repeated vertex) in front of and inside the face list, and one face whose three
    distinct vertices lie within a few ten nanometres of each other and so snap to the same 1/256-pixel point."""
    m = torus_model()
    n = len(m['pts'])
    base = m['pts'][5]
    extra = np.float32(np.stack([base, base + [3e-5, 0, 0], base + [0, 3e-5, 0]])).astype(np.float64)
    m['pts'] = np.concatenate([m['pts'], extra])
    m['normals'] = np.concatenate([m['normals'], np.repeat(m['normals'][5:6], 3, axis=0)])
    m['colors'] = np.concatenate([m['colors'], np.repeat(m['colors'][5:6], 3, axis=0)])
    f = m['faces']
    m['faces'] = np.concatenate([[[3, 3, 40]], f[:100], [[17, 90, 90]], f[100:], [[n, n + 1, n + 2]]]).astype(np.float64)
    return m


def write_ply(path, model, binary=False):
    """x y z nx ny nz (float) red green blue (uchar) + triangular faces, ascii or binary_little_endian."""
    pts, normals, colors, faces = model['pts'], model['normals'], model['colors'], model['faces'].astype(np.int64)
    header = ['ply', 'format %s 1.0' % ('binary_little_endian' if binary else 'ascii'), 'comment generated by the rasteriser tests',
              'element vertex %d' % len(pts), 'property float x', 'property float y', 'property float z',
              'property float nx', 'property float ny', 'property float nz',
              'property uchar red', 'property uchar green', 'property uchar blue',
              'element face %d' % len(faces), 'property list uchar int vertex_indices', 'end_header']
    with open(path, 'wb') as f:
        f.write(('\n'.join(header) + '\n').encode('ascii'))
        for p, n, c in zip(pts, normals, colors):
            if binary:
                f.write(struct.pack('<6f3B', *(list(p) + list(n) + [int(v) for v in c])))
            else:
                f.write((' '.join(['%.9g' % np.float32(v) for v in list(p) + list(n)] + ['%d' % int(v) for v in c]) + '\n').encode('ascii'))
        for a in faces:
            if binary:
                f.write(struct.pack('<B3i', 3, int(a[0]), int(a[1]), int(a[2])))
            else:
                f.write(('3 %d %d %d\n' % (a[0], a[1], a[2])).encode('ascii'))


def mesh_dict(arrays, vertex_scale=1.0):
    """meshrenderer.mesh_arrays output -> the mesh dict render() takes (vertices scaled in float32, as the vertex buffer holds them)."""
    verts, normals, colors, faces = arrays
    return dict(verts=(verts * np.float32(vertex_scale)).astype(np.float32), normals=normals, colors=colors, faces=faces)


# ---- cameras of the tests --------------------------------------------------------------------------------------------
TEMPLATE_K = np.array([1075.65, 0, 720 / 2, 0, 1073.90, 540 / 2, 0, 0, 1]).reshape(3, 3)     # cfg/train_template.cfg


def scaled_K(W, H):
    K = TEMPLATE_K.copy()
    K[0] *= W / 720.0
    K[1] *= H / 540.0
    return K


def random_rotations(n, seed):
    rng = np.random.RandomState(seed)
    out = []
    for _ in range(n):
        q, r = np.linalg.qr(rng.randn(3, 3))
        q = q * np.sign(np.diag(r))[None, :]
        if np.linalg.det(q) < 0:
            q[:, 0] = -q[:, 0]
        out.append(q)
    return np.array(out)
