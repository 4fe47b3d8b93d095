"""The slice of ``Dataset`` (the reference's auto_pose/ae/dataset.py) that starts from a mesh and a cfg: the cfg keyword bag,
the crop shape, the codebook-row -> rotation table, the hook through which update_embedding obtains the views to embed, and
the training set (``get_training_images`` / ``render_training_images``: the ``<md5>.npz`` the reference's ``ae_train``
looks for first).

``render_embedding_image_batch`` delegates to a pluggable *view source*; ``MeshViewSource`` is the one that renders the
object's mesh on the GPU (meshrenderer.py, the HIP rasteriser) in place of the reference's OpenGL context.  The training
pairs come from the same rasteriser (``Renderer.render_training_views``): the images are this rasteriser's, not an OpenGL
driver's, and parity with a driver is unpinned exactly as for the codebook views.

``load_bg_images``, ``batch`` and ``batch_device`` are the training loop's side (dataset.py:146-174, 456-495): the background
composite, the ``[Augmentation] CODE`` chain and the /255 run as one HIP launch per batch (augmentation.py; imgaug and cv2 are
not dependencies).  The two occlusion switches and every augmenter outside the template's seven are refused by name.
"""
from __future__ import annotations

import ast
import glob
import hashlib
import os

import numpy as np

from . import viewsphere as vs
from .utils import lazy_property

_VIEWSPHERE_CACHE = {}


class SyntheticViewSource(object):
    """Deterministic stand-in for the renderer: view i is a smooth pattern whose
    phase/orientation follow rotation i, on a black background, as uint8."""

    def __init__(self, shape, seed=0):
        self.shape = tuple(shape)
        self.seed = int(seed)

    def __call__(self, start, end, Rs):
        H, W, C = self.shape
        yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
        yy = (yy - H / 2.0) / H
        xx = (xx - W / 2.0) / W
        n = end - start
        batch = np.empty((n, H, W, C), dtype=np.uint8)
        bbs = np.empty((n, 4))
        for k in range(n):
            R = Rs[k]
            u = R[0, 0] * xx + R[0, 1] * yy
            v = R[1, 0] * xx + R[1, 1] * yy
            mask = (u * u / 0.16 + v * v / (0.04 + 0.1 * abs(R[2, 2]))) < 1.0
            img = np.zeros((H, W, C))
            for c in range(C):
                img[..., c] = 127.5 + 127.5 * np.sin(6.0 * (R[2, c % 3] + 1.5) * u + 9.0 * R[c % 3, 2] * v + self.seed)
            img *= mask[..., None]
            batch[k] = np.clip(img, 0, 255).astype(np.uint8)
            ys, xs = np.nonzero(mask)
            if len(xs):
                bbs[k] = vs_calc_2d_bbox(xs, ys, (W, H))
            else:
                bbs[k] = (0, 0, 1, 1)
        return batch, bbs

    def torch_batch(self, Rs, device, noise=None):
        """The same pattern for a whole stack of rotations at once, evaluated with framework tensor ops on ``device``
        (float64): uint8 [n,H,W,C] device tensor, no bounding boxes.  Input plumbing for full-size codebook builds in
        tests and benchmarks (92232 views in seconds instead of minutes); rounding may differ from __call__ in the
        last grey level, so a codebook and its queries must come from the same method.  noise: optional float tensor
        [n,H,W,C] added before the uint8 conversion."""
        import torch
        H, W, C = self.shape
        R = torch.as_tensor(np.asarray(Rs, dtype=np.float64), device=device).reshape(-1, 3, 3)
        yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float64, device=device), torch.arange(W, dtype=torch.float64, device=device),
                                indexing='ij')
        yy = ((yy - H / 2.0) / H)[None]
        xx = ((xx - W / 2.0) / W)[None]
        r = lambda i, j: R[:, i, j].reshape(-1, 1, 1)
        u = r(0, 0) * xx + r(0, 1) * yy
        v = r(1, 0) * xx + r(1, 1) * yy
        mask = (u * u / 0.16 + v * v / (0.04 + 0.1 * r(2, 2).abs())) < 1.0
        chans = [127.5 + 127.5 * torch.sin(6.0 * (r(2, c % 3) + 1.5) * u + 9.0 * r(c % 3, 2) * v + self.seed) for c in range(C)]
        img = torch.stack(chans, dim=-1) * mask[..., None]
        if noise is not None:
            img = img + noise
        return img.clamp(0, 255).to(torch.uint8)


def vs_calc_2d_bbox(xs, ys, im_size):
    """pysixd_stuff/view_sampler.py:10-15."""
    tl = (max(xs.min() - 1, 0), max(ys.min() - 1, 0))
    br = (min(xs.max() + 1, im_size[0] - 1), min(ys.max() + 1, im_size[1] - 1))
    return [tl[0], tl[1], br[0] - tl[0], br[1] - tl[1]]


class MeshViewSource(object):
    """The view source that does what dataset.py:308-352 does: render codebook rows [start,end) of the dataset's mesh
    (Renderer.render at t = (0, 0, RADIUS)), take calc_2d_bbox of the depth, and cut the padded square patch resized with
    INTER_NEAREST -- on the GPU, for the whole batch in one call.  Returns (uint8 device tensor [n,H,W,3] BGR, numpy obj_bbs
    [n,4]); Codebook.update_embedding feeds the tensor to the encoder as it is, the views never visit the host.
    Raises ValueError naming the first row whose view covers no pixel (the reference's ValueError from calc_2d_bbox on an
    empty selection, dataset.py:273-277 -- 'Have you scaled the vertices to mm?')."""

    def __init__(self, dataset):
        from .codebook import _parse_K
        kw = dataset._kw
        h, w, c = dataset.shape
        if c != 3:
            raise NotImplementedError('C = %d: the grey-scale conversion (cv2.cvtColor, dataset.py:349-350) is not implemented; use C = 3' % c)
        if h != w:
            raise NotImplementedError('H = %d, W = %d: only square crops (the reference hands shape[:2] to cv2.resize as (width, height), '
                                      'dataset.py:347, and is only right for squares)' % (h, w))
        self.dataset = dataset
        self.crop = int(h)
        self.renderer = dataset.renderer
        dims = _parse_K(kw['render_dims'])
        if not isinstance(dims, list) or len(dims) != 2:
            raise ValueError('[Dataset] RENDER_DIMS must be (width, height), got %r' % (kw['render_dims'],))
        self.render_dims = (int(dims[0]), int(dims[1]))
        self.K = np.array(_parse_K(kw['k']), dtype=np.float64).reshape(3, 3)
        self.clip_near = float(kw['clip_near'])
        self.clip_far = float(kw['clip_far'])
        self.pad_factor = float(kw['pad_factor'])
        self.t = np.array([0, 0, float(kw['radius'])])

    def __call__(self, start, end, Rs):
        crops, bbs, visible = self.renderer.render_embedding_views(0, self.render_dims[0], self.render_dims[1], self.K, Rs, self.t,
                                                                   self.clip_near, self.clip_far, self.pad_factor, self.crop)
        hidden = np.nonzero(visible.cpu().numpy() == 0)[0]
        if len(hidden):
            raise ValueError('Object in Rendering not visible (codebook row %d). Have you scaled the vertices to mm?' % (start + int(hidden[0])))
        return crops, bbs.cpu().numpy().astype(np.float64)


class Dataset(object):

    def __init__(self, dataset_path, **kw):
        self.shape = (int(kw['h']), int(kw['w']), int(kw['c']))
        self.dataset_path = dataset_path
        self._kw = kw
        self._view_source = None

    def set_view_source(self, fn):
        """fn(start, end, Rs[start:end]) -> (batch [n,H,W,C] uint8 or float in [0,1], obj_bbs [n,4])."""
        self._view_source = fn

    @lazy_property
    def viewsphere_for_embedding(self):
        kw = self._kw
        key = (int(kw['min_n_views']), float(kw['radius']), int(kw['num_cyclo']))
        if key not in _VIEWSPHERE_CACHE:
            _VIEWSPHERE_CACHE[key] = vs.viewsphere_for_embedding(*key)
        return _VIEWSPHERE_CACHE[key]

    @lazy_property
    def renderer(self):
        """dataset.py:60-80: the renderer of [Dataset] MODEL / MODEL_PATH / ANTIALIASING / VERTEX_SCALE (here VERTEX_SCALE
        scales both kinds of model; the reference's reconst call hands it to the unused ``clamp`` parameter)."""
        from . import meshrenderer
        kw = self._kw
        kind = kw.get('model')
        if kind not in meshrenderer.MODEL_KINDS:
            raise ValueError("[Dataset] MODEL must be 'cad' or 'reconst', got %r" % (kind,))
        path = kw.get('model_path')
        if not path or not os.path.isfile(path):
            raise FileNotFoundError('[Paths] MODEL_PATH: no such file: %s' % (path,))
        return meshrenderer.Renderer([path], int(kw.get('antialiasing', 1)), self.dataset_path, float(kw.get('vertex_scale', 1.0)), model=kind)

    @property
    def embedding_size(self):
        return len(self.viewsphere_for_embedding)

    # ---- the training set (dataset.py:82-95, 219-306, 354-373) -------------------------------------------------------
    @lazy_property
    def noof_training_imgs(self):
        return int(self._kw['noof_training_imgs'])

    def get_training_images(self, dataset_path, args, batch=256):
        """dataset.py:82-95: load <md5 of the [Dataset] and [Paths] items>.npz from dataset_path, or render the training set
        and write it there (train_x, mask_x, train_y); returns the file's path."""
        current_config_hash = hashlib.md5((str(args.items('Dataset') + args.items('Paths'))).encode('utf-8')).hexdigest()
        current_file_name = os.path.join(dataset_path, current_config_hash + '.npz')
        if os.path.exists(current_file_name):
            training_data = np.load(current_file_name)
            self.train_x = training_data['train_x'].astype(np.uint8)
            self.mask_x = training_data['mask_x']
            self.train_y = training_data['train_y'].astype(np.uint8)
        else:
            self.render_training_images(batch)
            np.savez(current_file_name, train_x=self.train_x, mask_x=self.mask_x, train_y=self.train_y)
        self.noof_obj_pixels = np.count_nonzero(self.mask_x == 0, axis=(1, 2))
        print('loaded %s training images' % len(self.train_x))
        return current_file_name

    def render_training_images(self, batch=256):
        """dataset.py:219-306 on the GPU: train_x uint8 [N,H,W,3] (random light, cut around a randomly shifted box), mask_x bool
        [N,H,W] (its background), train_y uint8 [N,H,W,3] (default light, true box) as host arrays, `batch` pairs a call.
        np.random is consumed in the reference's order (meshrenderer.draw_training_params), all of it before the first
        launch.  Deviation: an image whose view covers no pixel raises ValueError naming it; the reference prints the same
        hint and leaves the loop with the rest of its arrays uninitialised."""
        from . import meshrenderer
        src = MeshViewSource(self)                               # the cfg parsing and the C = 1 / non-square errors of the codebook views
        n = self.noof_training_imgs
        max_rel_offset = float(self._kw['max_rel_offset'])
        Rs, lights, offsets = meshrenderer.draw_training_params(n, max_rel_offset, self._kw['model'])
        self.train_x = np.empty((n,) + self.shape, dtype=np.uint8)
        self.mask_x = np.empty((n,) + self.shape[:2], dtype=bool)
        self.train_y = np.empty((n,) + self.shape, dtype=np.uint8)
        batch = max(1, int(batch))
        for a in range(0, n, batch):
            e = min(a + batch, n)
            x, m, y, _, visible = src.renderer.render_training_views(0, src.render_dims[0], src.render_dims[1], src.K, Rs[a:e], src.t, src.clip_near,
                                                                     src.clip_far, src.pad_factor, src.crop, lights[a:e], offsets[a:e])
            hidden = np.nonzero(visible.cpu().numpy() == 0)[0]
            if len(hidden):
                raise ValueError('Object in Rendering not visible (training image %d). Have you scaled the vertices to mm?' % (a + int(hidden[0])))
            self.train_x[a:e] = x.cpu().numpy()
            self.mask_x[a:e] = m.cpu().numpy()
            self.train_y[a:e] = y.cpu().numpy()

    # ---- the training batches (dataset.py:24-25, 146-174, 456-495) ----------------------------------------------------------
    @lazy_property
    def bg_img_paths(self):
        return glob.glob(self._kw['background_images_glob'])

    @lazy_property
    def noof_bg_imgs(self):
        return min(int(self._kw['noof_bg_imgs']), len(self.bg_img_paths))

    @lazy_property
    def _aug_plan(self):
        from . import augmentation
        return augmentation.parse_code(self._kw['code'])

    def _refuse_occlusion(self):
        """REALISTIC_OCCLUSION / SQUARE_OCCLUSION (dataset.py:470-474): rejection loops over mask data this package has no file
        format for; the template has both off"""
        for key in ('realistic_occlusion', 'square_occlusion'):
            if ast.literal_eval(str(self._kw.get(key, 'False')).strip()):
                raise NotImplementedError('[Augmentation] %s: %s is not implemented; set it to False' % (key.upper(), self._kw[key]))

    def load_bg_images(self, dataset_path):
        """dataset.py:146-174: bg_imgs uint8 [noof_bg_imgs,H,W,C] from <md5(str(shape) + str(noof_bg_imgs) + str(glob))>.npy in
        dataset_path, or cut from the first noof_bg_imgs files of the glob at random anchors (random.shuffle of the list, then
        np.random.rand() for y and for x per file, the reference's order) and saved there.  Deviations: the array starts as zeros
        (the reference leaves np.empty garbage for a file it skips as too small), and files are decoded by PIL's codecs into BGR,
        not by cv2.imread (JPEG decoders may differ in the last grey level).  PIL is imported only when files are decoded."""
        name = hashlib.md5((str(self.shape) + str(self.noof_bg_imgs) + str(self._kw['background_images_glob'])).encode('utf-8')).hexdigest()
        current_file_name = os.path.join(dataset_path, name + '.npy')
        if os.path.exists(current_file_name):
            self.bg_imgs = np.load(current_file_name)
        else:
            from random import shuffle
            from PIL import Image
            h, w, c = self.shape
            if c != 3:
                raise NotImplementedError('C = %d: the grey-scale conversion (cv2.cvtColor, dataset.py:167-168) is not implemented; use C = 3' % c)
            self.bg_imgs = np.zeros((self.noof_bg_imgs,) + self.shape, dtype=np.uint8)
            file_list = self.bg_img_paths[:self.noof_bg_imgs]
            shuffle(file_list)
            for j, fname in enumerate(file_list):
                with Image.open(fname) as im:
                    bgr = np.asarray(im.convert('RGB'))[:, :, ::-1]
                H, W = bgr.shape[:2]
                y_anchor = int(np.random.rand() * (H - h))
                x_anchor = int(np.random.rand() * (W - w))
                bgr = bgr[y_anchor:y_anchor + h, x_anchor:x_anchor + w, :]
                if bgr.shape[0] != h or bgr.shape[1] != w:
                    continue
                self.bg_imgs[j] = bgr
            np.save(current_file_name, self.bg_imgs)
        print('loaded %s bg images' % self.noof_bg_imgs)
        return current_file_name

    def to_device(self, device='cuda'):
        """train_x, mask_x, train_y and bg_imgs uploaded once; batch_device and batch read them from there"""
        import torch
        from . import augmentation
        augmentation.check_image_bytes(self.shape)
        up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).astype(dt, copy=False)).to(device)
        if np.shape(self.train_x)[1:] != np.shape(self.bg_imgs)[1:]:
            raise ValueError('training images of %s, backgrounds of %s' % (np.shape(self.train_x)[1:], np.shape(self.bg_imgs)[1:]))
        self._device_arrays = (up(self.train_x, np.uint8), up(self.mask_x, bool), up(self.train_y, np.uint8), up(self.bg_imgs, np.uint8))
        return self

    def _draw_batch(self, batch_size):
        """np.random in the reference's order: the two choice(..., replace=False) calls of dataset.py:461-465, then -- on the first
        batch only -- whatever np.random.rand() the CODE text holds (the reference's lazy ``_aug`` is first touched at
        dataset.py:488, after the choices), then draw_programs"""
        from . import augmentation
        self._refuse_occlusion()
        n_train, n_bg = len(self.train_x), len(self.bg_imgs)            # the reference's noof_training_imgs and noof_bg_imgs
        rand_idcs = np.random.choice(n_train, batch_size, replace=False)
        assert n_bg > 0
        rand_idcs_bg = np.random.choice(n_bg, batch_size, replace=False)
        plan = self._aug_plan
        return rand_idcs, rand_idcs_bg, augmentation.draw_programs(plan, batch_size, self.train_x.shape[1:])

    def _on_device(self):
        if not hasattr(self, '_device_arrays'):
            self.to_device()
        return self._device_arrays

    def batch_device(self, batch_size):
        """dataset.py:456-495 as one launch: (batch_x, batch_y) float32 device tensors [batch_size,H,W,C] in [0,1]"""
        from . import augmentation
        rand_idcs, rand_idcs_bg, programs = self._draw_batch(batch_size)
        _, x, y = augmentation.run_batch(*self._on_device(), rand_idcs, rand_idcs_bg, programs, want_u8=False)
        return x, y

    def batch(self, batch_size):
        """dataset.py:456-495: (batch_x, batch_y) as the reference returns them, NumPy float64 ``uint8 / 255.``, batch_x from the
        kernel's uint8 output"""
        from . import augmentation
        rand_idcs, rand_idcs_bg, programs = self._draw_batch(batch_size)
        x, _, _ = augmentation.run_batch(*self._on_device(), rand_idcs, rand_idcs_bg, programs, want_x=False, want_y=False)
        return x.cpu().numpy() / 255., np.asarray(self.train_y)[rand_idcs] / 255.

    def extract_square_patch(self, scene_img, bb_xywh, pad_factor, resize=(128, 128), interpolation='nearest', black_borders=False):
        """dataset.py:354-373 on the host in NumPy, with cv2.resize(INTER_NEAREST) restated (OpenCV resize.cpp, resizeNN);
        interpolation: 'nearest' or cv2.INTER_NEAREST's value 0, anything else raises NotImplementedError."""
        if not (interpolation == 'nearest' or (not isinstance(interpolation, str) and interpolation == 0)):
            raise NotImplementedError('extract_square_patch: only nearest-neighbour interpolation is implemented, got %r' % (interpolation,))
        scene_img = np.asarray(scene_img)
        x, y, w, h = np.array(bb_xywh).astype(np.int32)
        size = int(np.maximum(h, w) * pad_factor)
        left = int(np.maximum(x + w / 2 - size / 2, 0))
        right = int(np.minimum(x + w / 2 + size / 2, scene_img.shape[1]))
        top = int(np.maximum(y + h / 2 - size / 2, 0))
        bottom = int(np.minimum(y + h / 2 + size / 2, scene_img.shape[0]))
        scene_crop = scene_img[top:bottom, left:right].copy()
        if black_borders:
            scene_crop[:(y - top), :] = 0
            scene_crop[(y + h - top):, :] = 0
            scene_crop[:, :(x - left)] = 0
            scene_crop[:, (x + w - left):] = 0
        src_h, src_w = scene_crop.shape[:2]
        dst_w, dst_h = int(resize[0]), int(resize[1])
        cols = np.minimum(np.floor(np.arange(dst_w) * (1.0 / (float(dst_w) / src_w))).astype(np.int64), src_w - 1)
        rows = np.minimum(np.floor(np.arange(dst_h) * (1.0 / (float(dst_h) / src_h))).astype(np.int64), src_h - 1)
        return scene_crop[rows][:, cols]

    def render_embedding_image_batch(self, start, end):
        """(batch float64 in [0,1] or uint8, obj_bbs) for codebook rows [start,end)
        (dataset.py:308-352, with the OpenGL render behind the view source)."""
        if self._view_source is None:
            raise NotImplementedError(
                'Rendering is out of scope of this package: attach a view source with '
                'Dataset.set_view_source(fn) (e.g. pre-rendered views, or SyntheticViewSource).')
        return self._view_source(start, end, self.viewsphere_for_embedding[start:end])
