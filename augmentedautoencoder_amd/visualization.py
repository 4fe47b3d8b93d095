"""``PoseVisualizer`` with the signature of the reference's visualization/render_pose.py: the estimated poses of a frame drawn
into the camera image.  All models of the estimator are rendered at their poses into one frame with one depth buffer
(``Renderer.render_scenes``, one call), and the green channel of the render is blended over the image on the GPU
(``aae_overlay_blend``: the reference's ``g_y*2./3. + image*1./3.`` bit for bit).

Deviations from the reference, all of them on the output side:
  * no window is opened: ``cv2.imshow`` / ``cv2.waitKey`` are not called and ``waitKey`` is ignored; the blended image is returned;
  * ``vis_bbs`` draws the detection boxes and labels only when ``cv2`` can be imported, else it is skipped;
  * ``downsample != 1`` raises NotImplementedError (the reference resizes with cv2's bilinear filter);
  * ``all_pose_estimates_rgb is not None`` raises NotImplementedError (the reference's branch reads an undefined name,
    ``all_class_idcs``);
  * ``depth_image`` is accepted and not drawn (the reference shows it in a second window).
Translations are read from ``trafo[:3, 3]`` as they stand, as the reference reads them: millimetres."""
from __future__ import annotations

import numpy as np

from . import meshrenderer

NEAR, FAR = 10, 10000                        # render_pose.py:37-38


class PoseVisualizer(object):

    def __init__(self, ae_pose_est, downsample=1):
        self.downsample = downsample
        self.classes = list(ae_pose_est.class_2_encoder.keys())
        self.vertex_scale = list(set([ae_pose_est.all_train_args[c].getint('Dataset', 'VERTEX_SCALE') for c in self.classes]))
        self.ply_model_paths = [str(ae_pose_est.all_train_args[c].get('Paths', 'MODEL_PATH')) for c in self.classes]
        self._renderer = None

    @property
    def renderer(self):
        """Created at first use, of kind 'cad' (the reference builds meshrenderer.Renderer, render_pose.py:20-25)."""
        if self._renderer is None:
            self._renderer = meshrenderer.Renderer(self.ply_model_paths, samples=1, vertex_tmp_store_folder='.',
                                                   vertex_scale=float(self.vertex_scale[0]), model='cad')      # 1000 for models in meters
        return self._renderer

    def _check(self, all_pose_estimates_rgb):
        if self.downsample != 1:
            raise NotImplementedError('downsample = %r: only 1 is implemented (the reference resizes the image with cv2)' % (self.downsample,))
        if all_pose_estimates_rgb is not None:
            raise NotImplementedError('all_pose_estimates_rgb: not implemented (the reference\'s branch reads the undefined name all_class_idcs)')

    def _blend_frames(self, images, camK, pose_ests_per_image):
        """images uint8 [S,H,W,3] -> blended uint8 [S,H,W,3] on the host; one scene per image."""
        import torch
        S, H, W = images.shape[:3]
        obj_ids, scene_ids, Rs, ts = [], [], [], []
        for s, pose_ests in enumerate(pose_ests_per_image):
            for pose_est in pose_ests:
                obj_ids.append(self.classes.index(pose_est.name))
                scene_ids.append(s)
                Rs.append(np.asarray(pose_est.trafo, dtype=np.float64)[:3, :3])
                ts.append(np.asarray(pose_est.trafo, dtype=np.float64)[:3, 3])
        if not obj_ids:
            return images.copy()
        r = self.renderer
        bgr, _, _, vis = r.render_scenes(obj_ids, scene_ids, S, W, H, np.asarray(camK, dtype=np.float64).copy(), np.asarray(Rs), np.asarray(ts), NEAR, FAR)
        shown = r.overlay_blend(torch.as_tensor(np.ascontiguousarray(images), device=bgr.device), bgr, channel=1)
        vis = vis.cpu().numpy()
        for d in range(len(obj_ids)):
            if not vis[d]:                                                   # the reference: ValueError from calc_2d_bbox in render_many
                raise ValueError('render_poses: draw %d (obj_id %d, image %d) covers no pixel' % (d, obj_ids[d], scene_ids[d]))
        return shown.cpu().numpy()

    def render_poses(self, image, camK, pose_ests, dets, vis_bbs=True, vis_mask=False, all_pose_estimates_rgb=None, depth_image=None, waitKey=True):
        """render_pose.py:27-93: image uint8 [H,W,3] BGR with the models of pose_ests (PoseEstimate: name, trafo) drawn over it in
        green -> image_show uint8 [H,W,3]; the input is not modified."""
        self._check(all_pose_estimates_rgb)
        image = np.asarray(image)
        if image.dtype != np.uint8 or image.ndim != 3 or image.shape[2] != 3:
            raise ValueError('render_poses: image must be uint8 [H,W,3], got %s %s' % (image.dtype, image.shape))
        image_show = self._blend_frames(image[None], camK, [pose_ests])[0]
        if vis_bbs:
            self._draw_boxes(image_show, dets)
        return image_show

    def render_poses_batch(self, images, camK, pose_ests_per_image):
        """A list of frames of one size through one render call, one scene per image -> uint8 [S,H,W,3]; image s equals
        render_poses(images[s], camK, pose_ests_per_image[s], [], vis_bbs=False)."""
        self._check(None)
        images = np.stack([np.asarray(im) for im in images])
        if images.dtype != np.uint8 or images.ndim != 4 or images.shape[3] != 3:
            raise ValueError('render_poses_batch: images must be uint8 [H,W,3] of one size, got %s %s' % (images.dtype, images.shape))
        if len(pose_ests_per_image) != len(images):
            raise ValueError('render_poses_batch: %d images, %d lists of poses' % (len(images), len(pose_ests_per_image)))
        return self._blend_frames(images, camK, pose_ests_per_image)

    @staticmethod
    def _draw_boxes(image_show, dets):
        try:
            import cv2
        except ImportError:
            return
        H_d, W_d = image_show.shape[:2]
        for det in dets:
            xmin, ymin, xmax, ymax = int(det.xmin * W_d), int(det.ymin * H_d), int(det.xmax * W_d), int(det.ymax * H_d)
            label, score = list(det.classes.items())[0]
            cv2.putText(image_show, '%s : %1.3f' % (label, score), (xmin, ymax + 20), cv2.FONT_ITALIC, .5, (0, 0, 255), 2)
            cv2.rectangle(image_show, (xmin, ymin), (xmax, ymax), (255, 0, 0), 2)

    def close(self):
        if self._renderer is not None:
            self._renderer.close()
        self._renderer = None
