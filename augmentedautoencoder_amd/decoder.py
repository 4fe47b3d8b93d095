"""``Decoder`` with the constructor and the inference properties of
/root/reference/auto_pose/ae/decoder.py:12-84, backed by the HIP decoder engine
(aae_decoder_* in include/aae_hip.h) instead of a TF graph.

Reference call sites kept working (auto_pose/eval/eval_plots.py:24-34,37-72,75-80):
    sess.run(decoder.x, feed_dict={encoder.x: crops})            # encode, then reconstruct
    sess.run(decoder.x, feed_dict={decoder._latent_code: codes}) # reconstruct given codes
and the number the training loop logs (auto_pose/ae/ae_train.py):
    sess.run(decoder.reconstr_loss, feed_dict={encoder.x: batch_x, decoder.reconstruction_target: batch_y})
The mask head (auxiliary_mask) and its loss are not provided."""
from __future__ import annotations

import numpy as np

from . import session as S
from .weights import DecoderConfig


class Decoder(object):

    def __init__(self, reconstruction_target, latent_code, num_filters, kernel_size, strides, loss='L2',
                 bootstrap_ratio=1, auxiliary_mask=False, batch_norm=False, is_training=False, encoder=None):
        """num_filters / strides arrive REVERSED, as ae_factory.build_decoder passes them
        (ae_factory.py:59-70).  latent_code: the encoder's z fetchable; encoder: the Encoder it
        belongs to (found through latent_code when omitted)."""
        if is_training:
            raise NotImplementedError('training graphs are out of scope; is_training must be False')
        self._reconstruction_target = reconstruction_target
        self._latent_code = latent_code
        self._auxiliary_mask = bool(auxiliary_mask)
        self._num_filters = list(num_filters)
        self._kernel_size = int(kernel_size)
        self._strides = list(strides)
        from .loss import loss_kind
        loss_kind(loss)                          # an unknown name is refused here (the reference prints and calls exit())
        self._loss = loss
        self._bootstrap_ratio = bootstrap_ratio
        self._batch_normalization = bool(batch_norm)
        self._is_training = False
        self._encoder = encoder if encoder is not None else getattr(latent_code, 'owner', None)
        shape = tuple(reconstruction_target.shape) if hasattr(reconstruction_target, 'shape') else tuple(reconstruction_target)
        latent = self._encoder.latent_space_size if self._encoder is not None else None
        if latent is None:
            raise ValueError('Decoder needs the encoder its latent code comes from (pass encoder=...)')
        self.config = DecoderConfig(shape[-3:], list(reversed(self._num_filters)), list(reversed(self._strides)),
                                    self._kernel_size, latent, self._batch_normalization, self._auxiliary_mask)
        self.weights = None
        self._engine = None
        self._device = None
        self._x_op = S.Op('decoder/x', self._run)
        self._loss_op = S.Op('decoder/reconstr_loss', lambda feed: self.reconstr_loss_device(feed)[0].cpu().numpy()[0])
        S.register(decoder=self)

    @property
    def reconstruction_target(self):
        return self._reconstruction_target

    @property
    def x(self):
        """Fetchable reconstruction [B,H,W,C] float32 in [0,1] (decoder.py:36-84)."""
        return self._x_op

    @property
    def reconstr_loss(self):
        """Fetchable float32 scalar (decoder.py:86-132): the decoder's `loss` ('L2' / 'L1') between the reconstruction and
        decoder.reconstruction_target, over the n // bootstrap_ratio largest errors of each image when bootstrap_ratio > 1.
        Feed encoder.x (or decoder._latent_code) and decoder.reconstruction_target."""
        if self._auxiliary_mask:
            raise NotImplementedError('auxiliary_mask=True adds the mask head (_xmask) and its mask loss to reconstr_loss; the decoder '
                                      'engine does not compute the mask head')
        return self._loss_op

    def reconstr_loss_device(self, feed, grad=False):
        """(loss [1], per_image [B], dx or None, reconstruction [B,H,W,C]) as device tensors: encode (or take the fed latent
        codes), decode and evaluate the loss without leaving the device."""
        from .loss import reconstruction_loss
        if self._auxiliary_mask:
            self.reconstr_loss
        target = None
        for k, v in feed.items():
            if k is self._reconstruction_target:
                target = v
        if target is None:
            raise ValueError('feed_dict has no value for decoder.reconstruction_target')
        x = self._reconstruct(feed)
        target = self.engine.target_batch(target, tuple(x.shape))
        loss, per_image, dx = reconstruction_loss(x, target, loss=self._loss, bootstrap_ratio=self._bootstrap_ratio, grad=grad)
        return loss, per_image, dx, x

    def gradients_device(self, feed):
        """(loss [1], OrderedDict variable name -> gradient, dz) as device tensors: decode, the loss with its gradient, the decoder's
        backward pass.  Nothing is updated: there is no optimiser behind this."""
        from .decoder_grad import check_trainable
        check_trainable(self.config)
        z = None
        for k, v in feed.items():
            if k is self._latent_code:
                z = self.engine._z(v if hasattr(v, 'is_cuda') else np.asarray(v, dtype=np.float32))
        if z is None:
            if self._encoder is None:
                raise ValueError('feed_dict has no value for decoder._latent_code')
            z = self.engine._z(self._encoder.engine.encode_checked(self._encoder._feed(feed)))
        feed = dict(feed)
        feed[self._latent_code] = z
        loss, _, dx, x = self.reconstr_loss_device(feed, grad=True)
        grads, dz = self.engine.backward(z, x, dx)
        return loss, grads, dz

    # -- plumbing ------------------------------------------------------------------
    def load_weights(self, weights, device=None):
        """Stand-in for Saver.restore on the decoder variables (dense_1, conv2d_<L>.., BN)."""
        self.weights = {k: np.asarray(v) for k, v in weights.items()}
        self._device = device
        if self._engine is not None:
            self._engine.close()
            self._engine = None

    def close(self):
        """Free the device weights now and leave the module registry."""
        if self._engine is not None:
            self._engine.close()
            self._engine = None
        S.unregister(self)

    @property
    def engine(self):
        if self._engine is None:
            if self.weights is None:
                raise RuntimeError('decoder has no weights: restore a checkpoint (factory.restore_checkpoint) '
                                   'or call Decoder.load_weights first')
            from .engine import DecoderEngine
            self._engine = DecoderEngine(self.config, self.weights, device=self._device)
        return self._engine

    def _reconstruct(self, feed):
        """Decoder.x as a device tensor"""
        for k, v in feed.items():
            if k is self._latent_code:
                return self.engine.decode(v if hasattr(v, 'is_cuda') else np.asarray(v, dtype=np.float32))
        if self._encoder is None:
            raise ValueError('feed_dict has no value for decoder._latent_code')
        z = self._encoder.engine.encode_checked(self._encoder._feed(feed))  # stays on the device
        return self.engine.decode(z)

    def _run(self, feed):
        return self._reconstruct(feed).cpu().numpy()
