"""``AE`` with the constructor and properties of the reference's auto_pose/ae/ae.py:11-53: the encoder and decoder of one
autoencoder and the loss its training minimises, as a fetchable evaluated on the device; gradients_device() adds the decoder's
backward pass, variable_gradients_device() the encoder's behind it (the optimiser is not built)."""
from __future__ import annotations

import numpy as np

from . import session as S


class AE(object):

    def __init__(self, encoder, decoder, norm_regularize, variational):
        if variational:
            raise NotImplementedError('variational = %r adds the KL term over the q_sigma head (encoder.py:70-94), which this package '
                                      'does not have' % (variational,))
        self._encoder = encoder
        self._decoder = decoder
        self._norm_regularize = float(norm_regularize)
        self._variational = variational
        decoder.reconstr_loss                          # as the reference builds the loss here: an unsupported decoder is refused now
        self._global_step = np.int64(0)
        self._loss_op = S.Op('ae/loss', self._loss)
        self._step_op = S.Op('ae/global_step', lambda feed: np.int64(self._global_step))

    @property
    def x(self):
        return self._encoder.x

    @property
    def z(self):
        return self._encoder.z

    @property
    def reconstruction(self):
        return self._decoder.x

    @property
    def reconstruction_target(self):
        return self._decoder.reconstruction_target

    @property
    def global_step(self):
        """Fetchable int64 (ae.py:38-40): 0 until something restores it."""
        return self._step_op

    @property
    def loss(self):
        """Fetchable float32 scalar (ae.py:42-53): reconstr_loss + reg_loss * float32(norm_regularize) when norm_regularize > 0."""
        return self._loss_op

    def loss_device(self, feed):
        """the loss as a device tensor [1]: one encode, one decode, the two loss calls, one fp32 multiply-add"""
        import torch
        dec, enc = self._decoder, self._encoder
        if self._norm_regularize > 0 and not any(k is dec._latent_code for k in feed):
            z = enc.engine.encode_checked(enc._feed(feed))
            feed = dict(feed)
            feed[dec._latent_code] = z
        loss = dec.reconstr_loss_device(feed)[0]
        if self._norm_regularize > 0:
            z = next(v for k, v in feed.items() if k is dec._latent_code)
            z = dec.engine._z(z)
            reg = enc.reg_loss_device(feed, z=z)[0]
            loss = loss + reg * torch.tensor(np.float32(self._norm_regularize), dtype=torch.float32, device=loss.device)
        return loss

    def gradients_device(self, feed):
        """(loss [1], OrderedDict decoder variable -> gradient, dz) as device tensors: the loss of AE.loss, the gradient of every
        decoder variable, and dL/dz with float32(norm_regularize) * d(reg_loss)/dz added in -- what an encoder backward starts from."""
        import torch
        dec, enc = self._decoder, self._encoder
        z = next((v for k, v in feed.items() if k is dec._latent_code), None)
        if z is None:
            z = enc.engine.encode_checked(enc._feed(feed))
        z = dec.engine._z(z)
        feed = dict(feed)
        feed[dec._latent_code] = z
        loss, grads, dz = dec.gradients_device(feed)
        if self._norm_regularize > 0:
            from .loss import latent_reg_loss
            reg, dz_reg = latent_reg_loss(z, grad=True)
            scale = torch.tensor(np.float32(self._norm_regularize), dtype=torch.float32, device=loss.device)
            loss = loss + reg * scale
            dz = dz + dz_reg * scale
        return loss, grads, dz

    def variable_gradients_device(self, feed):
        """(loss [1], OrderedDict variable -> gradient) as device tensors, over every encoder variable and then every decoder
        variable, in checkpoint shapes: gradients_device() of a batch encoded here, then the encoder's backward pass from its dz.
        The latent code is computed from the encoder's input: a feed that supplies decoder._latent_code has no encoder gradient."""
        import collections
        dec, enc = self._decoder, self._encoder
        if any(k is dec._latent_code for k in feed):
            raise ValueError('variable_gradients_device differentiates through the encoder: feed its input, not decoder._latent_code')
        enc.engine.check_trainable()
        loss, dec_grads, dz = self.gradients_device(feed)
        enc_grads, _ = enc.gradients_device(feed, dz.contiguous())
        grads = collections.OrderedDict(enc_grads)
        for name, g in dec_grads.items():
            if name in grads:
                raise ValueError('the encoder and the decoder both have a variable named %r' % name)
            grads[name] = g
        return loss, grads

    def _loss(self, feed):
        return self.loss_device(feed).cpu().numpy()[0]
