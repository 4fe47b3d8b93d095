"""The number the reference's training loop minimises, evaluated on the device: ``Decoder.reconstr_loss``
(the reference's auto_pose/ae/decoder.py:86-132: L2 or L1, bootstrapped over the ``n // bootstrap_ratio`` largest errors of each
image) and ``Encoder.reg_loss`` (encoder.py:97-100), each with its gradient with respect to the tensor it reads
(aae_recon_loss / aae_latent_reg_loss in include/aae_hip.h).  Device tensors in, device tensors out: no
host copy, no synchronisation."""
from __future__ import annotations

import ctypes

from . import _lib

KINDS = {'L2': _lib.AAE_LOSS_L2, 'L1': _lib.AAE_LOSS_L1}


def loss_kind(name):
    """'L2' / 'L1' -> AAE_LOSS_*; anything else is a ValueError (the reference prints and calls exit())."""
    if name not in KINDS:
        raise ValueError('unknown loss %r: the reconstruction loss is one of %s' % (name, sorted(KINDS)))
    return KINDS[name]


def check_bootstrap_ratio(ratio, n=None):
    if isinstance(ratio, bool) or int(ratio) != ratio or int(ratio) < 1:
        raise ValueError('bootstrap_ratio must be an integer >= 1, got %r' % (ratio,))
    if n is not None and n // int(ratio) < 1:
        raise ValueError('bootstrap_ratio %d selects n // ratio = 0 of the %d elements of an image' % (int(ratio), n))
    return int(ratio)


def _device_f32(t, name, dev=None):
    import torch
    if not isinstance(t, torch.Tensor):
        raise ValueError('%s must be a torch tensor on the GPU, got %s' % (name, type(t).__name__))
    if t.dtype != torch.float32:
        raise ValueError('%s has dtype %s, float32 is expected' % (name, t.dtype))
    if not t.is_cuda:
        raise ValueError('%s lives on %s, a GPU tensor is expected' % (name, t.device))
    if dev is not None and t.device != dev:
        raise ValueError('%s lives on %s, the other tensors on %s' % (name, t.device, dev))
    if not t.is_contiguous():
        raise ValueError('%s must be contiguous' % name)
    return t


def _out(t, name, shape, dev):
    _device_f32(t, name, dev)
    if tuple(t.shape) != tuple(shape):
        raise ValueError('%s has shape %s, this call writes %s' % (name, tuple(t.shape), tuple(shape)))
    return t


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream(torch, dev):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def reconstruction_loss(x, target, loss='L2', bootstrap_ratio=1, grad=False, out=None, workspace=None):
    """x / target: contiguous float32 device tensors [B, ...] of one shape (a reconstruction and its target).  Returns
    (loss [1], per_image [B], dx or None), all on the device: per_image[b] is the mean of image b's selected errors, loss their
    mean over B, dx (grad=True; the shape of x) the gradient of loss with respect to x.  out=(loss, per_image, dx): the caller's
    tensors to write into (dx None for no gradient); workspace: a caller's uint8 device tensor of at least
    aae_recon_loss_workspace_bytes(B, n) bytes.  Two launches on the current stream."""
    import torch
    kind = loss_kind(loss)
    _device_f32(x, 'x')
    dev = x.device
    _device_f32(target, 'target', dev)
    if x.dim() < 1 or tuple(x.shape) != tuple(target.shape):
        raise ValueError('x has shape %s, target %s: one shape [B, ...] is expected' % (tuple(x.shape), tuple(target.shape)))
    B = int(x.shape[0])
    n = int(x.numel() // B) if B else 0
    if B < 1 or n < 1:
        raise ValueError('x has shape %s: an empty batch has no loss' % (tuple(x.shape),))
    if B > _lib.AAE_LOSS_MAX_BATCH or n > _lib.AAE_LOSS_MAX_N:
        raise ValueError('B = %d, n = %d: over the limits of %d images and %d elements per image' % (B, n, _lib.AAE_LOSS_MAX_BATCH, _lib.AAE_LOSS_MAX_N))
    ratio = check_bootstrap_ratio(bootstrap_ratio, n)
    if out is not None:
        out_loss, per_image, dx = out
        _out(out_loss, 'out[0] (loss)', (1,), dev)
        _out(per_image, 'out[1] (per_image)', (B,), dev)
        if dx is not None:
            _out(dx, 'out[2] (dx)', x.shape, dev)
    else:
        out_loss = torch.empty((1,), dtype=torch.float32, device=dev)
        per_image = torch.empty((B,), dtype=torch.float32, device=dev)
        dx = torch.empty_like(x) if grad else None
    lib = _lib.load()
    need = int(lib.aae_recon_loss_workspace_bytes(B, n))
    if workspace is None:
        workspace = torch.empty((need,), dtype=torch.uint8, device=dev)
    elif not isinstance(workspace, torch.Tensor) or workspace.dtype != torch.uint8 or workspace.device != dev or not workspace.is_contiguous():
        raise ValueError('workspace must be a contiguous uint8 tensor on %s' % dev)
    desc = _lib.ReconLossDesc(B, n, kind, ratio)
    with torch.cuda.device(dev):
        rc = lib.aae_recon_loss(ctypes.byref(desc), _ptr(x), _ptr(target), _ptr(out_loss), _ptr(per_image), _ptr(dx), _ptr(workspace),
                                int(workspace.numel()), _stream(torch, dev))
    _lib.check(lib, rc, 'aae_recon_loss')       # `workspace` is freed into the stream it was used on: the allocator orders its reuse
    return out_loss, per_image, dx


def latent_reg_loss(z, grad=False, out=None):
    """z: contiguous float32 device tensor [B, J].  Returns (loss [1], dz or None) on the device: loss = mean_b | ||z_b|| - 1 |,
    dz its gradient (0 for a zero row).  out=(loss, dz): the caller's tensors.  One launch on the current stream."""
    import torch
    _device_f32(z, 'z')
    if z.dim() != 2 or z.shape[0] < 1 or z.shape[1] < 1:
        raise ValueError('z has shape %s, [B, J] is expected' % (tuple(z.shape),))
    B, J = int(z.shape[0]), int(z.shape[1])
    if B > _lib.AAE_LOSS_MAX_BATCH or J > _lib.AAE_LOSS_MAX_LATENT:
        raise ValueError('B = %d, J = %d: over the limits of %d rows and %d columns' % (B, J, _lib.AAE_LOSS_MAX_BATCH, _lib.AAE_LOSS_MAX_LATENT))
    dev = z.device
    if out is not None:
        out_loss, dz = out
        _out(out_loss, 'out[0] (loss)', (1,), dev)
        if dz is not None:
            _out(dz, 'out[1] (dz)', z.shape, dev)
    else:
        out_loss = torch.empty((1,), dtype=torch.float32, device=dev)
        dz = torch.empty_like(z) if grad else None
    lib = _lib.load()
    with torch.cuda.device(dev):
        rc = lib.aae_latent_reg_loss(_ptr(z), B, J, _ptr(out_loss), _ptr(dz), _stream(torch, dev))
    _lib.check(lib, rc, 'aae_latent_reg_loss')
    return out_loss, dz
