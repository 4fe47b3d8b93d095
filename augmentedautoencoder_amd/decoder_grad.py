"""The decoder's backward pass on device tensors (aae_upconv_backward / aae_dense_backward in include/aae_hip.h):
the gradient of a stage's kernel and bias and dL/d(input) from dL/d(output) and the two activations the forward left behind.  Device
tensors in, device tensors out: no host copy, no synchronisation, no floating-point atomic (the same inputs give the same bits).
A stage whose resize is neither exactly 2x nor 1x is refused with NotImplementedError before anything is launched."""
from __future__ import annotations

import ctypes

from . import _lib
from .loss import _device_f32, _out, _ptr, _stream

ACTIVATIONS = {'relu': 0, 'sigmoid': 1}


def check_resize(H, W, UH, UW):
    """the stages the backward pass is built for: exact 2x (phase-folded) and 1x (the one-phase case)"""
    if (UH, UW) != (2 * H, 2 * W) and (UH, UW) != (H, W):
        raise NotImplementedError('the backward pass of a %dx%d -> %dx%d resize is not built: only exact 2x and 1x stages train '
                                  '(the forward runs this stage through its direct kernel)' % (H, W, UH, UW))


def check_trainable(cfg):
    """NotImplementedError for a DecoderConfig the backward pass is not built for: batch norm, the mask head, a resize other than 2x / 1x"""
    if cfg.batch_norm:
        raise NotImplementedError('batch_norm: the backward pass needs the training-mode batch statistics of batch normalisation, which are not built')
    if cfg.auxiliary_mask:
        raise NotImplementedError('auxiliary_mask: the decoder engine does not compute the mask head, so it has no gradient')
    dims = cfg.layer_dimensions() + [list(cfg.shape[:2])]
    for (h, w), (uh, uw) in zip(dims[:-1], dims[1:]):
        check_resize(h, w, uh, uw)


def _workspace(torch, workspace, need, dev):
    if workspace is None:
        return torch.empty((need,), dtype=torch.uint8, device=dev)
    if not isinstance(workspace, torch.Tensor) or workspace.dtype != torch.uint8 or workspace.device != dev or not workspace.is_contiguous():
        raise ValueError('workspace must be a contiguous uint8 tensor on %s' % dev)
    return workspace


def labels():
    """what the calling thread's last backward call launched, in order: '<stage>:<form> ... M= N= K= ... splits='"""
    lib = _lib.load()
    return [lib.aae_decoder_bwd_label(i).decode() for i in range(lib.aae_decoder_bwd_label_count())]


def upconv_backward(a_in, a_out, g_out, w, activation='relu', need_g_in=True, out=None, workspace=None):
    """a_in [B,H,W,Cin]: the stage's input; a_out [B,UH,UW,Cout]: its output; g_out = dL/da_out; w [KS,KS,Cin,Cout]; all contiguous
    float32 device tensors.  Returns (dw [KS,KS,Cin,Cout], db [Cout], g_in [B,H,W,Cin] or None).  out=(dw, db, g_in): the caller's
    tensors to write into (g_in None: that product is not computed); workspace: a caller's uint8 device tensor of at least
    aae_upconv_backward_workspace_bytes bytes, 256-byte aligned."""
    import torch
    if activation not in ACTIVATIONS:
        raise ValueError('unknown activation %r: one of %s' % (activation, sorted(ACTIVATIONS)))
    _device_f32(a_in, 'a_in')
    dev = a_in.device
    for t, name in ((a_out, 'a_out'), (g_out, 'g_out'), (w, 'w')):
        _device_f32(t, name, dev)
    if a_in.dim() != 4 or a_out.dim() != 4 or w.dim() != 4 or min(a_in.shape) < 1 or min(a_out.shape) < 1:
        raise ValueError('a_in has shape %s, a_out %s, w %s: [B,H,W,Cin], [B,UH,UW,Cout] and [KS,KS,Cin,Cout] are expected' % (tuple(a_in.shape), tuple(a_out.shape), tuple(w.shape)))
    B, H, W, Cin = (int(v) for v in a_in.shape)
    UH, UW, Cout = (int(v) for v in a_out.shape[1:])
    KS = int(w.shape[0])
    if int(a_out.shape[0]) != B or tuple(g_out.shape) != tuple(a_out.shape):
        raise ValueError('a_out has shape %s, g_out %s, the batch is %d: one shape [B,UH,UW,Cout] is expected' % (tuple(a_out.shape), tuple(g_out.shape), B))
    if tuple(w.shape) != (KS, KS, Cin, Cout) or KS % 2 == 0:
        raise ValueError('w has shape %s: [KS,KS,%d,%d] with an odd KS is expected' % (tuple(w.shape), Cin, Cout))
    check_resize(H, W, UH, UW)
    if out is not None:
        dw, db, g_in = out
        _out(dw, 'out[0] (dw)', w.shape, dev)
        _out(db, 'out[1] (db)', (Cout,), dev)
        if g_in is not None:
            _out(g_in, 'out[2] (g_in)', a_in.shape, dev)
    else:
        dw = torch.empty_like(w)
        db = torch.empty((Cout,), dtype=torch.float32, device=dev)
        g_in = torch.empty_like(a_in) if need_g_in else None
    lib = _lib.load()
    desc = _lib.UpconvBackwardDesc(B, H, W, Cin, UH, UW, Cout, KS, ACTIVATIONS[activation])
    need = int(lib.aae_upconv_backward_workspace_bytes(ctypes.byref(desc), int(g_in is not None)))
    if need == 0:
        _lib.check(lib, -2, 'aae_upconv_backward_workspace_bytes')
    workspace = _workspace(torch, workspace, need, dev)
    with torch.cuda.device(dev):
        rc = lib.aae_upconv_backward(ctypes.byref(desc), _ptr(a_in), _ptr(a_out), _ptr(g_out), _ptr(w), _ptr(dw), _ptr(db), _ptr(g_in), _ptr(workspace),
                                     int(workspace.numel()), _stream(torch, dev))
    _lib.check(lib, rc, 'aae_upconv_backward')
    return dw, db, g_in


def dense_backward(z, a_out, g_out, w, need_dz=True, out=None, workspace=None):
    """The dense layer a_out = relu(z w + b): z [B,J], a_out / g_out [B,U] (or [B,h,w,C] with h w C = U), w [J,U].  Returns
    (dw [J,U], db [U], dz [B,J] or None); out=(dw, db, dz) and workspace as in upconv_backward."""
    import torch
    _device_f32(z, 'z')
    dev = z.device
    for t, name in ((a_out, 'a_out'), (g_out, 'g_out'), (w, 'w')):
        _device_f32(t, name, dev)
    if z.dim() != 2 or w.dim() != 2 or min(z.shape) < 1 or min(w.shape) < 1 or int(w.shape[0]) != int(z.shape[1]):
        raise ValueError('z has shape %s, w %s: [B,J] and [J,U] are expected' % (tuple(z.shape), tuple(w.shape)))
    B, J, U = int(z.shape[0]), int(z.shape[1]), int(w.shape[1])
    if tuple(a_out.shape) != tuple(g_out.shape) or a_out.dim() < 2 or int(a_out.shape[0]) != B or a_out.numel() != B * U:
        raise ValueError('a_out has shape %s, g_out %s: [%d, ...] with %d elements per row is expected' % (tuple(a_out.shape), tuple(g_out.shape), B, U))
    if out is not None:
        dw, db, dz = out
        _out(dw, 'out[0] (dw)', w.shape, dev)
        _out(db, 'out[1] (db)', (U,), dev)
        if dz is not None:
            _out(dz, 'out[2] (dz)', z.shape, dev)
    else:
        dw = torch.empty_like(w)
        db = torch.empty((U,), dtype=torch.float32, device=dev)
        dz = torch.empty_like(z) if need_dz else None
    lib = _lib.load()
    desc = _lib.DenseBackwardDesc(B, J, U)
    need = int(lib.aae_dense_backward_workspace_bytes(ctypes.byref(desc), int(dz is not None)))
    if need == 0:
        _lib.check(lib, -2, 'aae_dense_backward_workspace_bytes')
    workspace = _workspace(torch, workspace, need, dev)
    with torch.cuda.device(dev):
        rc = lib.aae_dense_backward(ctypes.byref(desc), _ptr(z), _ptr(a_out), _ptr(g_out), _ptr(w), _ptr(dw), _ptr(db), _ptr(dz), _ptr(workspace),
                                    int(workspace.numel()), _stream(torch, dev))
    _lib.check(lib, rc, 'aae_dense_backward')
    return dw, db, dz
