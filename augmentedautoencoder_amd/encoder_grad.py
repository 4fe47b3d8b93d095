"""The encoder's backward pass on device tensors (aae_conv_backward / aae_linear_backward in include/aae_hip.h):
the gradient of a layer's kernel and bias and dL/d(input) from dL/d(output) and the two activations the forward left behind.  Device
tensors in, device tensors out: no host copy, no synchronisation, no floating-point atomic (the same inputs give the same bits).
A stride of 3 or more is refused with NotImplementedError before anything is launched."""
from __future__ import annotations

import ctypes

from . import _lib
from .decoder_grad import _workspace
from .loss import _device_f32, _out, _ptr, _stream

MAX_STRIDE = 2
MAX_KERNEL_SIZE = 7


def check_stride(stride, kernel_size=1):
    """the layers the backward pass is built for: strides 1 and 2, kernels of 1 ... 7"""
    if int(stride) > MAX_STRIDE:
        raise NotImplementedError('stride %d: the backward pass is built for strides 1 and 2' % int(stride))
    if int(kernel_size) > MAX_KERNEL_SIZE:
        raise NotImplementedError('kernel size %d: the backward pass is built for KS 1 ... %d' % (int(kernel_size), MAX_KERNEL_SIZE))


def check_trainable(cfg):
    """NotImplementedError for an EncoderConfig the backward pass is not built for: batch norm, a stride of 3 or more"""
    if cfg.batch_norm:
        raise NotImplementedError('batch_norm: the backward pass needs the training-mode batch statistics of batch normalisation, which are not built')
    for s in cfg.strides:
        check_stride(s, cfg.kernel_size)


def labels():
    """what the calling thread's last encoder-backward call launched, in order: '<layer>:<form> ... M= N= K= ... splits='"""
    lib = _lib.load()
    return [lib.aae_encoder_bwd_label(i).decode() for i in range(lib.aae_encoder_bwd_label_count())]


def _layer_input(a_in, name):
    """a_in: float32, or uint8 (the first layer's crops, read as float32(v / 255.))"""
    import torch
    if isinstance(a_in, torch.Tensor) and a_in.dtype == torch.uint8:
        if not a_in.is_cuda:
            raise ValueError('%s lives on %s, a GPU tensor is expected' % (name, a_in.device))
        if not a_in.is_contiguous():
            raise ValueError('%s must be contiguous' % name)
        return _lib.AAE_DTYPE_U8
    _device_f32(a_in, name)
    return _lib.AAE_DTYPE_F32


def conv_backward(a_in, a_out, g_out, w, stride, need_g_in=True, out=None, workspace=None):
    """a_in [B,H,W,Cin]: the layer's input, float32 or uint8; a_out [B,Ho,Wo,Cout]: its output; g_out = dL/da_out; w [KS,KS,Cin,Cout];
    contiguous device tensors, float32 but for a uint8 a_in.  Returns (dw [KS,KS,Cin,Cout], db [Cout], g_in [B,H,W,Cin] or None).
    out=(dw, db, g_in): the caller's tensors to write into (g_in None: that product is not computed); workspace: a caller's uint8
    device tensor of at least aae_conv_backward_workspace_bytes bytes, 256-byte aligned."""
    import torch
    dtype = _layer_input(a_in, 'a_in')
    dev = a_in.device
    for t, name in ((a_out, 'a_out'), (g_out, 'g_out'), (w, 'w')):
        _device_f32(t, name, dev)
    if a_in.dim() != 4 or a_out.dim() != 4 or w.dim() != 4 or min(a_in.shape) < 1 or min(a_out.shape) < 1 or min(w.shape) < 1:
        raise ValueError('a_in has shape %s, a_out %s, w %s: [B,H,W,Cin], [B,Ho,Wo,Cout] and [KS,KS,Cin,Cout] are expected' % (tuple(a_in.shape), tuple(a_out.shape), tuple(w.shape)))
    if isinstance(stride, bool) or int(stride) != stride or int(stride) < 1:
        raise ValueError('stride must be an integer >= 1, got %r' % (stride,))
    S = int(stride)
    B, H, W, Cin = (int(v) for v in a_in.shape)
    Ho, Wo, Cout = (int(v) for v in a_out.shape[1:])
    KS = int(w.shape[0])
    if tuple(w.shape) != (KS, KS, Cin, Cout):
        raise ValueError('w has shape %s: [KS,KS,%d,%d] is expected' % (tuple(w.shape), Cin, Cout))
    if int(a_out.shape[0]) != B or tuple(g_out.shape) != tuple(a_out.shape) or (Ho, Wo) != (-(-H // S), -(-W // S)):
        raise ValueError('a_out has shape %s, g_out %s: [%d,%d,%d,Cout], the \'same\' output of a stride-%d layer, is expected'
                         % (tuple(a_out.shape), tuple(g_out.shape), B, -(-H // S), -(-W // S), S))
    check_stride(S, KS)
    if out is not None:
        dw, db, g_in = out
        _out(dw, 'out[0] (dw)', w.shape, dev)
        _out(db, 'out[1] (db)', (Cout,), dev)
        if g_in is not None:
            _out(g_in, 'out[2] (g_in)', a_in.shape, dev)
    else:
        dw = torch.empty_like(w)
        db = torch.empty((Cout,), dtype=torch.float32, device=dev)
        g_in = torch.empty(a_in.shape, dtype=torch.float32, device=dev) if need_g_in else None
    lib = _lib.load()
    desc = _lib.ConvBackwardDesc(B, H, W, Cin, Cout, KS, S, dtype)
    need = int(lib.aae_conv_backward_workspace_bytes(ctypes.byref(desc)))
    if need == 0:
        _lib.check(lib, -2, 'aae_conv_backward_workspace_bytes')
    workspace = _workspace(torch, workspace, need, dev)
    with torch.cuda.device(dev):
        rc = lib.aae_conv_backward(ctypes.byref(desc), _ptr(a_in), _ptr(a_out), _ptr(g_out), _ptr(w), _ptr(dw), _ptr(db), _ptr(g_in), _ptr(workspace),
                                   int(workspace.numel()), _stream(torch, dev))
    _lib.check(lib, rc, 'aae_conv_backward')
    return dw, db, g_in


def linear_backward(a, dz, w, need_g_a=True, out=None, workspace=None):
    """The dense layer z = flat(a) w + b: a [B,J] (or [B,h,w,C] with h w C = J), dz = dL/dz [B,U], w [J,U].  Returns
    (dw [J,U], db [U], g_a in the shape of a, or None); out=(dw, db, g_a) and workspace as in conv_backward."""
    import torch
    _device_f32(a, 'a')
    dev = a.device
    for t, name in ((dz, 'dz'), (w, 'w')):
        _device_f32(t, name, dev)
    if dz.dim() != 2 or w.dim() != 2 or min(dz.shape) < 1 or min(w.shape) < 1 or int(w.shape[1]) != int(dz.shape[1]):
        raise ValueError('dz has shape %s, w %s: [B,U] and [J,U] are expected' % (tuple(dz.shape), tuple(w.shape)))
    B, J, U = int(dz.shape[0]), int(w.shape[0]), int(w.shape[1])
    if a.dim() < 2 or int(a.shape[0]) != B or a.numel() != B * J:
        raise ValueError('a has shape %s: [%d, ...] with %d elements per row is expected' % (tuple(a.shape), B, J))
    if out is not None:
        dw, db, g_a = out
        _out(dw, 'out[0] (dw)', w.shape, dev)
        _out(db, 'out[1] (db)', (U,), dev)
        if g_a is not None:
            _out(g_a, 'out[2] (g_a)', a.shape, dev)
    else:
        dw = torch.empty_like(w)
        db = torch.empty((U,), dtype=torch.float32, device=dev)
        g_a = torch.empty_like(a) if need_g_a else None
    lib = _lib.load()
    desc = _lib.DenseBackwardDesc(B, J, U)
    need = int(lib.aae_linear_backward_workspace_bytes(ctypes.byref(desc), int(g_a is not None)))
    if need == 0:
        _lib.check(lib, -2, 'aae_linear_backward_workspace_bytes')
    workspace = _workspace(torch, workspace, need, dev)
    with torch.cuda.device(dev):
        rc = lib.aae_linear_backward(ctypes.byref(desc), _ptr(a), _ptr(dz), _ptr(w), _ptr(dw), _ptr(db), _ptr(g_a), _ptr(workspace), int(workspace.numel()),
                                     _stream(torch, dev))
    _lib.check(lib, rc, 'aae_linear_backward')
    return dw, db, g_a
