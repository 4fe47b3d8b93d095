"""The ``[Augmentation] CODE`` chain of a train cfg without imgaug: a reader of the chain's text (``parse_code``), the random
draws of a batch (``draw_programs``) and the op programs the HIP kernel runs (``ProgramBuilder``; csrc/kernels/augment_core.h
states the arithmetic, DESIGN section 4 the imgaug 0.4.0 semantics it assumes).

The reference eval()s CODE with imgaug's augmenters in scope (dataset.py:380-390) and calls ``augment_images`` on every batch.
Here the text is parsed with ``ast`` and nothing is executed; the seven augmenters of the template are restated, everything
else is refused by name.  The draws follow imgaug's parameter distributions but **not** its random stream: a seed gives other
numbers here than under imgaug.
"""
from __future__ import annotations

import ast
import ctypes

import numpy as np

from . import _lib

AUGMENTERS = ('Affine', 'CoarseDropout', 'GaussianBlur', 'Add', 'Invert', 'Multiply', 'ContrastNormalization')
# augmenter -> (name of the first positional parameter, keywords understood)
_SIGNATURES = {
    'Affine': (None, ('scale',)),
    'CoarseDropout': ('p', ('p', 'size_percent', 'per_channel')),
    'GaussianBlur': ('sigma', ('sigma',)),
    'Add': ('value', ('value', 'per_channel')),
    'Invert': ('p', ('p', 'per_channel')),
    'Multiply': ('mul', ('mul', 'per_channel')),
    'ContrastNormalization': ('alpha', ('alpha', 'per_channel')),
}
_DEFAULTS = {'Affine': {'scale': 1.0}, 'CoarseDropout': {'p': 0.0}, 'GaussianBlur': {'sigma': 0.0}, 'Add': {'value': 0}, 'Invert': {'p': 0.0},
             'Multiply': {'mul': 1.0}, 'ContrastNormalization': {'alpha': 1.0}}

OP_DTYPE = np.dtype([('code', '<i4'), ('i', '<i4', (4,)), ('f', '<f4', (3,))])
assert OP_DTYPE.itemsize == ctypes.sizeof(_lib.AugmentOp) == 32
MAX_OPS = _lib.AAE_AUGMENT_MAX_OPS
MAX_BLUR_K = _lib.AAE_AUGMENT_MAX_BLUR_K
MAX_IMAGE_BYTES = 80 * 1024           # aae_augment_max_image_bytes(): two image buffers in the workgroup's 160 KiB of LDS


# ---- the CODE grammar -------------------------------------------------------------------------------------------------------
def _is_np_random_rand(node):
    f = node.func
    return (isinstance(f, ast.Attribute) and f.attr == 'rand' and isinstance(f.value, ast.Attribute) and f.value.attr == 'random'
            and isinstance(f.value.value, ast.Name) and f.value.value.id in ('np', 'numpy'))


def _value(node, what):
    """a number, a bool, a tuple of numbers, or + - * / arithmetic on numbers that may call np.random.rand() (drawn here, once,
    as the reference's eval() of the cfg text draws it)"""
    if isinstance(node, ast.Constant) and isinstance(node.value, (bool, int, float)):
        return node.value
    if isinstance(node, ast.Tuple):
        vals = tuple(_value(e, what) for e in node.elts)
        if len(vals) != 2 or any(isinstance(v, (bool, tuple)) for v in vals):
            raise ValueError('%s: a range is a tuple of two numbers' % what)
        return vals
    if isinstance(node, ast.UnaryOp) and isinstance(node.op, (ast.USub, ast.UAdd)):
        v = _value(node.operand, what)
        if isinstance(v, (bool, tuple)):
            raise ValueError('%s: sign of a non-number' % what)
        return -v if isinstance(node.op, ast.USub) else v
    if isinstance(node, ast.BinOp) and isinstance(node.op, (ast.Add, ast.Sub, ast.Mult, ast.Div)):
        a, b = _value(node.left, what), _value(node.right, what)
        if isinstance(a, (bool, tuple)) or isinstance(b, (bool, tuple)):
            raise ValueError('%s: arithmetic on a non-number' % what)
        if isinstance(node.op, ast.Div):
            return a / b
        return {ast.Add: a + b, ast.Sub: a - b, ast.Mult: a * b}[type(node.op)]
    if isinstance(node, ast.Call) and _is_np_random_rand(node) and not node.args and not node.keywords:
        return float(np.random.rand())
    raise ValueError('%s: only numbers, bools, two-number tuples, + - * / and np.random.rand() are allowed, found %s' % (what, ast.dump(node)[:60]))


def _call_name(node):
    if not isinstance(node, ast.Call):
        raise ValueError('[Augmentation] CODE: expected an augmenter call, found %s' % type(node).__name__)
    if isinstance(node.func, ast.Name):
        return node.func.id
    if isinstance(node.func, ast.Attribute):                           # iaa.Affine(...)
        return node.func.attr
    raise ValueError('[Augmentation] CODE: expected an augmenter name')


def _augmenter(node, sometimes):
    name = _call_name(node)
    if name not in _SIGNATURES:
        raise NotImplementedError('[Augmentation] CODE: augmenter %s is not implemented (implemented: %s)' % (name, ', '.join(AUGMENTERS)))
    first, keywords = _SIGNATURES[name]
    args = dict(_DEFAULTS[name])
    positional = [first] + (['per_channel'] if 'per_channel' in keywords and name != 'CoarseDropout' else [])
    if len(node.args) > len(positional) or (node.args and first is None):
        raise NotImplementedError('[Augmentation] CODE: %s with %d positional arguments' % (name, len(node.args)))
    for key, a in zip(positional, node.args):
        args[key] = _value(a, name)
    for kw in node.keywords:
        if kw.arg not in keywords:
            raise NotImplementedError('[Augmentation] CODE: %s(%s=...) is not implemented' % (name, kw.arg))
        args[kw.arg] = _value(kw.value, '%s(%s=)' % (name, kw.arg))
    pc = args.pop('per_channel', False)
    if isinstance(pc, tuple) or not 0.0 <= float(pc) <= 1.0:
        raise ValueError('[Augmentation] CODE: %s per_channel must be a bool or a probability, got %r' % (name, pc))
    if name == 'CoarseDropout' and 'size_percent' not in args:
        raise NotImplementedError('[Augmentation] CODE: CoarseDropout needs size_percent (size_px is not implemented)')
    for key, v in args.items():
        if isinstance(v, bool):
            raise ValueError('[Augmentation] CODE: %s(%s=%r): a number or a range is expected' % (name, key, v))
    return {'name': name, 'sometimes': sometimes, 'per_channel': float(pc), 'args': args}


def parse_code(text):
    """The plan of ``Sequential([...], random_order=False)``: a list of {'name', 'sometimes' (probability or None), 'per_channel'
    (probability; 0.0 / 1.0 for a bool), 'args' (numbers or (low, high) ranges)} in chain order.  ``np.random.rand()`` inside a
    parameter is drawn once, here.  NotImplementedError names what the kernel has no op for: random_order=True, another
    augmenter, another keyword."""
    tree = ast.parse(text.strip(), mode='eval').body
    if _call_name(tree) != 'Sequential':
        raise NotImplementedError('[Augmentation] CODE: the chain must be Sequential([...]), found %s' % _call_name(tree))
    if len(tree.args) != 1 or not isinstance(tree.args[0], (ast.List, ast.Tuple)):
        raise ValueError('[Augmentation] CODE: Sequential takes one list of augmenters')
    for kw in tree.keywords:
        if kw.arg != 'random_order':
            raise NotImplementedError('[Augmentation] CODE: Sequential(%s=...) is not implemented' % kw.arg)
        if _value(kw.value, 'random_order') is not False:
            raise NotImplementedError('[Augmentation] CODE: random_order=True is not implemented')
    plan = []
    for node in tree.args[0].elts:
        if _call_name(node) == 'Sometimes':
            if len(node.args) != 2 or node.keywords:
                raise NotImplementedError('[Augmentation] CODE: Sometimes(p, augmenter) is the only form implemented')
            p = _value(node.args[0], 'Sometimes')
            if isinstance(p, (bool, tuple)) or not 0.0 <= p <= 1.0:
                raise ValueError('[Augmentation] CODE: Sometimes(p): p must be a probability, got %r' % (p,))
            plan.append(_augmenter(node.args[1], float(p)))
        else:
            plan.append(_augmenter(node, None))
    if len(plan) > MAX_OPS:
        raise NotImplementedError('[Augmentation] CODE: %d augmenters, at most %d are supported' % (len(plan), MAX_OPS))
    return plan


# ---- host-side parameters of the ops ----------------------------------------------------------------------------------------
def blur_kernel_size(sigma):
    """imgaug 0.4.0 blur_gaussian_ (cv2 backend): 3.3 sigma below 3, 2.9 sigma below 5, else 2.6 sigma; at least 5; made odd."""
    k = 3.3 * sigma if sigma < 3.0 else (2.9 * sigma if sigma < 5.0 else 2.6 * sigma)
    k = int(max(k, 5))
    return k + 1 if k % 2 == 0 else k


def gaussian_weights(k, sigma):
    """cv2.getGaussianKernel(k, sigma) for sigma > 0: exp(-(i - (k-1)/2)^2 / (2 sigma^2)) normalised in float64, handed over as fp32"""
    x = np.arange(k, dtype=np.float64) - (k - 1) / 2.0
    w = np.exp(-(x * x) / (2.0 * float(sigma) ** 2))
    return (w / w.sum()).astype(np.float32)


def nearest_table(dst, src):
    """destination index -> source index of cv2.resize(INTER_NEAREST), the rule Dataset.extract_square_patch restates"""
    return np.minimum(np.floor(np.arange(dst) * (1.0 / (float(dst) / src))).astype(np.int64), src - 1)


def dropout_grid(H, W, size_percent):
    return max(1, int(H * size_percent)), max(1, int(W * size_percent))


class ProgramBuilder(object):
    """The op programs of one batch as the arrays aae_augment_batch takes (n_ops int32 [B], ops OP_DTYPE [B,16], aux uint32
    words) and, per image, the same ops as (name, values) tuples for a host restatement (``programs``)."""

    def __init__(self, batch_size, shape):
        self.B = int(batch_size)
        self.H, self.W, self.C = [int(v) for v in shape]
        if not 1 <= self.C <= 3:
            raise NotImplementedError('C = %d: the augmentation kernel handles 1 to 3 channels' % self.C)
        self.n_ops = np.zeros(self.B, dtype=np.int32)
        self.ops = np.zeros((self.B, MAX_OPS), dtype=OP_DTYPE)
        self.programs = [[] for _ in range(self.B)]
        self._aux = []
        self._aux_words = 0
        self._tables = {}

    def _push(self, words):
        words = np.ascontiguousarray(words).view(np.uint32).reshape(-1)
        at = self._aux_words
        self._aux.append(words)
        self._aux_words += len(words)
        return at

    def _op(self, b, code, i=(), f=()):
        k = int(self.n_ops[b])
        if k >= MAX_OPS:
            raise ValueError('image %d: more than %d ops' % (b, MAX_OPS))
        rec = self.ops[b, k]
        rec['code'] = code
        rec['i'][:len(i)] = i
        rec['f'][:len(f)] = f
        self.n_ops[b] = k + 1

    def _three(self, values, dtype):
        v = np.asarray(values, dtype=dtype).reshape(-1)
        if len(v) == 1:
            v = np.repeat(v, 3)
        if len(v) < 3:
            v = np.concatenate([v, np.repeat(v[-1:], 3 - len(v))])
        return v[:3]

    def affine(self, b, inv_s):
        inv_s = np.float32(inv_s)
        if not np.isfinite(inv_s) or inv_s <= 0:
            raise ValueError('Affine: scale must be positive and finite')
        self._op(b, _lib.AAE_AUGMENT_AFFINE, f=(inv_s,))
        self.programs[b].append(('affine', float(inv_s)))

    def dropout(self, b, dropped):
        """dropped: bool [planes, h_s, w_s], planes = 1 (one mask for all channels) or C"""
        dropped = np.asarray(dropped, dtype=bool)
        planes, h_s, w_s = dropped.shape
        if planes not in (1, self.C) or not (1 <= h_s <= self.H and 1 <= w_s <= self.W):
            raise ValueError('CoarseDropout: mask of shape %s for an image of %dx%dx%d' % (dropped.shape, self.H, self.W, self.C))
        key = (h_s, w_s)
        if key not in self._tables:
            rows, cols = nearest_table(self.H, h_s), nearest_table(self.W, w_s)
            self._tables[key] = (self._push((rows * w_s).astype(np.int32)), self._push(cols.astype(np.int32)), rows, cols)
        r0, c0, rows, cols = self._tables[key]
        bits = np.packbits(dropped.reshape(-1), bitorder='little')
        bits = np.concatenate([bits, np.zeros(-len(bits) % 4, dtype=np.uint8)])
        m0 = self._push(bits)
        self._op(b, _lib.AAE_AUGMENT_DROPOUT, i=(m0, r0, c0, h_s * w_s if planes > 1 else 0))
        self.programs[b].append(('dropout', dropped.copy(), rows, cols))

    def blur(self, b, sigma):
        sigma = float(sigma)
        if sigma < 1e-3:                                            # imgaug: sigma below its eps leaves the image alone
            return
        k = blur_kernel_size(sigma)
        if k > MAX_BLUR_K:
            raise NotImplementedError('GaussianBlur(sigma=%g): kernel size %d, at most %d is supported' % (sigma, k, MAX_BLUR_K))
        if k // 2 >= min(self.H, self.W):
            raise ValueError('GaussianBlur: kernel size %d on an image of %dx%d' % (k, self.H, self.W))
        w = gaussian_weights(k, sigma)
        self._op(b, _lib.AAE_AUGMENT_BLUR, i=(k, self._push(w)))
        self.programs[b].append(('blur', k, w))

    def add(self, b, values):
        v = self._three(values, np.int64)
        if np.abs(v).max() > 255:
            raise ValueError('Add: |value| > 255')
        self._op(b, _lib.AAE_AUGMENT_ADD, f=v.astype(np.float32))
        self.programs[b].append(('add', v.astype(np.float64)))

    def invert(self, b, flags):
        v = self._three(flags, bool)
        self._op(b, _lib.AAE_AUGMENT_INVERT, i=v.astype(np.int32))
        self.programs[b].append(('invert', v))

    def multiply(self, b, factors):
        v = self._three(factors, np.float32)
        if not np.isfinite(v).all():
            raise ValueError('Multiply: factors must be finite')
        self._op(b, _lib.AAE_AUGMENT_MULTIPLY, f=v)
        self.programs[b].append(('multiply', v.astype(np.float64)))

    def contrast(self, b, alphas):
        v = self._three(alphas, np.float32)
        if not np.isfinite(v).all():
            raise ValueError('ContrastNormalization: alphas must be finite')
        self._op(b, _lib.AAE_AUGMENT_CONTRAST, f=v)
        self.programs[b].append(('contrast', v.astype(np.float64)))

    @property
    def aux(self):
        return np.concatenate(self._aux) if self._aux else np.zeros(0, dtype=np.uint32)


# ---- the draws ----------------------------------------------------------------------------------------------------------------
def _uniform(v, size=None):
    if isinstance(v, tuple):
        return np.random.uniform(v[0], v[1], size=size)
    return float(v) if size is None else np.full(size, float(v))


def draw_programs(plan, batch_size, shape=(128, 128, 3)):
    """The programs of one batch, drawn from ``np.random`` in this fixed order: image by image, and per image augmenter by
    augmenter in chain order:
      1. the ``Sometimes`` coin, ``np.random.rand() < p``; when it falls false nothing else is drawn for this augmenter;
      2. the ``per_channel`` coin, ``np.random.rand() < per_channel``, only when 0 < per_channel < 1 (one per image);
      3. the parameters, n = C values when per channel, else one shared by all channels; a constant draws nothing:
         Affine ``uniform(scale)``; CoarseDropout ``uniform(p)``, ``uniform(size_percent)``, then ``rand(planes, h_s, w_s) < p``
         (a cell is kept with probability 1 - p); GaussianBlur ``uniform(sigma)``; Add ``randint(low, high + 1, n)``; Invert
         ``rand(n) < p``; Multiply and ContrastNormalization ``uniform(range, n)``.
    The distributions are imgaug 0.4.0's; its random stream is not reproduced.  Returns a ProgramBuilder."""
    H, W, C = [int(v) for v in shape]
    out = ProgramBuilder(batch_size, (H, W, C))
    for b in range(int(batch_size)):
        for aug in plan:
            if aug['sometimes'] is not None and not np.random.rand() < aug['sometimes']:
                continue
            pc = aug['per_channel']
            per_channel = pc >= 1.0 or (pc > 0.0 and np.random.rand() < pc)
            n = C if per_channel else 1
            name, args = aug['name'], aug['args']
            if name == 'Affine':
                out.affine(b, 1.0 / _uniform(args['scale']))
            elif name == 'CoarseDropout':
                p = _uniform(args['p'])
                h_s, w_s = dropout_grid(H, W, _uniform(args['size_percent']))
                out.dropout(b, np.random.rand(n, h_s, w_s) < p)
            elif name == 'GaussianBlur':
                out.blur(b, _uniform(args['sigma']))
            elif name == 'Add':
                v = args['value']
                out.add(b, np.random.randint(int(v[0]), int(v[1]) + 1, size=n) if isinstance(v, tuple) else np.full(n, int(v)))
            elif name == 'Invert':
                out.invert(b, np.random.rand(n) < float(args['p']))
            elif name == 'Multiply':
                out.multiply(b, _uniform(args['mul'], n))
            elif name == 'ContrastNormalization':
                out.contrast(b, _uniform(args['alpha'], n))
    return out


# ---- the launch -----------------------------------------------------------------------------------------------------------------
def check_image_bytes(shape):
    H, W, C = [int(v) for v in shape]
    if H * W * C > MAX_IMAGE_BYTES:
        raise ValueError('an image of %dx%dx%d = %d bytes is over the limit of %d bytes (two image buffers in the workgroup\'s LDS)'
                         % (H, W, C, H * W * C, MAX_IMAGE_BYTES))


def run_batch(train_x, mask_x, train_y, bg, train_idx, bg_idx, programs, want_u8=True, want_x=True, want_y=True, out=None, timed=0):
    """aae_augment_batch on device tensors: train_x / train_y uint8 [N,H,W,C], mask_x bool or uint8 [N,H,W], bg uint8 [M,H,W,C];
    train_idx / bg_idx host integer arrays [B]; programs a ProgramBuilder.  Returns (batch_x uint8, batch_x float32, batch_y
    float32) device tensors, None where not wanted; out: the three tensors to write into instead (None for a null pointer).  One
    launch on the current stream.  timed = n > 0 repeats the launch n more times between two events and also returns the
    milliseconds of one launch (synchronises)."""
    import torch
    lib = _lib.load()
    dev = train_x.device
    N, H, W, C = [int(v) for v in train_x.shape]
    M, B = int(bg.shape[0]), programs.B
    train_idx = np.ascontiguousarray(train_idx, dtype=np.int32).reshape(-1)
    bg_idx = np.ascontiguousarray(bg_idx, dtype=np.int32).reshape(-1)
    if len(train_idx) != B or len(bg_idx) != B:
        raise ValueError('%d training indices, %d background indices, programs of %d images' % (len(train_idx), len(bg_idx), B))
    if tuple(train_y.shape) != (N, H, W, C) or tuple(mask_x.shape) != (N, H, W) or tuple(bg.shape[1:]) != (H, W, C) or (H, W, C) != (programs.H, programs.W, programs.C):
        raise ValueError('train_x %s, mask_x %s, train_y %s, bg %s, programs for %s' % (tuple(train_x.shape), tuple(mask_x.shape), tuple(train_y.shape),
                                                                                       tuple(bg.shape), (programs.H, programs.W, programs.C)))
    if (train_idx < 0).any() or (train_idx >= N).any() or (bg_idx < 0).any() or (bg_idx >= M).any():
        raise ValueError('a training or background index is out of range')
    for t in (train_x, mask_x, train_y, bg):
        if not t.is_cuda or not t.is_contiguous() or t.element_size() != 1:
            raise ValueError('train_x, mask_x, train_y and bg must be contiguous one-byte device tensors')
    aux = programs.aux
    # one upload: indices, op counts, ops and aux words in a single int32 buffer
    head = np.concatenate([train_idx, bg_idx, programs.n_ops, programs.ops.reshape(-1).view(np.int32), aux.view(np.int32)])
    plan = torch.from_numpy(head).to(dev, non_blocking=False)
    base = plan.data_ptr()
    ops_at, aux_at = base + 12 * B, base + 12 * B + 32 * MAX_OPS * B
    if out is not None:
        out_u8, out_x, out_y = out
        for t, dt in ((out_u8, torch.uint8), (out_x, torch.float32), (out_y, torch.float32)):
            if t is not None and (t.dtype != dt or tuple(t.shape) != (B, H, W, C) or not t.is_contiguous() or t.device != dev):
                raise ValueError('out: contiguous %s tensors of %s on %s are expected' % (dt, (B, H, W, C), dev))
    else:
        out_u8 = torch.empty((B, H, W, C), dtype=torch.uint8, device=dev) if want_u8 else None
        out_x = torch.empty((B, H, W, C), dtype=torch.float32, device=dev) if want_x else None
        out_y = torch.empty((B, H, W, C), dtype=torch.float32, device=dev) if want_y else None
    ptr = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    s = _lib.AugmentShape(N, M, H, W, C, B, len(aux))
    with torch.cuda.device(dev):
        stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        launch = lambda: lib.aae_augment_batch(ctypes.byref(s), ptr(train_x), ptr(mask_x), ptr(train_y), ptr(bg), ctypes.c_void_p(base),
                                               ctypes.c_void_p(base + 4 * B), ctypes.c_void_p(base + 8 * B), ctypes.c_void_p(ops_at),
                                               ctypes.c_void_p(aux_at) if len(aux) else None, ptr(out_u8), ptr(out_x), ptr(out_y), stream)
        _lib.check(lib, launch(), 'aae_augment_batch')      # `plan` is freed into the stream it was used on: the allocator orders its reuse
        if timed > 0:
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(int(timed)):
                _lib.check(lib, launch(), 'aae_augment_batch')
            t1.record()
            t1.synchronize()
            return out_u8, out_x, out_y, t0.elapsed_time(t1) / int(timed)
    return out_u8, out_x, out_y
