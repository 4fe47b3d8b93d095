"""Device plumbing between the reference-shaped Python API and libaae_hip.so.

torch is used for exactly three things here: device memory (tensors that own
the buffers handed to the C ABI as raw pointers), the current HIP stream, and
host<->device copies.  All arithmetic happens in the hand-written HIP kernels.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib
from .weights import EncoderConfig, as_pointer_array, ordered_weight_arrays


_TORCH = None


def _torch():
    """torch, once it has been seen with a GPU (the check costs ~8 us per call: asked once per process, not per launch)."""
    global _TORCH
    if _TORCH is None:
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError('augmentedautoencoder_amd needs an AMD GPU (MI355X / gfx950); '
                               'torch.cuda.is_available() is False and there is no CPU fallback.')
        _TORCH = torch
    return _TORCH


def _stream_ptr(torch):
    """raw handle of the current stream of the current device (the fast accessor where torch has it: ~0.3 us instead of ~4)"""
    raw = getattr(torch._C, '_cuda_getCurrentRawStream', None)
    if raw is not None:
        return ctypes.c_void_p(raw(torch.cuda.current_device()))
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


class _on_device(object):
    """`with torch.cuda.device(d)` without its cost when d is current already (the per-detection loop: one GPU per process)."""

    def __init__(self, device):
        self.idx = device.index if device.index is not None else 0

    def __enter__(self):
        torch = _torch()
        self.prev = torch.cuda.current_device()
        if self.prev != self.idx:
            torch.cuda.set_device(self.idx)

    def __exit__(self, *exc):
        if self.prev != self.idx:
            _torch().cuda.set_device(self.prev)
        return False


class _Workspace(object):
    """One grow-only device scratch buffer per engine.  The pointer handed out is 256-B aligned and has at least the
    requested bytes behind it; a fresh buffer starts zeroed (the ticket words of the in-launch reductions are then in
    their clean state from the first call on -- the kernels tolerate garbage, this only saves the install path).
    A buffer SHARED by several engines (share_workspaces) serves calls of ONE stream only: it remembers the stream of its
    first use and raises when asked from another one (two streams would scratch in the same memory at the same time)."""

    def __init__(self, device):
        self.device = device
        self.buf = None
        self.shared = False
        self.stream = None

    def get(self, nbytes):
        torch = _torch()
        nbytes = int(nbytes)
        if self.shared:
            cur = _stream_ptr(torch).value or 0
            if self.stream is None:
                self.stream = cur
            elif cur != self.stream and self._idle(torch, self.stream):
                self.stream = cur              # (the earlier stream has drained: the buffer moves to the new one)
            elif cur != self.stream:
                raise RuntimeError('this scratch buffer is shared by several engines (engine.share_workspaces / AePoseEstimator) and serves one '
                                   'stream; stream %#x still has work queued, the call comes from %#x.  Build the estimator with share_workspaces=False, or call '
                                   'unshare_workspaces(), to use its engines from several streams' % (self.stream, cur))
        if self.buf is None or self._usable() < nbytes:
            self.buf = None
            self.buf = torch.zeros(nbytes + 256, dtype=torch.uint8, device=self.device)
        off = (-self.buf.data_ptr()) % 256
        assert self.buf.numel() - off >= nbytes
        return self.buf, self.buf.data_ptr() + off

    def _usable(self):
        return self.buf.numel() - (-self.buf.data_ptr()) % 256

    def _idle(self, torch, stream_ptr):
        try:
            st = torch.cuda.ExternalStream(stream_ptr, device=self.device) if stream_ptr else torch.cuda.default_stream(self.device)
            return bool(st.query())
        except Exception:
            return False


def share_workspaces(engines):
    """Engines that only ever run one after the other on one stream -- the N objects of one pose estimator
    (m3_interface/ae_pose_estimator.py:61-78 keeps N encoders + N codebooks in one process) -- can scratch in the SAME device
    memory: N x 973 MB of encoder workspace at batch 256 become one (7.8 GB -> 1 GB for eight objects).  `engines`: objects with
    a `.ws` scratch buffer and a `.device`, all of one kind (encoders, or codebooks: one call uses an encoder's and a codebook's
    workspace at the same time, so the two kinds never share).  Nothing in a workspace outlives a call (the ticket words at its
    front are nonce-tagged per launch), so sharing changes no result.  Explicit and reversible: every engine remembers its own
    buffer (`_own_ws`), the shared buffer refuses calls from a second stream, and unshare_workspaces() undoes it.  Returns the
    engines whose buffer was rebound."""
    pools, rebound = {}, []
    for e in engines:
        ws = getattr(e, 'ws', None)
        if e is None or ws is None or not hasattr(e, 'device'):
            continue
        key = (type(e), str(e.device))
        if key in pools:
            if e.ws is not pools[key]:
                if not hasattr(e, '_own_ws'):
                    e._own_ws = e.ws
                e.ws = pools[key]
                pools[key].shared = True
                pools[key].users = getattr(pools[key], 'users', 0) + 1
                rebound.append(e)
        else:
            pools[key] = ws
    return rebound


def unshare_workspaces(engines):
    """undo share_workspaces for these engines: each gets the buffer it owned before; the pool owner's buffer stops being a
    shared (one-stream) buffer once the last engine that borrowed it is gone"""
    for e in engines:
        own = getattr(e, '_own_ws', None)
        if own is not None:
            pool = e.ws
            e.ws = own
            del e._own_ws
            pool.users = max(0, getattr(pool, 'users', 1) - 1)
            if pool.users == 0:                # only its owner is left: an ordinary single-engine buffer again (any stream may use it)
                pool.shared = False
                pool.stream = None


class EncoderEngine(object):
    """Owns one aae_encoder handle (device weights) -- the stand-in for the encoder
    part of the TF graph + session of the reference."""

    def __init__(self, cfg: EncoderConfig, weights, device=None, max_batch=256):
        torch = _torch()
        self.cfg = cfg
        self.device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        self.max_batch = int(max_batch)
        self.lib = _lib.load()
        arrays = ordered_weight_arrays(weights, cfg)
        handle = ctypes.c_void_p()
        desc = cfg.to_desc()
        with _on_device(self.device):
            rc = self.lib.aae_encoder_create(ctypes.byref(desc), as_pointer_array(arrays), len(arrays), ctypes.byref(handle))
        _lib.check(self.lib, rc, 'aae_encoder_create')
        self.handle = handle
        self.ws = _Workspace(self.device)
        self._last_B = None
        self.options = {}
        self._ws_bytes = {}                # batch -> aae_encoder_workspace_bytes (depends on the options: cleared by set_option)
        # f32x3h mode ('precision' = 1, 2): activations travel as fp16 (hi, lo) pairs that carry |x| < 4094 exactly.  Every
        # forward raises its own device flag when a value leaves that range; the flags of all forwards queued since the
        # last check are read in ONE host round trip by settle() -- when results are consumed, never per launch -- and
        # the affected chunks are recomputed in exact fp32, in place.
        self.x3h_fallback = True
        self.x3h_fallbacks = 0             # how many chunks were recomputed
        self._x3h_pending = []             # (flag slot, redo closure) of f32x3h forwards not yet checked
        self._host_weights = arrays        # what backward() differentiates with respect to: copied to the device on first use
        self._dev_weights = None
        self._bwd_ws = None

    def close(self):
        if getattr(self, 'handle', None):
            self.lib.aae_encoder_destroy(self.handle)
            self.handle = None
        self._dev_weights = None
        self._bwd_ws = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_option(self, name, value):
        """Launch-planning / precision knobs of aae_encoder_set_option, e.g.
        ('precision', 1) selects the f32x3h split-precision matrix-core path
        (fp32 in/out, 3 fp16 MFMAs per product, fp32 accumulate); ('precision', 2) uses it only for batches it is faster on
        (B >= 4 of the default net; per-detection batches stay on the exact fp32 wave-split-K path); default 0 = exact fp32."""
        _lib.check(self.lib, self.lib.aae_encoder_set_option(self.handle, name.encode(), int(value)), 'aae_encoder_set_option')
        self.options[name] = int(value)
        self._ws_bytes.clear()

    def workspace_bytes(self, B):
        n = self._ws_bytes.get(B)
        if n is None:
            n = self._ws_bytes[B] = self.lib.aae_encoder_workspace_bytes(self.handle, B)
        return n

    # ---- input handling: codebook.py:58-61 --------------------------------
    def to_device_batch(self, x):
        """np.ndarray / torch.Tensor, HWC or NHWC, uint8 or float -> contiguous
        device tensor [B,H,W,C] of dtype uint8 or float32.  uint8 is scaled by
        1/255 inside the first kernel (exactly float32(v/255.)); float input is
        what the reference feeds to the float32 placeholder."""
        torch = _torch()
        if isinstance(x, np.ndarray):
            if x.dtype != np.uint8:
                x = x.astype(np.float32)
            t = torch.from_numpy(np.ascontiguousarray(x)).to(self.device, non_blocking=False)
        elif torch.is_tensor(x):
            t = x
            if t.dtype != torch.uint8:
                t = t.to(torch.float32)
            t = t.to(self.device).contiguous()
        else:
            raise TypeError('crops must be a numpy array or a torch tensor, got %r' % type(x))
        if t.dim() == 3:
            t = t.unsqueeze(0)
        if t.dim() != 4 or tuple(t.shape[1:]) != tuple(self.cfg.shape):
            raise ValueError('crop batch has shape %s, encoder expects [B,%d,%d,%d]' % ((tuple(t.shape),) + tuple(self.cfg.shape)))
        return t

    def _x3h_note(self, redo):
        """Called right after a forward / encode_nn C call: if it ran in f32x3h, remember its range-flag slot and how to
        redo it in exact fp32.  No synchronisation here; settle() looks at the flags."""
        if self.options.get('precision', 0) not in (1, 2):
            return
        slot = self.lib.aae_encoder_x3h_last_slot()
        if slot < 0:
            return
        torch = _torch()
        if torch.cuda.is_current_stream_capturing():
            self._x3h_captured_slot = slot        # a graph owns this slot until it is released (CapturedNearestNeighbour polls it after each replay)
            return
        if not self.x3h_fallback:
            return
        self._x3h_pending.append((slot, redo))
        if len(self._x3h_pending) >= 192:         # the ring has 256 slots: never let un-checked forwards share one
            self.settle()

    def _x3h_poll(self, slots):
        torch = _torch()
        arr = (ctypes.c_int * len(slots))(*slots)
        flags = (ctypes.c_int * len(slots))()
        with _on_device(self.device):
            _lib.check(self.lib, self.lib.aae_encoder_x3h_poll(self.handle, arr, len(slots), flags, _stream_ptr(torch)),
                       'aae_encoder_x3h_poll')
        return [int(f) for f in flags]

    def settle(self):
        """Check the range flags of every f32x3h forward queued since the last settle() (ONE wait for the stream) and
        recompute the affected chunks in exact fp32 -- in place, into the tensors the earlier calls returned.  Returns
        how many chunks were recomputed.  The reference-shaped API (codebook.py) calls this where it copies results to
        the host; engine-level users in split-precision mode call it before they trust z / idx / score (results that
        were DERIVED from a recomputed z by another call, e.g. CodebookEngine.nn, have to be derived again)."""
        pending, self._x3h_pending = self._x3h_pending, []
        if not pending:
            return 0
        flags = self._x3h_poll([slot for slot, _ in pending])
        redone = 0
        mode = self.options.get('precision', 0)
        for (slot, redo), flag in zip(pending, flags):
            if not flag:
                continue
            redone += 1
            self.x3h_fallbacks += 1
            if self.x3h_fallbacks == 1:
                import warnings
                warnings.warn('f32x3h: an activation exceeded the range of its fp16 (hi, lo) pair (|x| >= 4094 at the default '
                              'x3h_act_shift); the batch is recomputed in exact fp32 (further occurrences are counted in '
                              'EncoderEngine.x3h_fallbacks)', RuntimeWarning)
            self.set_option('precision', 0)
            try:
                redo()
            finally:
                self.set_option('precision', mode)
        return redone

    def _forward_chunk(self, t, z_out, timed=False):
        torch = _torch()
        B = t.shape[0]
        dt = _lib.AAE_DTYPE_U8 if t.dtype == torch.uint8 else _lib.AAE_DTYPE_F32
        nbytes = self.workspace_bytes(B)
        _, ws_ptr = self.ws.get(nbytes)
        self._last_B = B
        with _on_device(self.device):
            if not timed:
                rc = self.lib.aae_encoder_forward(self.handle, ctypes.c_void_p(t.data_ptr()), dt, B,
                                                  ctypes.c_void_p(z_out.data_ptr()), ctypes.c_void_p(ws_ptr), nbytes,
                                                  _stream_ptr(torch))
                _lib.check(self.lib, rc, 'aae_encoder_forward')
                self._x3h_note(lambda: self._forward_chunk(t, z_out))     # documented failure mode of the split-precision mode: redo in fp32
                return None
            ms = (ctypes.c_float * 32)()
            n = ctypes.c_int(0)
            rc = self.lib.aae_encoder_forward_timed(self.handle, ctypes.c_void_p(t.data_ptr()), dt, B,
                                                    ctypes.c_void_p(z_out.data_ptr()), ctypes.c_void_p(ws_ptr), nbytes,
                                                    _stream_ptr(torch), ms, 32, ctypes.byref(n))
            _lib.check(self.lib, rc, 'aae_encoder_forward_timed')
            return [(self.lib.aae_encoder_kernel_label(self.handle, i).decode(), float(ms[i]),
                     float(self.lib.aae_encoder_kernel_flops(self.handle, i))) for i in range(n.value)]

    def encode(self, x):
        """Encoder.z for a batch: device float32 [B, J]."""
        torch = _torch()
        t = self.to_device_batch(x)
        B = t.shape[0]
        z = torch.empty((B, self.cfg.latent_space_size), dtype=torch.float32, device=self.device)
        for a in range(0, B, self.max_batch):
            e = min(a + self.max_batch, B)
            self._forward_chunk(t[a:e], z[a:e])
        return z

    def encode_checked(self, x):
        """encode() + settle(): latents that other device work may be derived from right away (in exact fp32, the
        default, settle() has nothing to do)."""
        z = self.encode(x)
        self.settle()
        return z

    def detect_nn(self, codebook_engine, image, rows, n, col_stride, crops, z, idx, score):
        """All `n` detections of this object in a frame in ONE C call (aae_detect_nn): crop + bilinear resize of the boxes
        `rows` (int32 [n,5] x, y, w, h, size) out of `image` (uint8 [H,W,C]) into `crops`, encoder, top-1 codebook query.
        Every argument is caller-owned storage that the per-frame loop reuses: image / rows on the device or in pinned host
        memory (device-accessible), crops [>=n,h,w,c] uint8 / z [>=n,J] / score [>=n] device tensors, idx int64 [>=n] on the
        device or pinned (a pinned tensor receives the indices without a copy back).  No checks beyond the C side's: the
        estimator's staging code is the one caller.  Chunks of max_batch."""
        torch = _torch()
        cb = codebook_engine
        H, W, C = int(image.shape[0]), int(image.shape[1]), int(image.shape[2])
        cb.ensure_upright(col_stride, 1)
        stream = _stream_ptr(torch)
        rows_ptr, crops_ptr, z_ptr, idx_ptr, score_ptr = rows.data_ptr(), crops.data_ptr(), z.data_ptr(), idx.data_ptr(), score.data_ptr()
        per_crop, J = int(crops[0].numel()), int(z.shape[1])
        for a in range(0, n, self.max_batch):
            m = min(self.max_batch, n - a)
            nb_e = self.workspace_bytes(m)
            nb_c = cb.workspace_bytes(m, 1)
            _, ws_e = self.ws.get(nb_e)
            _, ws_c = cb.ws.get(nb_c)
            self._last_B = m
            with _on_device(self.device):
                rc = self.lib.aae_detect_nn(self.handle, cb.handle, ctypes.c_void_p(image.data_ptr()), H, W, C,
                                            ctypes.c_void_p(rows_ptr + 20 * a), m, int(col_stride), ctypes.c_void_p(crops_ptr + per_crop * a),
                                            ctypes.c_void_p(z_ptr + 4 * J * a), ctypes.c_void_p(idx_ptr + 8 * a), ctypes.c_void_p(score_ptr + 4 * a),
                                            ctypes.c_void_p(ws_e), nb_e, ctypes.c_void_p(ws_c), nb_c, stream)
            _lib.check(self.lib, rc, 'aae_detect_nn')

            def redo(a=a, m=m):                   # (split precision, out of range: the chunk again in exact fp32, from its crops)
                za, ia, sa = self.encode_nn(cb, crops[a:a + m], col_stride)
                z[a:a + m] = za
                score[a:a + m] = sa[:, 0]
                idx[a:a + m].copy_(ia[:, 0])
                torch.cuda.current_stream().synchronize()
            self._x3h_note(redo)

    def encode_nn(self, codebook_engine, x, col_stride=1, out=None, topk=1):
        """Encoder.z + the codebook query of a batch in one C call per chunk (aae_encode_nn; topk > 1: aae_encode_nn_topk): what
        Codebook.nearest_rotation does per detection.  Returns (z [B,J], idx int64 [B,topk], cosine float32 [B,topk]) on
        the device; bit-identical to encode() followed by codebook_engine.nn(z, topk, col_stride).  out: optional
        caller-owned (z, idx, score) device tensors of at least B rows to write into (a per-frame loop then allocates nothing)."""
        torch = _torch()
        cb = codebook_engine
        topk = int(topk)
        if topk < 1:
            raise ValueError('encode_nn: topk %d < 1' % topk)
        if topk > 1 and int(col_stride) != 1:
            raise ValueError('encode_nn: upright (col_stride > 1) is defined for topk == 1 only')
        if cb.device != self.device:
            raise ValueError('encode_nn: encoder on %s, codebook on %s -- one C call needs both on one device' % (self.device, cb.device))
        t = self.to_device_batch(x)
        B = t.shape[0]
        if out is not None:
            z, idx, score = out[0][:B], out[1][:B], out[2][:B]
            if (z.shape != (B, self.cfg.latent_space_size) or idx.shape != (B, topk) or score.shape != (B, topk) or z.dtype != torch.float32
                    or idx.dtype != torch.int64 or score.dtype != torch.float32 or not (z.is_contiguous() and idx.is_contiguous() and score.is_contiguous())
                    or z.device != self.device or idx.device != self.device or score.device != self.device):
                raise ValueError('encode_nn(out=...): need contiguous float32 [>=B,J], int64 [>=B,%d], float32 [>=B,%d] tensors on %s' % (topk, topk, self.device))
        else:
            z = torch.empty((B, self.cfg.latent_space_size), dtype=torch.float32, device=self.device)
            idx = torch.empty((B, topk), dtype=torch.int64, device=self.device)
            score = torch.empty((B, topk), dtype=torch.float32, device=self.device)
        if B == 0:
            return z, idx, score
        cb.ensure_upright(col_stride, topk)
        dt = _lib.AAE_DTYPE_U8 if t.dtype == torch.uint8 else _lib.AAE_DTYPE_F32
        for a in range(0, B, self.max_batch):
            e = min(a + self.max_batch, B)
            n = e - a
            nb_e = self.workspace_bytes(n)
            nb_c = cb.workspace_bytes(n, topk)
            _, ws_e = self.ws.get(nb_e)
            _, ws_c = cb.ws.get(nb_c)
            self._last_B = n
            with _on_device(self.device):
                if topk == 1:
                    rc = self.lib.aae_encode_nn(self.handle, cb.handle, ctypes.c_void_p(t[a:e].data_ptr()), dt, n, int(col_stride),
                                                ctypes.c_void_p(z[a:e].data_ptr()), ctypes.c_void_p(idx[a:e].data_ptr()),
                                                ctypes.c_void_p(score[a:e].data_ptr()), ctypes.c_void_p(ws_e), nb_e,
                                                ctypes.c_void_p(ws_c), nb_c, _stream_ptr(torch))
                else:
                    rc = self.lib.aae_encode_nn_topk(self.handle, cb.handle, ctypes.c_void_p(t[a:e].data_ptr()), dt, n, topk,
                                                     ctypes.c_void_p(z[a:e].data_ptr()), ctypes.c_void_p(idx[a:e].data_ptr()),
                                                     ctypes.c_void_p(score[a:e].data_ptr()), ctypes.c_void_p(ws_e), nb_e,
                                                     ctypes.c_void_p(ws_c), nb_c, _stream_ptr(torch))
            _lib.check(self.lib, rc, 'aae_encode_nn' if topk == 1 else 'aae_encode_nn_topk')

            def redo(a=a, e=e):
                za, ia, sa = self.encode_nn(cb, t[a:e], col_stride, topk=topk)
                z[a:e], idx[a:e], score[a:e] = za, ia, sa
            self._x3h_note(redo)
        return z, idx, score

    def encode_timed(self, x):
        """(z, [(kernel label, ms, algorithmic flops)]) for one chunk (B <= max_batch)."""
        torch = _torch()
        t = self.to_device_batch(x)
        if t.shape[0] > self.max_batch:
            raise ValueError('encode_timed takes at most max_batch=%d crops' % self.max_batch)
        z = torch.empty((t.shape[0], self.cfg.latent_space_size), dtype=torch.float32, device=self.device)
        return z, self._forward_chunk(t, z, timed=True)

    def activation(self, layer):
        """Layer output [B,Ho,Wo,Cout] of the most recent (single-chunk) forward."""
        torch = _torch()
        off, cnt = ctypes.c_size_t(), ctypes.c_size_t()
        _lib.check(self.lib, self.lib.aae_encoder_activation_info(self.handle, self._last_B, layer, ctypes.byref(off),
                                                                  ctypes.byref(cnt)), 'aae_encoder_activation_info')
        buf, ws_ptr = self.ws.get(0)
        start = ws_ptr - buf.data_ptr() + off.value
        _, _, _, Ho, Wo, Co = self.cfg.layer_shapes()[layer]
        raw = buf[start:start + 4 * cnt.value]
        if self.lib.aae_encoder_split_precision_for_batch(self.handle, int(self._last_B)):
            # f32x3h keeps activations as fp16 (hi, lo) pairs of value * 2^shift: [pixel][32-channel chunk][hi x 32 | lo x 32]
            pairs = raw.view(torch.float16).reshape(-1, 2, 32).to(torch.float64)      # chunks of the flat [B*Ho*Wo*Co] index
            return ((pairs[:, 0, :] + pairs[:, 1, :]).reshape(self._last_B, Ho, Wo, Co)
                    / 2.0 ** self.options.get('x3h_act_shift', 4)).to(torch.float32)
        return raw.view(torch.float32).reshape(self._last_B, Ho, Wo, Co).clone()

    # ---- the backward pass --------------------------
    def gradient_names(self):
        """the encoder's variables in the order of aae_encoder_create: kernel and bias of every convolution, then of the dense layer"""
        from .weights import conv_names
        return [n + s for n in list(conv_names(self.cfg.num_layers)) + ['dense'] for s in ('/kernel', '/bias')]

    def check_trainable(self):
        """NotImplementedError for what the backward pass is not built for"""
        from .encoder_grad import check_trainable
        check_trainable(self.cfg)

    def device_weights(self):
        """device copies of the weights the engine was created from, in checkpoint shapes (made on first use)"""
        torch = _torch()
        if self._dev_weights is None:
            self._dev_weights = [torch.from_numpy(np.array(a)).to(self.device) for a in self._host_weights]
        return self._dev_weights

    def backward(self, x, dz, out=None, need_dx=False, timed=False):
        """The gradient of every encoder variable from dz = dL/dz [B, latent], after encode(x) of the same batch (one chunk: the
        layer activations are read from the engine's workspace).  Returns (OrderedDict name -> tensor in checkpoint shape, dx
        [B,H,W,C] float32 or None); out: an OrderedDict of the caller's tensors to write into.  timed=True: also the list of
        (label, milliseconds) per launch (synchronises).  NotImplementedError, with nothing launched: batch norm, a stride of 3 or
        more, a forward that ran in split precision or with compact_workspace."""
        import collections
        torch = _torch()
        self.check_trainable()
        t = self.to_device_batch(x)
        B = int(t.shape[0])
        if self._last_B is None or B != self._last_B or B > self.max_batch:
            raise ValueError('backward() takes the batch of the last encode() as a single chunk: that was %s crops (max_batch %d), this is %d'
                             % (self._last_B, self.max_batch, B))
        if not isinstance(dz, torch.Tensor) or dz.dtype != torch.float32 or not dz.is_cuda or not dz.is_contiguous() or tuple(dz.shape) != (B, self.cfg.latent_space_size):
            raise ValueError('dz must be a contiguous float32 device tensor of shape %s' % ((B, self.cfg.latent_space_size),))
        weights = self.device_weights()
        names = self.gradient_names()
        if out is None:
            grads = collections.OrderedDict((n, torch.empty_like(w)) for n, w in zip(names, weights))
        else:
            grads = collections.OrderedDict((n, out[n]) for n in names)
            for (n, g), w in zip(grads.items(), weights):
                if not isinstance(g, torch.Tensor) or g.dtype != torch.float32 or g.device != w.device or not g.is_contiguous() or g.shape != w.shape:
                    raise ValueError('out[%r] must be a contiguous float32 tensor of shape %s on %s' % (n, tuple(w.shape), w.device))
        dx = torch.empty(t.shape, dtype=torch.float32, device=self.device) if need_dx else None
        need = max(int(self.lib.aae_encoder_backward_workspace_bytes(self.handle, B)), 256)         # (0: the call below says why it refuses)
        if self._bwd_ws is None or self._bwd_ws.numel() < need:
            self._bwd_ws = torch.empty((need,), dtype=torch.uint8, device=self.device)
        _, fwd_ptr = self.ws.get(0)
        n = len(weights)
        wp = (ctypes.c_void_p * n)(*[w.data_ptr() for w in weights])
        gp = (ctypes.c_void_p * n)(*[g.data_ptr() for g in grads.values()])
        dt = _lib.AAE_DTYPE_U8 if t.dtype == torch.uint8 else _lib.AAE_DTYPE_F32
        args = [self.handle, B, ctypes.c_void_p(t.data_ptr()), dt, ctypes.c_void_p(dz.data_ptr()), ctypes.c_void_p(fwd_ptr), wp, gp,
                ctypes.c_void_p(dx.data_ptr()) if need_dx else None, ctypes.c_void_p(self._bwd_ws.data_ptr()), int(self._bwd_ws.numel()), _stream_ptr(torch)]
        ms = (ctypes.c_float * 64)()
        cnt = ctypes.c_int(0)
        with _on_device(self.device):
            if timed:
                rc, what = self.lib.aae_encoder_backward_timed(*(args + [ms, 64, ctypes.byref(cnt)])), 'aae_encoder_backward_timed'
            else:
                rc, what = self.lib.aae_encoder_backward(*args), 'aae_encoder_backward'
        if rc == -2:
            msg = self.lib.aae_last_error()
            raise NotImplementedError(msg.decode('utf-8', 'replace') if msg else what)
        _lib.check(self.lib, rc, what)
        if not timed:
            return grads, dx
        return grads, dx, [(self.lib.aae_encoder_bwd_label(i).decode(), float(ms[i])) for i in range(cnt.value)]


class CodebookEngine(object):
    """Owns one aae_codebook handle: the device-resident embedding_normalized
    variable (codebook.py:28-36) and the fused normalise + scan + arg-max."""

    def __init__(self, embedding_normalized, device=None, dtype='f32'):
        """dtype 'f32' (reference storage) or 'bf16' (half the bytes per row: the float32
        codebook is rounded to bfloat16 once, queries keep fp32 accuracy -- see
        csrc/kernels/codebook_scan_bf16.h)."""
        torch = _torch()
        self.device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        self.lib = _lib.load()
        self.dtype = dtype
        handle = ctypes.c_void_p()
        with _on_device(self.device):
            if dtype == 'bf16':
                from .weights import to_bf16_bits
                src = embedding_normalized.cpu().numpy() if torch.is_tensor(embedding_normalized) else embedding_normalized
                E = to_bf16_bits(src)
                self.N, self.J = int(E.shape[0]), int(E.shape[1])
                rc = self.lib.aae_codebook_create(E.ctypes.data, self.N, self.J, _lib.AAE_DTYPE_BF16, 0, ctypes.byref(handle))
            elif dtype != 'f32':
                raise ValueError("codebook dtype must be 'f32' or 'bf16', got %r" % (dtype,))
            elif torch.is_tensor(embedding_normalized):
                E = embedding_normalized.to(self.device, torch.float32).contiguous()
                self.N, self.J = int(E.shape[0]), int(E.shape[1])
                torch.cuda.synchronize(self.device)
                rc = self.lib.aae_codebook_create(ctypes.c_void_p(E.data_ptr()), self.N, self.J, _lib.AAE_DTYPE_F32, 1, ctypes.byref(handle))
            else:
                E = np.ascontiguousarray(np.asarray(embedding_normalized, dtype=np.float32))
                self.N, self.J = int(E.shape[0]), int(E.shape[1])
                rc = self.lib.aae_codebook_create(E.ctypes.data, self.N, self.J, _lib.AAE_DTYPE_F32, 0, ctypes.byref(handle))
        _lib.check(self.lib, rc, 'aae_codebook_create')
        self.handle = handle
        self.ws = _Workspace(self.device)
        self._ws_bytes = {}               # (batch, topk) -> aae_codebook_workspace_bytes
        self._upright_stride = 0          # stride the compacted upright copy was prepared for (0 = none yet)

    def close(self):
        if getattr(self, 'handle', None):
            self.lib.aae_codebook_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_scan_mode(self, mode):
        _lib.check(self.lib, self.lib.aae_codebook_set_scan_mode(self.handle, int(mode)), 'aae_codebook_set_scan_mode')
        self._ws_bytes.clear()

    def workspace_bytes(self, B, topk):
        n = self._ws_bytes.get((B, topk))
        if n is None:
            n = self._ws_bytes[(B, topk)] = self.lib.aae_codebook_workspace_bytes(self.handle, B, topk)
        return n

    def update(self, embedding_normalized):
        torch = _torch()
        E = np.ascontiguousarray(np.asarray(embedding_normalized, dtype=np.float32))
        if E.shape != (self.N, self.J):
            raise ValueError('embedding has shape %s, codebook is [%d,%d]' % (E.shape, self.N, self.J))
        if self.dtype == 'bf16':
            from .weights import to_bf16_bits
            E = to_bf16_bits(E)
        with _on_device(self.device):
            rc = self.lib.aae_codebook_update(self.handle, E.ctypes.data, 0, _stream_ptr(torch))
        _lib.check(self.lib, rc, 'aae_codebook_update')

    def _z(self, z):
        torch = _torch()
        if isinstance(z, np.ndarray):
            z = torch.from_numpy(np.ascontiguousarray(z, dtype=np.float32))
        z = z.to(self.device, torch.float32).contiguous()
        if z.dim() != 2 or z.shape[1] != self.J:
            raise ValueError('latents have shape %s, expected [B,%d]' % (tuple(z.shape), self.J))
        return z

    def ensure_upright(self, col_stride, topk=1):
        """First upright query with this stride: build the every-k-th-row copy the scan then runs over (allocates once;
        a CapturedNearestNeighbour reaches this in its eager warm-up call, before the capture starts)."""
        if col_stride > 1 and topk == 1 and self._upright_stride != int(col_stride):
            torch = _torch()
            with _on_device(self.device):
                rc = self.lib.aae_codebook_prepare_upright(self.handle, int(col_stride), _stream_ptr(torch))
            _lib.check(self.lib, rc, 'aae_codebook_prepare_upright')
            self._upright_stride = int(col_stride)

    def nn(self, z, topk=1, col_stride=1):
        """(idx int64 [B,topk], cosine float32 [B,topk]) on the device."""
        torch = _torch()
        z = self._z(z)
        B = z.shape[0]
        idx = torch.empty((B, topk), dtype=torch.int64, device=self.device)
        score = torch.empty((B, topk), dtype=torch.float32, device=self.device)
        if B == 0:                    # an empty batch is an empty answer (TF/NumPy semantics of the reference), not an error
            return idx, score
        self.ensure_upright(col_stride, topk)
        nbytes = self.workspace_bytes(B, topk)
        _, ws_ptr = self.ws.get(nbytes)
        with _on_device(self.device):
            rc = self.lib.aae_codebook_nn(self.handle, ctypes.c_void_p(z.data_ptr()), B, int(topk), int(col_stride),
                                          ctypes.c_void_p(idx.data_ptr()), ctypes.c_void_p(score.data_ptr()),
                                          ctypes.c_void_p(ws_ptr), nbytes, _stream_ptr(torch))
        _lib.check(self.lib, rc, 'aae_codebook_nn')
        return idx, score

    def nn_timed(self, z, topk=1, col_stride=1, reps=100):
        """nn() `reps` times back to back, queued from C between two HIP events: (idx, score, device milliseconds per query --
        kernel(s) + dependent-launch gap, free of the per-call host cost of a Python loop)."""
        torch = _torch()
        z = self._z(z)
        B = z.shape[0]
        idx = torch.empty((B, topk), dtype=torch.int64, device=self.device)
        score = torch.empty((B, topk), dtype=torch.float32, device=self.device)
        self.ensure_upright(col_stride, topk)
        nbytes = self.workspace_bytes(B, topk)
        _, ws_ptr = self.ws.get(nbytes)
        ms = ctypes.c_float(0.0)
        with _on_device(self.device):
            rc = self.lib.aae_codebook_nn_timed(self.handle, ctypes.c_void_p(z.data_ptr()), B, int(topk), int(col_stride),
                                                ctypes.c_void_p(idx.data_ptr()), ctypes.c_void_p(score.data_ptr()),
                                                ctypes.c_void_p(ws_ptr), nbytes, _stream_ptr(torch), int(reps), ctypes.byref(ms))
        _lib.check(self.lib, rc, 'aae_codebook_nn_timed')
        return idx, score, float(ms.value)

    def similarity(self, z):
        """Full cos_similarity [B,N] (codebook.py:50) on the device."""
        torch = _torch()
        z = self._z(z)
        B = z.shape[0]
        cs = torch.empty((B, self.N), dtype=torch.float32, device=self.device)
        if B == 0:
            return cs
        nbytes = self.workspace_bytes(B, 1)
        _, ws_ptr = self.ws.get(nbytes)
        with _on_device(self.device):
            rc = self.lib.aae_codebook_similarity(self.handle, ctypes.c_void_p(z.data_ptr()), B, ctypes.c_void_p(cs.data_ptr()),
                                                  ctypes.c_void_p(ws_ptr), nbytes, _stream_ptr(torch))
        _lib.check(self.lib, rc, 'aae_codebook_similarity')
        return cs

    def l2_normalize(self, z):
        torch = _torch()
        z = self._z(z)
        q = torch.empty_like(z)
        if z.shape[0] == 0:
            return q
        with _on_device(self.device):
            rc = self.lib.aae_l2_normalize(ctypes.c_void_p(z.data_ptr()), z.shape[0], z.shape[1], ctypes.c_void_p(q.data_ptr()),
                                           _stream_ptr(torch))
        _lib.check(self.lib, rc, 'aae_l2_normalize')
        return q


class MultiObjectQuery(object):
    """A frame's detections of SEVERAL objects in one C call (aae_encode_nn_multi): the reference keeps one AAE per object
    class in one process and runs one session.run per detected box, whatever its class
    (m3_interface/ae_pose_estimator.py:61-78,143-170; 30 classes for T-LESS, cfg_m3vision/m3_config_tless.cfg:10-39).
    items: [(EncoderEngine, CodebookEngine, n detections[, col_stride])] in the order the crops are concatenated.  Items
    with n <= 4 at the default options are GROUPED -- one launch per layer across all of them, objects with different
    detection counts included (six launches for the frame instead of six per object); items with n >= 5 whose conv layers
    run as Winograd share one launch per conv layer when together they fill the chip (eight buckets of ~32 crops: the
    reference's one-AAE-per-class frame at B = 256); the rest take the per-object path inside the same call.  Against one
    EncoderEngine.encode_nn call per item the answers differ by fp32 summation order only (a group brings its own launch
    plan, as a batch of another size does: <= 2.3e-6 of the latent scale, indices equal wherever the top-2 gap exceeds
    that); encoder option multi_group_plan = 0 (and multi_mid_group = 0) makes them bit-identical.  The layout is fixed at construction (a detector's class mix changes per
    frame: AePoseEstimator builds the item array per frame instead -- detect_nn_multi below); outputs are static device
    tensors, valid until the next call."""

    def __init__(self, items, device=None):
        torch = _torch()
        self.lib = _lib.load()
        norm = [(it[0], it[1], int(it[2]), int(it[3]) if len(it) > 3 else 1) for it in items]
        if not norm:
            raise ValueError('MultiObjectQuery needs at least one item')
        self.device = norm[0][1].device if device is None else torch.device(device)
        for enc, cb, n, stride in norm:
            if cb.device != self.device or (enc is not None and enc.device != self.device):
                raise ValueError('MultiObjectQuery: every engine must live on %s' % (self.device,))
            cb.ensure_upright(stride, 1)
        self._keep = norm                                   # the engines own the handles: keep them alive
        self.items = multi_item_array(norm)
        self.n_items = len(norm)
        self.rows = int(self.lib.aae_multi_rows(self.items, self.n_items))
        encs = [e for e, _, _, _ in norm if e is not None]
        self.cfg = encs[0].cfg if encs else None
        self.J = norm[0][1].J
        self.ws = _Workspace(self.device)
        self.z = torch.empty((self.rows, self.J), dtype=torch.float32, device=self.device)
        self.idx = torch.empty((self.rows,), dtype=torch.int64, device=self.device)
        self.score = torch.empty((self.rows,), dtype=torch.float32, device=self.device)
        self.launches = None                                # kernel launches of the grouped part of the last call

    def __call__(self, x):
        """x: the crops of all items, [rows,H,W,C] uint8 or float32 on the device, in item order -> (z, idx, score)"""
        torch = _torch()
        if self.cfg is None:
            raise ValueError('MultiObjectQuery without encoders answers nn(z) only')
        if (not torch.is_tensor(x) or x.device != self.device or not x.is_contiguous() or tuple(x.shape) != (self.rows,) + tuple(self.cfg.shape)
                or x.dtype not in (torch.uint8, torch.float32)):
            raise ValueError('MultiObjectQuery: need a contiguous uint8 / float32 device tensor of shape %s' % (((self.rows,) + tuple(self.cfg.shape)),))
        dt = _lib.AAE_DTYPE_U8 if x.dtype == torch.uint8 else _lib.AAE_DTYPE_F32
        nbytes = self.lib.aae_multi_workspace_bytes(self.items, self.n_items, 0)
        _, ws_ptr = self.ws.get(nbytes)
        with _on_device(self.device):
            rc = self.lib.aae_encode_nn_multi(self.items, self.n_items, ctypes.c_void_p(x.data_ptr()), dt, ctypes.c_void_p(self.z.data_ptr()),
                                              ctypes.c_void_p(self.idx.data_ptr()), ctypes.c_void_p(self.score.data_ptr()),
                                              ctypes.c_void_p(ws_ptr), nbytes, _stream_ptr(torch))
        _lib.check(self.lib, rc, 'aae_encode_nn_multi')
        self.launches = int(self.lib.aae_multi_last_launches())
        return self.z, self.idx, self.score

    def nn(self, z):
        """the codebook stage alone (aae_codebook_nn_multi): z [rows,J] raw latent codes in item order -> (idx, score);
        the grouped items' codebooks are streamed by ONE launch per distinct n"""
        torch = _torch()
        if not torch.is_tensor(z) or z.device != self.device or z.dtype != torch.float32 or not z.is_contiguous() or tuple(z.shape) != (self.rows, self.J):
            raise ValueError('MultiObjectQuery.nn: need a contiguous float32 device tensor [%d,%d]' % (self.rows, self.J))
        nbytes = self.lib.aae_multi_workspace_bytes(self.items, self.n_items, 1)
        _, ws_ptr = self.ws.get(nbytes)
        with _on_device(self.device):
            rc = self.lib.aae_codebook_nn_multi(self.items, self.n_items, ctypes.c_void_p(z.data_ptr()), ctypes.c_void_p(self.idx.data_ptr()),
                                                ctypes.c_void_p(self.score.data_ptr()), ctypes.c_void_p(ws_ptr), nbytes, _stream_ptr(torch))
        _lib.check(self.lib, rc, 'aae_codebook_nn_multi')
        self.launches = int(self.lib.aae_multi_last_launches())
        return self.idx, self.score


def multi_item_array(items):
    """[(EncoderEngine or None, CodebookEngine, n, col_stride)] -> the aae_multi_item array of the C ABI"""
    arr = (_lib.MultiItem * len(items))()
    for k, (enc, cb, n, stride) in enumerate(items):
        arr[k].enc = enc.handle if enc is not None else None
        arr[k].cb = cb.handle
        arr[k].n = int(n)
        arr[k].col_stride = int(stride)
    return arr


def detect_nn_multi(items, image, rows, crops, z, idx, score, ws):
    """ALL detections of a frame -- every class, in the order of `items` [(EncoderEngine, CodebookEngine, n, col_stride)] -- in
    ONE C call (aae_detect_nn_multi): crop + bilinear resize of the boxes `rows` (int32 [total,5]) out of `image`, then
    one launch per layer across the classes with at most four detections each (per-object path for the rest).  Storage as
    for EncoderEngine.detect_nn; ws: a _Workspace on the engines' device.  Returns the launches of the grouped part."""
    torch = _torch()
    lib = _lib.load()
    arr = multi_item_array(items)
    k = len(items)
    dev = items[0][0].device
    for enc, cb, n, stride in items:
        cb.ensure_upright(stride, 1)
    nbytes = lib.aae_multi_workspace_bytes(arr, k, 0)
    _, ws_ptr = ws.get(nbytes)
    with _on_device(dev):
        rc = lib.aae_detect_nn_multi(arr, k, ctypes.c_void_p(image.data_ptr()), int(image.shape[0]), int(image.shape[1]), int(image.shape[2]),
                                     ctypes.c_void_p(rows.data_ptr()), ctypes.c_void_p(crops.data_ptr()), ctypes.c_void_p(z.data_ptr()),
                                     ctypes.c_void_p(idx.data_ptr()), ctypes.c_void_p(score.data_ptr()), ctypes.c_void_p(ws_ptr), nbytes,
                                     _stream_ptr(torch))
    _lib.check(lib, rc, 'aae_detect_nn_multi')
    return int(lib.aae_multi_last_launches())


def _pair_operand(t, dtype, device, what):
    torch = _torch()
    if not torch.is_tensor(t) or t.dtype != dtype or t.device != device:
        raise ValueError('%s must be a %s tensor on %s, got %s' % (what, dtype, device,
                                                                   (t.dtype, t.device) if torch.is_tensor(t) else type(t)))
    return t.contiguous()


def pack_pairs(idx, score, pos, packed):
    """packed[pos[i]] = (idx[i, 0], float bits of score[i, 0]) in one launch (aae_pack_pairs): the payload of the
    multi-GPU gather.  idx int64 [n,k], score float32 [n,k], pos int32 [n] device tensor or None (rows 0..n-1),
    packed int64 [capacity, 2] -- all on one device."""
    torch = _torch()
    lib = _lib.load()
    n = int(idx.shape[0])
    if n == 0:
        return packed
    if packed.dtype != torch.int64 or not packed.is_contiguous():
        raise ValueError('packed must be a contiguous int64 [capacity, 2] tensor')
    idx = _pair_operand(idx, torch.int64, packed.device, 'idx')
    score = _pair_operand(score, torch.float32, packed.device, 'score')
    if tuple(score.shape) != tuple(idx.shape):
        raise ValueError('idx %s and score %s differ in shape' % (tuple(idx.shape), tuple(score.shape)))
    stride = int(idx.shape[1]) if idx.dim() == 2 else 1
    if pos is not None:
        if pos.dtype != torch.int32:
            pos = pos.to(torch.int32)
        pos = _pair_operand(pos, torch.int32, packed.device, 'pos')
    with _on_device(packed.device):
        rc = lib.aae_pack_pairs(ctypes.c_void_p(idx.data_ptr()), ctypes.c_void_p(score.data_ptr()),
                                ctypes.c_void_p(pos.data_ptr()) if pos is not None else None, n, stride,
                                ctypes.c_void_p(packed.data_ptr()), _stream_ptr(torch))
    _lib.check(lib, rc, 'aae_pack_pairs')
    return packed


def unpack_pairs(gathered, owner, n, rows_per_rank, idx_out, score_out):
    """The inverse after the all_gather (aae_unpack_pairs, one launch): idx_out[i], score_out[i] = row i of block
    owner[i] of gathered [world * rows_per_rank, 2] (owner None: block 0).  Outputs are caller-owned (pre-allocated)."""
    torch = _torch()
    lib = _lib.load()
    if n == 0:
        return idx_out, score_out
    dev = gathered.device
    gathered = _pair_operand(gathered, torch.int64, dev, 'gathered')
    if owner is not None:
        owner = _pair_operand(owner, torch.int32, dev, 'owner')
    if (idx_out.dtype != torch.int64 or score_out.dtype != torch.float32 or not idx_out.is_contiguous() or not score_out.is_contiguous()
            or idx_out.device != dev or score_out.device != dev or idx_out.numel() < n or score_out.numel() < n):
        raise ValueError('unpack_pairs: outputs must be contiguous int64 / float32 tensors of at least n elements on %s' % dev)
    with _on_device(dev):
        rc = lib.aae_unpack_pairs(ctypes.c_void_p(gathered.data_ptr()), ctypes.c_void_p(owner.data_ptr()) if owner is not None else None,
                                  int(n), int(rows_per_rank), ctypes.c_void_p(idx_out.data_ptr()), ctypes.c_void_p(score_out.data_ptr()),
                                  _stream_ptr(torch))
    _lib.check(lib, rc, 'aae_unpack_pairs')
    return idx_out, score_out


def crop_resize_into(image_dev, boxes_dev, out):
    """The launch alone, on buffers the caller owns: image_dev uint8 [H,W,C], boxes_dev int32 [D,5] rows (x, y, w, h, size),
    out uint8 [D,out_h,out_w,C] -- contiguous tensors on one device; nothing is allocated or copied here."""
    torch = _torch()
    lib = _lib.load()
    dev = out.device
    if (image_dev.dtype != torch.uint8 or out.dtype != torch.uint8 or boxes_dev.dtype != torch.int32 or image_dev.dim() != 3 or out.dim() != 4
            or boxes_dev.dim() != 2 or boxes_dev.shape[1] != 5 or boxes_dev.shape[0] != out.shape[0] or out.shape[3] != image_dev.shape[2]
            or image_dev.device != dev or boxes_dev.device != dev
            or not (image_dev.is_contiguous() and boxes_dev.is_contiguous() and out.is_contiguous())):
        raise ValueError('crop_resize_into: need contiguous uint8 [H,W,C], int32 [D,5], uint8 [D,h,w,C] tensors on one device')
    if out.shape[0] == 0:
        return out
    with _on_device(dev):
        rc = lib.aae_crop_resize_u8(ctypes.c_void_p(image_dev.data_ptr()), int(image_dev.shape[0]), int(image_dev.shape[1]), int(image_dev.shape[2]),
                                    ctypes.c_void_p(boxes_dev.data_ptr()), int(out.shape[0]), int(out.shape[1]), int(out.shape[2]),
                                    ctypes.c_void_p(out.data_ptr()), _stream_ptr(torch))
    _lib.check(lib, rc, 'aae_crop_resize_u8')
    return out


def crop_resize(image, boxes_xywh_size, out_hw, device=None):
    """All detector crops of one image in one launch (extract_square_patch(black_borders=True) +
    cv2.resize(INTER_LINEAR), m3_interface/ae_pose_estimator.py:106-131).
    image: uint8 [H,W,C] numpy array or device tensor; boxes_xywh_size: int [D,5] rows
    (x, y, w, h, size); returns a device uint8 tensor [D, out_h, out_w, C]."""
    torch = _torch()
    lib = _lib.load()
    dev = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    if isinstance(image, np.ndarray):
        if image.dtype != np.uint8:
            raise TypeError('crop_resize needs a uint8 image, got %s' % image.dtype)
        img = torch.from_numpy(np.ascontiguousarray(image)).to(dev)
    else:
        if image.dtype != torch.uint8:
            raise TypeError('crop_resize needs a uint8 image, got %s' % image.dtype)
        img = image.to(dev).contiguous()
    if img.dim() != 3:
        raise ValueError('image must be [H,W,C], got shape %s' % (tuple(img.shape),))
    boxes = torch.from_numpy(np.ascontiguousarray(np.asarray(boxes_xywh_size, dtype=np.int32).reshape(-1, 5))).to(dev)
    D = int(boxes.shape[0])
    oh, ow = int(out_hw[0]), int(out_hw[1])
    out = torch.empty((D, oh, ow, int(img.shape[2])), dtype=torch.uint8, device=dev)
    if D == 0:
        return out
    with _on_device(dev):
        rc = lib.aae_crop_resize_u8(ctypes.c_void_p(img.data_ptr()), int(img.shape[0]), int(img.shape[1]), int(img.shape[2]),
                                    ctypes.c_void_p(boxes.data_ptr()), D, oh, ow, ctypes.c_void_p(out.data_ptr()),
                                    _stream_ptr(torch))
    _lib.check(lib, rc, 'aae_crop_resize_u8')
    return out


class DecoderEngine(object):
    """Owns one aae_decoder handle: Decoder.x of /root/reference/auto_pose/ae/decoder.py:36-84
    (dense -> [nearest-neighbour resize -> conv]* -> sigmoid) for batches of latent codes."""

    def __init__(self, cfg, weights, device=None, max_batch=256):
        from .weights import ordered_decoder_weight_arrays
        torch = _torch()
        self.cfg = cfg
        self.device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        self.max_batch = int(max_batch)
        self.lib = _lib.load()
        arrays = ordered_decoder_weight_arrays(weights, cfg)
        handle = ctypes.c_void_p()
        desc = cfg.to_desc()
        with _on_device(self.device):
            rc = self.lib.aae_decoder_create(ctypes.byref(desc), as_pointer_array(arrays), len(arrays), ctypes.byref(handle))
        _lib.check(self.lib, rc, 'aae_decoder_create')
        self.handle = handle
        self.ws = _Workspace(self.device)
        self._last_B = None
        self._host_weights = arrays             # what backward() differentiates with respect to: copied to the device on first use
        dense, convs, final, _ = cfg.variable_names(weights)
        self._grad_names = [n + s for n in [dense] + list(convs) + [final] for s in ('/kernel', '/bias')]
        self._dev_weights = None
        self._bwd_ws = None

    def close(self):
        if getattr(self, 'handle', None):
            self.lib.aae_decoder_destroy(self.handle)
            self.handle = None
        self._dev_weights = None
        self._bwd_ws = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _z(self, z):
        torch = _torch()
        if isinstance(z, np.ndarray):
            z = torch.from_numpy(np.ascontiguousarray(z, dtype=np.float32))
        z = z.to(self.device, torch.float32).contiguous()
        if z.dim() == 1:
            z = z.unsqueeze(0)
        if z.dim() != 2 or z.shape[1] != self.cfg.latent_space_size:
            raise ValueError('latent batch has shape %s, decoder expects [B,%d]' % (tuple(z.shape), self.cfg.latent_space_size))
        return z

    def _chunk(self, z, out, timed=False):
        torch = _torch()
        B = z.shape[0]
        nbytes = self.lib.aae_decoder_workspace_bytes(self.handle, B)
        _, ws_ptr = self.ws.get(nbytes)
        self._last_B = B
        with _on_device(self.device):
            if not timed:
                rc = self.lib.aae_decoder_forward(self.handle, ctypes.c_void_p(z.data_ptr()), B, ctypes.c_void_p(out.data_ptr()),
                                                  ctypes.c_void_p(ws_ptr), nbytes, _stream_ptr(torch))
                _lib.check(self.lib, rc, 'aae_decoder_forward')
                return None
            ms = (ctypes.c_float * 32)()
            n = ctypes.c_int(0)
            rc = self.lib.aae_decoder_forward_timed(self.handle, ctypes.c_void_p(z.data_ptr()), B, ctypes.c_void_p(out.data_ptr()),
                                                    ctypes.c_void_p(ws_ptr), nbytes, _stream_ptr(torch), ms, 32, ctypes.byref(n))
            _lib.check(self.lib, rc, 'aae_decoder_forward_timed')
            return [(self.lib.aae_decoder_kernel_label(self.handle, i).decode(), float(ms[i]),
                     float(self.lib.aae_decoder_kernel_flops(self.handle, i))) for i in range(n.value)]

    def target_batch(self, target, shape):
        """a reconstruction target (np.ndarray or torch.Tensor, float) as a contiguous float32 device tensor of `shape`"""
        torch = _torch()
        if isinstance(target, np.ndarray):
            target = torch.from_numpy(np.ascontiguousarray(target, dtype=np.float32))
        elif not torch.is_tensor(target):
            raise TypeError('the reconstruction target must be a numpy array or a torch tensor, got %r' % type(target))
        t = target.to(self.device, torch.float32).contiguous()
        if tuple(t.shape) != tuple(shape):
            raise ValueError('the reconstruction target has shape %s, the reconstruction %s' % (tuple(t.shape), tuple(shape)))
        return t

    def decode(self, z, out=None):
        """Decoder.x: device float32 [B,H,W,C] in [0,1].  out: the caller's tensor to decode into (contiguous float32
        [B,H,W,C] on the engine's device; returned) -- every element of it is written."""
        torch = _torch()
        z = self._z(z)
        B = z.shape[0]
        shape = (B,) + tuple(self.cfg.shape)
        if out is None:
            out = torch.empty(shape, dtype=torch.float32, device=self.device)
        else:
            if not isinstance(out, torch.Tensor):
                raise ValueError('out must be a torch tensor, got %s' % type(out).__name__)
            if tuple(out.shape) != shape:
                raise ValueError('out has shape %s, this call decodes into %s' % (tuple(out.shape), shape))
            if out.dtype != torch.float32:
                raise ValueError('out has dtype %s, the decoder writes float32' % out.dtype)
            if out.device.type != self.device.type or (out.device.index or 0) != (self.device.index or 0):
                raise ValueError('out lives on %s, the decoder on %s' % (out.device, self.device))
            if not out.is_contiguous():
                raise ValueError('out must be contiguous')
        for a in range(0, B, self.max_batch):
            e = min(a + self.max_batch, B)
            self._chunk(z[a:e], out[a:e])
        return out

    def decode_timed(self, z):
        torch = _torch()
        z = self._z(z)
        if z.shape[0] > self.max_batch:
            raise ValueError('decode_timed takes at most max_batch=%d codes' % self.max_batch)
        out = torch.empty((z.shape[0],) + tuple(self.cfg.shape), dtype=torch.float32, device=self.device)
        return out, self._chunk(z, out, timed=True)

    def gradient_names(self):
        """the decoder's variables in the order of aae_decoder_create: kernel and bias of the dense layer, of every hidden
        convolution, of the output convolution"""
        return list(self._grad_names)

    def check_trainable(self):
        """NotImplementedError for what the backward pass is not built for"""
        from .decoder_grad import check_trainable
        check_trainable(self.cfg)

    def device_weights(self):
        """device copies of the weights the engine was created from, in checkpoint shapes (made on first use)"""
        torch = _torch()
        if self._dev_weights is None:
            self._dev_weights = [torch.from_numpy(np.array(a)).to(self.device) for a in self._host_weights]
        return self._dev_weights

    def backward(self, z, x, dx, out=None, timed=False):
        """The gradient of every decoder variable and dL/dz from dx = dL/dx, after decode(z) -> x of the same batch (one chunk:
        the hidden activations are read from the engine's workspace).  Returns (OrderedDict name -> tensor in checkpoint shape, dz
        [B, latent]); out: an OrderedDict of the caller's tensors to write into.  timed=True: also the list of
        (label, milliseconds) per launch (synchronises)."""
        import collections
        torch = _torch()
        self.check_trainable()
        z = self._z(z)
        B = int(z.shape[0])
        if self._last_B is None or B != self._last_B or B > self.max_batch:
            raise ValueError('backward() takes the batch of the last decode() as a single chunk: that was %s codes (max_batch %d), this is %d'
                             % (self._last_B, self.max_batch, B))
        shape = (B,) + tuple(self.cfg.shape)
        for t, name in ((x, 'x'), (dx, 'dx')):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous() or tuple(t.shape) != shape:
                raise ValueError('%s must be a contiguous float32 device tensor of shape %s' % (name, shape))
        weights = self.device_weights()
        names = self.gradient_names()
        if out is None:
            grads = collections.OrderedDict((n, torch.empty_like(w)) for n, w in zip(names, weights))
        else:
            grads = collections.OrderedDict((n, out[n]) for n in names)
            for (n, g), w in zip(grads.items(), weights):
                if not isinstance(g, torch.Tensor) or g.dtype != torch.float32 or g.device != w.device or not g.is_contiguous() or g.shape != w.shape:
                    raise ValueError('out[%r] must be a contiguous float32 tensor of shape %s on %s' % (n, tuple(w.shape), w.device))
        dz = torch.empty_like(z)
        need = int(self.lib.aae_decoder_backward_workspace_bytes(self.handle, B))
        if need == 0:
            _lib.check(self.lib, -2, 'aae_decoder_backward_workspace_bytes')
        if self._bwd_ws is None or self._bwd_ws.numel() < need:
            self._bwd_ws = torch.empty((need,), dtype=torch.uint8, device=self.device)
        _, fwd_ptr = self.ws.get(0)
        n = len(weights)
        wp = (ctypes.c_void_p * n)(*[w.data_ptr() for w in weights])
        gp = (ctypes.c_void_p * n)(*[g.data_ptr() for g in grads.values()])
        args = [self.handle, B, ctypes.c_void_p(z.data_ptr()), ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(dx.data_ptr()), ctypes.c_void_p(fwd_ptr), wp, gp,
                ctypes.c_void_p(dz.data_ptr()), ctypes.c_void_p(self._bwd_ws.data_ptr()), int(self._bwd_ws.numel()), _stream_ptr(torch)]
        with _on_device(self.device):
            if not timed:
                _lib.check(self.lib, self.lib.aae_decoder_backward(*args), 'aae_decoder_backward')
                return grads, dz
            ms = (ctypes.c_float * 64)()
            cnt = ctypes.c_int(0)
            _lib.check(self.lib, self.lib.aae_decoder_backward_timed(*(args + [ms, 64, ctypes.byref(cnt)])), 'aae_decoder_backward_timed')
        return grads, dz, [(self.lib.aae_decoder_bwd_label(i).decode(), float(ms[i])) for i in range(cnt.value)]

    def activation(self, stage):
        """Hidden activation of the most recent single-chunk decode: stage 0 = dense output
        [B,h0,w0,F0], stage i = output of the i-th hidden convolution."""
        torch = _torch()
        off, cnt = ctypes.c_size_t(), ctypes.c_size_t()
        _lib.check(self.lib, self.lib.aae_decoder_activation_info(self.handle, self._last_B, stage, ctypes.byref(off),
                                                                  ctypes.byref(cnt)), 'aae_decoder_activation_info')
        buf, ws_ptr = self.ws.get(0)
        start = ws_ptr - buf.data_ptr() + off.value
        dims = self.cfg.layer_dimensions()[stage]
        return buf[start:start + 4 * cnt.value].view(torch.float32).reshape(self._last_B, dims[0], dims[1],
                                                                              self.cfg.num_filters[stage]).clone()


class CapturedNearestNeighbour(object):
    """encode + codebook nearest-neighbour for one fixed batch shape, recorded once into a HIP
    graph and replayed: the launches of a small-batch query (six for B <= 4: conv1, three wave-split-K
    convolutions, dense GEMV, scan) without the host-side launch cost -- the shape the reference's
    per-detection loop uses (m3_interface/ae_pose_estimator.py:143-170).  On the GPU side a replay
    takes as long as the eager launches (the chain is kernel-bound); the gain is host time.
    Inputs are copied into a static buffer; outputs are static device tensors, valid until the
    next call.  Results are bit-identical to the eager calls (same kernels, same order).  Captured in
    split-precision mode ('precision' 1 / 2 on a batch that runs f32x3h) every replay is followed by a look at the
    forward's range flag (a host round trip) and, if it is up, by an eager exact-fp32 recomputation -- the same
    guarantee the eager path gives."""

    def __init__(self, encoder_engine, codebook_engine, batch, in_dtype='uint8', topk=1, col_stride=1, force_graph=False):
        """force_graph: record and replay a graph also for the per-detection batches (B <= 4, top-1), where the fused eager call
        -- ONE C call that queues the six launches -- is measured FASTER than a graph replay (81.8 vs 87.0 us at B = 1: a replay
        costs the host 10-16 us, the C call 3-5): there the object keeps its interface (static input / output tensors) and
        simply makes that call.  bench.py forces the graph to keep measuring it."""
        torch = _torch()
        self.enc, self.cb = encoder_engine, codebook_engine
        self.batch, self.topk, self.col_stride = int(batch), int(topk), int(col_stride)
        dt = torch.uint8 if in_dtype in ('uint8', torch.uint8) else torch.float32
        dev = encoder_engine.device
        self._x3h_slot = -1
        self.graph = None
        self.x = torch.zeros((self.batch,) + tuple(encoder_engine.cfg.shape), dtype=dt, device=dev)
        self.eager = self.batch <= 4 and self.topk == 1 and not force_graph
        if self.eager:
            self.z = torch.empty((self.batch, encoder_engine.cfg.latent_space_size), dtype=torch.float32, device=dev)
            self.idx = torch.empty((self.batch, 1), dtype=torch.int64, device=dev)
            self.score = torch.empty((self.batch, 1), dtype=torch.float32, device=dev)
            self._ws = None
            return
        # The graph bakes raw device addresses: its scratch memory must outlive it and must never be regrown by somebody
        # else.  So the capture runs on PRIVATE workspaces owned by this object (the engines' own grow-only buffers are
        # put back afterwards and may be reallocated by later eager calls with larger batches without touching the graph);
        # the compacted upright copy is kept per stride by the codebook handle for its whole life.
        self._ws = (_Workspace(dev), _Workspace(dev))
        saved = (self.enc.ws, self.cb.ws)
        self.enc.ws, self.cb.ws = self._ws
        try:
            self._capture(torch, dev)
        finally:
            self.enc.ws, self.cb.ws = saved

    def _capture(self, torch, dev):
        with _on_device(dev):
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):                # warm-up: sizes the engines' workspaces outside the capture
                for _ in range(2):
                    self._query()
            torch.cuda.current_stream().wait_stream(side)
            self.enc.settle()
            self.enc._x3h_captured_slot = -1
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph):
                self.z, self.idx, self.score = self._query()
            # split-precision capture: the recorded forward owns a range-flag slot of its own, looked at after every replay
            self._owned_slot = self.enc._x3h_captured_slot
            self._x3h_slot = self._owned_slot if self.enc.x3h_fallback else -1

    def close(self):
        """Drop the graph and give the range-flag slot of a split-precision capture back to the encoder (64 per handle)."""
        self.graph = None
        slot, self._owned_slot = getattr(self, '_owned_slot', -1), -1
        self._x3h_slot = -1
        if slot >= 0 and getattr(self.enc, 'handle', None):
            _torch().cuda.synchronize(self.enc.device)          # (no replay may still be writing the flag)
            with _on_device(self.enc.device):
                _lib.check(self.enc.lib, self.enc.lib.aae_encoder_x3h_release_slot(self.enc.handle, int(slot), _stream_ptr(_torch())), 'aae_encoder_x3h_release_slot')

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _query(self):
        if self.topk == 1:                               # one C call: conv1 prepares the ticket words of the later launches
            return self.enc.encode_nn(self.cb, self.x, self.col_stride)
        z = self.enc.encode(self.x)
        idx, score = self.cb.nn(z, self.topk, self.col_stride)
        return z, idx, score

    def __call__(self, x):
        """x: [B,H,W,C] (or [H,W,C] when batch == 1) of the dtype given at construction, host or device.
        Returns (idx int64 [B,topk], cosine float32 [B,topk]) -- static device tensors."""
        torch = _torch()
        if isinstance(x, np.ndarray):
            x = torch.from_numpy(np.ascontiguousarray(x))
        if x.dim() == 3:
            x = x.unsqueeze(0)
        if tuple(x.shape) != tuple(self.x.shape):
            raise ValueError('captured for input shape %s, got %s' % (tuple(self.x.shape), tuple(x.shape)))
        if x.dtype != self.x.dtype:
            raise ValueError('captured for dtype %s, got %s' % (self.x.dtype, x.dtype))
        self.x.copy_(x, non_blocking=True)
        if self.eager:
            self.enc.encode_nn(self.cb, self.x, self.col_stride, out=(self.z, self.idx, self.score))
            if self.enc._x3h_pending:
                self.enc.settle()                # (split precision: the same checked result a replay gives)
            return self.idx, self.score
        self.graph.replay()
        if self._x3h_slot >= 0 and self.enc._x3h_poll([self._x3h_slot])[0]:
            # f32x3h replay that left the fp16 pair range (one host round trip per replay in this mode -- the price of a
            # checked result; exact-fp32 captures never get here): the same query again, eagerly, in exact fp32
            self.enc.x3h_fallbacks += 1
            mode = self.enc.options.get('precision', 0)
            self.enc.set_option('precision', 0)
            try:
                z, idx, score = self._query()
                self.z.copy_(z)
                self.idx.copy_(idx)
                self.score.copy_(score)
            finally:
                self.enc.set_option('precision', mode)
        return self.idx, self.score


class StreamingNearestNeighbour(object):
    """Host-resident crop batches -> (idx, score) with the H2D copy of batch i+1 overlapped with
    encode+scan of batch i: a ring of three device input buffers, a copy stream, event hand-offs.
    (Three, not two: in split-precision mode the range flag of batch i is only read when batch i's results are fetched,
    one iteration later, and a batch that left the fp16 pair range is then recomputed FROM ITS INPUT BUFFER -- which
    must not have been handed to the next upload by then.  With three buffers the buffer of batch i is recycled for
    batch i + 3, after batch i has been fetched and settled.)  The copy is
    issued straight from the caller's (pageable) array after the kernels of the previous batch
    have been queued -- the runtime's own bounce buffers move 12.6 MB in ~0.4 ms while the GPU is
    busy for ~8 ms; an extra staging copy into pinned memory measured 3.5x SLOWER end to end
    (host-side memcpy into pinned pages).  This is the PCIe-inclusive form of the hot path (the
    reference feeds NumPy arrays to session.run, codebook.py:63); batches already on the device
    should call the engines directly."""

    def __init__(self, encoder_engine, codebook_engine, batch, in_dtype='uint8', topk=1, col_stride=1):
        torch = _torch()
        self.enc, self.cb = encoder_engine, codebook_engine
        self.batch, self.topk, self.col_stride = int(batch), int(topk), int(col_stride)
        dt = torch.uint8 if in_dtype in ('uint8', torch.uint8) else torch.float32
        dev = encoder_engine.device
        shape = (self.batch,) + tuple(encoder_engine.cfg.shape)
        self.slots = 3
        self.dev = [torch.empty(shape, dtype=dt, device=dev) for _ in range(self.slots)]
        with _on_device(dev):
            self.copy_stream = torch.cuda.Stream()
            self.copied = [torch.cuda.Event() for _ in range(self.slots)]
            self.consumed = [torch.cuda.Event() for _ in range(self.slots)]

    def _upload(self, slot, x):
        torch = _torch()
        n = len(x)
        src = torch.from_numpy(np.ascontiguousarray(x)) if isinstance(x, np.ndarray) else x
        with torch.cuda.stream(self.copy_stream):
            self.copy_stream.wait_event(self.consumed[slot])       # the compute that last read this slot is done
            self.dev[slot][:n].copy_(src, non_blocking=True)
            self.copied[slot].record(self.copy_stream)
        return n

    def run(self, batches):
        """batches: iterable of host arrays [b,H,W,C] (b <= batch).  Yields (idx [b,topk] int64, score [b,topk]
        float32) as host arrays, in order."""
        torch = _torch()
        it = iter(batches)
        compute = torch.cuda.current_stream()
        pending = None
        slot = 0
        try:
            nxt = next(it)
        except StopIteration:
            return
        n = self._upload(slot, nxt)
        while True:
            compute.wait_event(self.copied[slot])
            if self.topk == 1:
                _, idx, score = self.enc.encode_nn(self.cb, self.dev[slot][:n], self.col_stride)
            else:
                zc = self.enc.encode(self.dev[slot][:n])
                self.enc.settle()                 # (split precision only) the scan below must read checked latents
                idx, score = self.cb.nn(zc, self.topk, self.col_stride)
            self.consumed[slot].record(compute)
            try:
                nxt = next(it)
            except StopIteration:
                nxt = None
            if nxt is not None:
                n_next = self._upload((slot + 1) % self.slots, nxt)  # overlaps the kernels just queued; that buffer's batch was fetched (and settled) an iteration ago
            if pending is not None:
                yield self._fetch(pending)
            pending = (idx, score)
            if nxt is None:
                break
            slot = (slot + 1) % self.slots
            n = n_next
        yield self._fetch(pending)

    def _fetch(self, pair):
        """(idx, score) to the host; the range flags of the split-precision forwards queued so far are read with them --
        an affected batch has been recomputed in place (exact fp32) when this returns."""
        idx, score = pair[0].cpu(), pair[1].cpu()
        if self.enc.settle():
            # recompute kernels were queued just now and read input buffers whose `consumed` events are older: no upload may
            # overtake them
            compute = _torch().cuda.current_stream()
            for ev in self.consumed:
                ev.record(compute)
            idx, score = pair[0].cpu(), pair[1].cpu()
        return idx.numpy(), score.numpy()
