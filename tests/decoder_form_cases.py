"""The launch forms of the decoder (aae_decoder_*: aae_decoder_impl.h, kernels/decoder_f32.h, the SCATTER mode of
conv_igemm_f32_kernel) at ragged and tiny sizes: one table, run on the CPU fiber emulator (tests/test_emu_decoder_forms.py:
the host branches of aae_decoder_create / launch_stage / plan_decoder_workspace, the labels, the values) and on the MI355X
(tests/test_gpu_decoder_forms.py: what the emulator cannot see -- the bounds-checked buffer views and the LDS DMA of the
phased igemm at these geometries, the raised LDS ceiling of the narrow kernel, its scalar weight loads).

The table is written in DECODER order (first stage first), the way aae_decoder_create walks the network; DecoderConfig and
oracle.decoder_cpu.make_decoder_weights take filters and strides in encoder order -- _encoder_order() below is the one place
that turns them round (mixing the two silently turns an igemm case into a direct-kernel case: Cin stops being a multiple
of 32).  dims[i] = int(out / prod(S[i:])); the dense layer gives dims[0] x F[0], stage i (up<i>) resizes dims[i-1] -> dims[i]
(the last one -> out) and convolves F[i-1] -> F[i] (the last one -> the image channels).

A case states every launch it expects, in order: the label's prefix and the numbers the label carries (M= N= K=, px= Cin=
Cout= taps=).  run_case() asserts them, so a case cannot drift to another form unnoticed.  The split count of a split-K
launch is stated only where the case is about it.

Checked per case, on both backends, with the output handed in full of NaN and the workspace full of 0xA5: shape and no
NaN (an unwritten pixel of a partial tile), |x - x64| <= OUT_TOL for EVERY batch row, every hidden activation within the
backend's bound of that stage's fp64 maximum (what localises a wrong stage: the final sigmoid hides a lot), a second call
on the same handle with the same bits (nothing in these forms is atomic), the labels.

Bounds: the project's own.  Output 2e-6 absolute (tests/test_gpu_decoder.py, tests/test_decoder_emu.py); hidden activations
5e-6 of the stage maximum on the emulator (tests/test_decoder_emu.py: -ffp-contract=off, k-ordered sums) and 2e-5 on the
GPU (tests/test_gpu_decoder.py: fp32 accumulation over K up to 12 800 there, at most 1600 here)."""
import collections
import ctypes
import functools
import re

import numpy as np

from augmentedautoencoder_amd.weights import DecoderConfig
from oracle import decoder_cpu as dref

OUT_TOL = 2e-6
HIDDEN_TOL_EMU = 5e-6
HIDDEN_TOL_GPU = 2e-5

PLAIN, PHASED, NARROW, DIRECT = 'plain', 'phased', 'narrow', 'direct'             # StageMode of aae_decoder_impl.h
STAGE_MODES = (PLAIN, PHASED, NARROW, DIRECT)
D_SPLIT, D_UNSPLIT, D_GENERIC = 'split', 'unsplit', 'generic'                        # the dense layer's three launches

Case = collections.namedtuple('Case', 'name out F S k bn latent B dense stages launches gpu_only seed')


# ---- the expected launches ------------------------------------------------------------------------------------------------------
def _igemm(name, M, N, K, split):
    """launch_igemm: split == False: one launch; True: split-K + reduce, any split count; an int: exactly that many"""
    if split is False:
        return [('%s:conv_igemm_f32_dma ' % name, dict(M=M, N=N, K=K))]
    prefix = '%s:conv_igemm_f32_dma_splitk' % name + ('' if split is True else '%d ' % split)
    return [(prefix, dict(M=M, N=N, K=K)), ('%s:splitk_reduce' % name, {})]


def dense(M, N, K, split=True):
    return (D_SPLIT if split else D_UNSPLIT), _igemm('dense', M, N, K, split)


def dense_generic():
    return D_GENERIC, [('dense:conv_direct_generic', {})]


def plain(M, N, K, split=True):
    return PLAIN, lambda name: _igemm(name, M, N, K, split)


def phased(M, N, K):
    return PHASED, lambda name: [('%s:upconv2x_igemm_f32_dma 4 phases x ' % name, dict(M=M, N=N, K=K))]


def narrow(px, Cin, Cout, taps):
    return NARROW, lambda name: [('%s:upconv2x_narrow ' % name, dict(px=px, Cin=Cin, Cout=Cout, taps='%dx%d' % (taps, taps)))]


def direct():
    return DIRECT, lambda name: [('%s:upconv_direct' % name, {})]


def _case(name, out, F, S, B, dense_form, stage_forms, k=5, bn=False, latent=128, gpu_only=False, seed=0):
    assert len(F) == len(S) == len(stage_forms), name
    launches = list(dense_form[1])
    for i, (_, make) in enumerate(stage_forms):
        launches += make('up%d' % (i + 1))
    return Case(name, tuple(out), tuple(F), tuple(S), k, bn, latent, B, dense_form[0], tuple(m for m, _ in stage_forms), tuple(launches), gpu_only,
                seed or 1000 + sum(ord(ch) for ch in name))


def cases():
    """Sizes: the smallest that still reach the form.  Taps per axis of a phase problem: k = 1: 1, 3: 2, 5: 3, 7: 4, 9: 5,
    11: 6; of the narrow kernel (the union over both parities): 3, 3, 3 ... k = 9: 5, k = 11: 7.  gpu_only: more than about
    ten seconds on the emulator."""
    out = [
        # up1: six M tiles, the last with 20 rows; up2: three 32-channel chunks, source 20 x 44 = 2 x 3 tiles, partial by 4 and 12
        _case('phased_ragged', (40, 88, 3), (32, 96), (2, 2), 3, dense(3, 7040, 128),
              [phased(660, 96, 288), narrow(2640, 96, 3, 3)]),
        # two N tiles, the second with 8 columns; 4 x 4 taps, the parities pad 2 and 1; last stage direct (Cin 136) with sigmoid, Cout 4
        _case('phased_two_ntiles', (20, 12, 4), (64, 136), (2, 2), 2, dense(2, 960, 128),
              [phased(30, 136, 1024), direct()], k=7),
        # one K slab, five columns; last stage direct (Cin 5)
        _case('phased_k1_cout5', (12, 20, 2), (32, 5), (2, 2), 2, dense(2, 480, 128),
              [phased(30, 5, 32), direct()], k=1),
        # a last stage with Cout > 4: sigmoid through the direct kernel at exact 2x
        _case('last_wide', (16, 16, 5), (32, 32), (2, 2), 2, dense(2, 512, 128),
              [phased(32, 32, 288), direct()]),
        # the narrow kernel as a hidden stage (ReLU), source 2 x 2; up2 has Cin 3
        _case('hidden_narrow', (16, 16, 3), (32, 3, 32), (2, 2, 2), 2, dense(2, 128, 128),
              [narrow(8, 32, 3, 3), direct(), narrow(128, 32, 3, 3)]),
        # ... and its neighbour with batch norm: the narrow kernel has none, up1 must be direct
        _case('hidden_narrow_bn', (16, 16, 3), (32, 4, 32), (2, 2, 2), 2, dense(2, 128, 128),
              [direct(), direct(), narrow(128, 32, 3, 3)], bn=True),
        # batch norm behind a phased stage, ragged M, 2 x 2 taps; last stage direct (Cin 40), one image channel
        _case('phased_bn_k3', (12, 20, 1), (32, 40), (2, 2), 3, dense(3, 480, 128),
              [phased(45, 40, 128), direct()], k=3, bn=True),
        # a stride-1 stage: plain igemm, split-K over 25 slabs, batch norm in the reduce tail; up2 direct (Cin 33); up3 narrow, two chunks
        _case('plain_splitk_bn', (12, 12, 3), (32, 33, 64), (1, 1, 2), 3, dense(3, 1152, 128),
              [plain(108, 33, 800), direct(), narrow(108, 64, 3, 3)], bn=True),
        # the partial buffer is shared by the dense layer (4 x 4 x 1152 floats) and up2 (50 x 576 x 32); up3: direct 1x with sigmoid
        _case('phased_then_plain', (12, 12, 3), (32, 64, 32), (2, 1, 1), 4, dense(4, 1152, 128),
              [phased(144, 64, 288), plain(576, 32, 1600), direct()]),
        # int(30 / 4) = 7: the direct kernel at the ratio 7 -> 15; the narrow kernel on a 15 x 15 source
        _case('ratio_7_15', (30, 30, 3), (32, 32), (2, 2), 2, dense(2, 1568, 128),
              [direct(), narrow(450, 32, 3, 3)]),
        _case('ratio_3', (27, 18, 3), (32, 32), (3, 3), 2, dense(2, 192, 128),
              [direct(), direct()]),
        # dense: two M tiles, the second with 2 rows; latent 96 = three slabs, one per split (up1: 2 x 3 -> 5 x 7, direct)
        _case('dense_two_mtiles', (10, 14, 3), (64, 32), (2, 2), 130, dense(130, 384, 96, split=3),
              [direct(), narrow(4550, 32, 3, 3)], latent=96),
        _case('dense_generic', (8, 8, 3), (32, 32), (2, 2), 2, dense_generic(),
              [phased(8, 32, 288), narrow(32, 32, 3, 3)], latent=33),
        _case('k9', (16, 16, 3), (32, 64), (2, 2), 1, dense(1, 512, 128),
              [phased(16, 64, 800), narrow(64, 64, 3, 5)], k=9),
        # 22 staged rows of 832 floats: 73 216 B of LDS, above the 64 KiB a kernel gets without asking
        _case('k11_lds', (16, 16, 3), (32, 64), (2, 2), 1, dense(1, 512, 128),
              [phased(16, 64, 1152), narrow(64, 64, 3, 7)], k=11),
        # dense: two splits over 65 536 outputs: the float4 reduce kernel (16 s per forward on the emulator: 512 dense blocks)
        _case('dense_small_reduce', (64, 64, 3), (128, 32), (2, 2), 2, dense(2, 32768, 128, split=2),
              [phased(512, 32, 512), narrow(2048, 32, 3, 3)], k=3, gpu_only=True),
        # dense: 2 x 192 = 384 base blocks, the un-split launch (16 x 16 x 96 = 192 x 128 columns: the first stage has stride 1;
        # up1: plain, 258 M tiles, two splits through the float4 reduce kernel)
        _case('dense_unsplit', (32, 32, 3), (96, 32), (1, 2), 129, dense(129, 24576, 128, split=False),
              [plain(33024, 32, 864, split=2), narrow(33024, 32, 3, 3)], k=3, gpu_only=True),
        # plain igemm with 384 M tiles: un-split, bias and ReLU in the igemm's own epilogue
        _case('plain_unsplit', (32, 32, 3), (32, 64, 32), (1, 1, 2), 192, dense(192, 8192, 128),
              [plain(49152, 64, 288, split=False), plain(49152, 32, 576, split=False), narrow(49152, 32, 3, 3)], k=3, gpu_only=True),
    ]
    names = [c.name for c in out]
    assert len(set(names)) == len(names), names
    return out


def case_id(c):
    return c.name


def check_coverage(cs):
    """what the table exists for; a case list that lost one of these fails at import"""
    assert {m for c in cs for m in c.stages} == set(STAGE_MODES), 'a StageMode is missing'
    assert {c.dense for c in cs} == {D_SPLIT, D_UNSPLIT, D_GENERIC}, 'a dense-layer launch is missing'
    hidden_bn = {m for c in cs if c.bn for m in c.stages[:-1]}                  # (the last stage has no batch norm)
    assert hidden_bn >= {PLAIN, PHASED, DIRECT}, 'batch norm is missing on %s' % sorted({PLAIN, PHASED, DIRECT} - hidden_bn)
    assert {c.k for c in cs} >= {1, 3, 5, 7, 9, 11} and 3 in {c.k for c in cs if not c.gpu_only}
    assert any(c.stages[-1] == DIRECT and c.out[2] > 4 for c in cs) and any(NARROW in c.stages[:-1] for c in cs)
    prefixes = {p for c in cs for p, _ in c.launches}
    assert any(re.match(r'up\d:conv_igemm_f32_dma $', p) for p in prefixes) and any(re.match(r'up\d:splitk_reduce$', p) for p in prefixes)


check_coverage(cases())


# ---- inputs --------------------------------------------------------------------------------------------------------------------
def _encoder_order(seq):
    """DecoderConfig and make_decoder_weights reverse what they are given: the ONE place the table's order is turned round"""
    return list(reversed(seq))


def config(c):
    return DecoderConfig(shape=c.out, num_filter=_encoder_order(c.F), strides=_encoder_order(c.S), kernel_size=c.k,
                         latent_space_size=c.latent, batch_norm=c.bn)


Inputs = collections.namedtuple('Inputs', 'cfg w z x64 acts64')


@functools.lru_cache(maxsize=None)
def build_inputs(name):
    """Weights, latent codes and the fp64 expectation of a case (computed once, shared by every test of the process, read-only).
    Asserts that the comparison cannot be empty: every hidden activation has a positive maximum and at least a tenth of its
    entries non-zero (a dead ReLU layer), the sigmoid output is unsaturated (0.01 < x < 0.99) on at least half the pixels."""
    c = {k.name: k for k in cases()}[name]
    cfg = config(c)
    assert cfg.num_filters == list(c.F) and cfg.strides == list(c.S), 'the table is in decoder order'
    w = dref.make_decoder_weights(seed=c.seed, out_shape=c.out, num_filter=_encoder_order(c.F), strides=_encoder_order(c.S),
                                  kernel_size=c.k, latent=c.latent, batch_norm=c.bn)
    z = np.random.default_rng(c.seed + 1).standard_normal((c.B, c.latent)).astype(np.float32)
    xs, acts = [], None
    for a in range(0, c.B, 16):                  # (the reference builds im2col matrices in fp64: 16 codes at a time bound its memory)
        x, act = dref.decoder_forward_np(z[a:a + 16], w, cfg.shape, cfg.num_filters, cfg.strides, cfg.batch_norm, return_activations=True)
        xs.append(x)
        acts = [[h] for h in act] if acts is None else [old + [h] for old, h in zip(acts, act)]
    x64 = np.concatenate(xs)
    acts64 = [np.concatenate(hs) for hs in acts]
    assert x64.shape == (c.B,) + c.out and len(acts64) == len(c.F)
    for i, h in enumerate(acts64):
        assert np.abs(h).max() > 0 and np.count_nonzero(h) >= h.size / 10.0, '%s: hidden activation %d is dead' % (name, i)
    assert np.count_nonzero((x64 > 0.01) & (x64 < 0.99)) >= x64.size / 2.0, '%s: the sigmoid output is saturated' % name
    for a in [z, x64] + acts64 + list(w.values()):
        a.setflags(write=False)
    return Inputs(cfg, w, z, x64, tuple(acts64))


# ---- the adapters over DecoderEngine / EmuDecoder --------------------------------------------------------------------------------
class GpuBackend(object):
    """engine.DecoderEngine: the output tensor arrives full of NaN (decode's out=), the workspace full of 0xA5"""
    hidden_tol = HIDDEN_TOL_GPU

    def create(self, cfg, w):
        from augmentedautoencoder_amd.engine import DecoderEngine
        return DecoderEngine(cfg, w)

    def forward(self, dec, z, dirty=True):
        import torch
        B = z.shape[0]
        if dirty:
            n = dec.lib.aae_decoder_workspace_bytes(dec.handle, B)
            dec.ws.get(n)[0].fill_(0xA5)         # (grown to the case's size first: the fill is of the buffer the call will use)
        out = torch.full((B,) + tuple(dec.cfg.shape), float('nan'), dtype=torch.float32, device=dec.device)
        got = dec.decode(np.array(z), out=out)        # (a copy: the shared inputs are read-only, torch wants a writable array)
        assert got is out
        return out.cpu().numpy()

    def activation(self, dec, i):
        return dec.activation(i).cpu().numpy()

    def labels(self, dec):
        out = []
        while True:
            s = dec.lib.aae_decoder_kernel_label(dec.handle, len(out))
            if not s:
                return out
            out.append(s.decode())


class EmuBackend(object):
    """emu_backend.EmuDecoder (or a subclass on another build of the emulator library): its forward() hands in a NaN output and
    a fresh 0xA5 workspace on every call"""
    hidden_tol = HIDDEN_TOL_EMU

    def __init__(self, decoder_class):
        self.decoder_class = decoder_class

    def create(self, cfg, w):
        return self.decoder_class(w, cfg)

    def forward(self, dec, z, dirty=True):
        return dec.forward(z)

    def activation(self, dec, i):
        return dec.activation(i)

    def labels(self, dec):
        return dec.labels()


_NUMBER = re.compile(r'(\w+)=(\d+x\d+|\d+)')


def check_labels(case, labels):
    assert len(labels) == len(case.launches), (labels, case.launches)
    for label, (prefix, numbers) in zip(labels, case.launches):
        assert label.startswith(prefix), (label, prefix)
        got = dict(_NUMBER.findall(label))
        for key, want in numbers.items():
            assert got.get(key) == str(want), (label, key, want)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def run_case(case, backend, dec=None):
    """One case on one backend; dec: a handle the caller keeps (else made and closed here).  Prints and returns
    (largest |x - x64|, largest hidden error relative to its stage's fp64 maximum)."""
    inp = build_inputs(case.name)
    own = dec is None
    if own:
        dec = backend.create(inp.cfg, inp.w)
    try:
        x = backend.forward(dec, inp.z)
        hidden = [backend.activation(dec, i) for i in range(len(inp.acts64))]
        labels = backend.labels(dec)
        out_err = float(np.abs(x - inp.x64).max()) if x.shape == inp.x64.shape and not np.isnan(x).any() else float('nan')
        rel = [float(np.abs(h - a).max() / np.abs(a).max()) if h.shape == a.shape else float('nan') for h, a in zip(hidden, inp.acts64)]
        print('%s: out err %.2e, hidden rel err %s, labels %s' % (case.name, out_err, ' '.join('%.2e' % r for r in rel), labels))
        assert x.shape == inp.x64.shape and x.dtype == np.float32
        assert not np.isnan(x).any(), 'unwritten output: %d elements, first at %s' % (np.isnan(x).sum(), np.argwhere(np.isnan(x))[0].tolist())
        for i, (h, a) in enumerate(zip(hidden, inp.acts64)):      # (before the output: the first wrong stage is the one reported)
            assert h.shape == a.shape, (i, h.shape, a.shape)
            assert np.isfinite(h).all(), 'stage %d: not finite' % i
            assert rel[i] <= backend.hidden_tol, 'stage %d (0 = dense) rel err %.2e, labels %s' % (i, rel[i], labels)
        per_row = np.abs(x - inp.x64).reshape(case.B, -1).max(axis=1)
        assert np.all(per_row <= OUT_TOL), ('output', int(np.argmax(per_row)), float(per_row.max()))
        x2 = backend.forward(dec, inp.z, dirty=False)
        assert np.array_equal(_bits(x), _bits(x2)), 'a second call on the same handle gives other bits'
        for i, h in enumerate(hidden):
            assert np.array_equal(_bits(h), _bits(backend.activation(dec, i))), 'stage %d: a second call gives other bits' % i
        check_labels(case, labels)
        return out_err, max(rel)
    finally:
        if own:
            dec.close()
