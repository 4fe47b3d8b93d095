"""The cases of tests/golden/encoder_launch_labels.json and how one is replayed: shared by the recorder
(tests/golden/make_encoder_launch_labels.py, run on the commit BEFORE the per-class launch code got its form lists), by
tests/test_encoder_launch_labels.py (the two emulator builds of the working tree) and by tests/test_gpu_launch_forms.py (the
product half on the MI355X, where a form whose dynamic-LDS ceiling was not raised fails to launch).

A case is one forward of a tiny network under an ORDERED option list; its record is the complete sequence of (kernel label,
flops) of that forward -- or, in the product build, the code with which the build refuses one of the options.  Every encoder
case names its wavek_target_blocks (the planner's round size), so the plan is the same on the emulator's three compute units and
on the hardware's 256.  ARMS names every dispatch arm of the launch code with the build, the case and the label that show it was
taken: what a label cannot show (uint8 / fp32 input, dword staging, the load schedule) is in the case's definition."""
import ctypes
import re

import numpy as np

from augmentedautoencoder_amd import _lib
from augmentedautoencoder_amd.weights import (DecoderConfig, EncoderConfig, as_pointer_array, ordered_decoder_weight_arrays,
                                              ordered_weight_arrays)
from oracle import decoder_cpu as dref
from oracle import reference_cpu as ref
from oracle import synth

# (shape, filters, strides, kernel, latent, batch norm)
NETS = {
    'n16': ((16, 16, 3), [32, 64], [2, 2], 5, 128, False),
    'n32': ((32, 32, 3), [32, 64], [2, 2], 5, 128, False),
    'n32_wide': ((32, 32, 3), [32, 256], [2, 2], 5, 128, False),
    'n24_bn': ((24, 16, 3), [64, 512], [2, 2], 5, 128, True),
    'gray12': ((12, 12, 1), [160, 32], [1, 2], 5, 128, False),
    'n40_odd': ((40, 24, 3), [48, 32], [2, 2], 5, 20, True),
    'n10_generic': ((10, 14, 3), [24, 8], [2, 1], 3, 12, True),
    # five conv layers: conv2 ... conv4 carry the per-layer kernel tags 1 ... 3, conv5 (and the dense layer) tag 0
    'n16_five': ((16, 16, 3), [32, 64, 64, 32, 32], [2, 2, 2, 1, 1], 5, 128, False),
    'gray12_small': ((12, 12, 1), [32, 32], [2, 2], 5, 128, False),
    'n8_wide': ((8, 8, 3), [32, 256], [2, 2], 5, 128, False),
    # conv2 and conv3 256 wide, 3 x 3 kernels (a short K for the emulator; conv1 is then the generic kernel)
    'n16_256_k3': ((16, 16, 3), [32, 256, 256], [2, 2, 2], 3, 128, True),
    # every layer behind the first 256 wide: the 128 x 256 and 256 x 256 block tiles for tags 1 ... 3
    'n16_256': ((16, 16, 3), [32, 256, 256, 256], [2, 2, 2, 1], 5, 128, True),
    # the Winograd nets of test_emu_winograd.py: regions of one image (conv2) and four images per block (conv3)
    'wino64_bn': ((64, 64, 3), [32, 64, 64], [2, 2, 2], 5, 128, True),
    # the persistent per-detection launch's four shape sequences (test_emu_kernels.py: _CHAIN_CASES)
    'chain_000': ((16, 16, 3), [32, 64, 64, 64], [2, 2, 2, 1], 5, 128, True),
    'chain_100': ((16, 16, 3), [32, 256, 64, 64], [2, 2, 2, 1], 5, 128, True),
    'chain_010': ((16, 16, 3), [32, 64, 256, 64], [2, 2, 2, 1], 5, 128, True),
    'chain_210': ((16, 16, 3), [32, 384, 256, 64], [2, 2, 2, 1], 5, 128, True),
}

ROUND = ('wavek_target_blocks', 256)
# the 128 x 128 igemm for small batches too, thresholds instead of the cost model (test_emu_kernels.py: _run)
IGEMM = [ROUND, ('wavek', 0), ('wavek_dense', 0), ('first_group_split_max_tiles', 0), ('planner_cost_model', 0)]
UNSPLIT = IGEMM + [('splitk_min_base_blocks', 0), ('dense_gemv', 0)]
# wave-split-K with the tile shape steered through the thresholds; the dense layer on the same kernel (tag 0)
WAVEK = [ROUND, ('planner_cost_model', 0), ('wavek_balance', 0), ('dense_gemv', 0)]
SHAPE_64x64 = [('wavek_tiny_max_tiles', 0), ('wavek_narrow_max_tiles', 0)]
SHAPE_64x32 = [('wavek_tiny_max_tiles', 0)]
X3H = [ROUND, ('precision', 1)]
CHAIN = [ROUND, ('wavek_balance', 0), ('planner_cost_batch3', 0)]
CHAIN_NARROW = [('wavek_tiny_max_tiles', 2), ('wavek_narrow_max_tiles', 128)]
WINO = [ROUND, ('winograd_min_batch', 1), ('winograd_min_blocks', 1)]


def _case(name, net, B, options, f32_in=False, seed=1, slow=False):
    return {'name': name, 'net': net, 'B': B, 'f32_in': f32_in, 'seed': seed, 'slow': slow, 'options': [list(o) for o in options]}


def cases():
    out = [
        # ---- conv_igemm_f32_kernel
        _case('igemm_splitk', 'n16', 3, IGEMM),
        _case('igemm_splitk_register_staged', 'n16', 3, IGEMM + [('igemm_dma', 0)]),
        _case('igemm_breg_tags', 'n16_five', 2, UNSPLIT + [('igemm_breg_min_blocks', 1)]),          # (the 32 KB footprint)
        _case('igemm_breg_large_footprint', 'n32', 5, UNSPLIT),
        _case('igemm_breg_n256', 'n16_256_k3', 1, UNSPLIT + [('igemm_breg_wide_min_blocks', 1)]),
        _case('igemm_dma_tags', 'n16_five', 2, UNSPLIT + [('igemm_breg', 0)]),
        _case('igemm_register_staged', 'n16', 2, UNSPLIT + [('igemm_dma', 0)]),
        # ---- conv_wavek_f32_kernel: 1000 * (32-row tile) + 100 * NT + 10 * waves + depth
        _case('wavek_242', 'n16_five', 3, WAVEK + SHAPE_64x64),
        _case('wavek_142', 'n16', 3, WAVEK + SHAPE_64x32),
        _case('wavek_1142', 'n16', 3, WAVEK),
        _case('wavek_242_burst', 'n16', 3, WAVEK + SHAPE_64x64 + [('wavek_spread', 0)]),
        _case('wavek_1142_burst', 'n16', 3, WAVEK + [('wavek_spread', 0)]),
        _case('wavek_243', 'n16', 3, WAVEK + SHAPE_64x64 + [('wavek_depth', 3)]),
        _case('wavek_143', 'n16', 3, WAVEK + SHAPE_64x32 + [('wavek_depth', 3)]),
        _case('wavek_1143', 'n16', 3, WAVEK + [('wavek_depth', 3)]),
        _case('wavek_282', 'n16', 3, WAVEK + SHAPE_64x64 + [('wavek_waves', 8)]),
        _case('wavek_182', 'n16', 3, WAVEK + SHAPE_64x32 + [('wavek_waves', 8)]),
        _case('wavek_1182', 'n16', 3, WAVEK + [('wavek_tiny_waves', 8)]),
        _case('wavek_tail_cut', 'n32', 5, [('wavek_target_blocks', 4), ('planner_cost_model', 0), ('wavek_balance', 0)] + SHAPE_64x64 +
              [('wavek_force_tail_tiles', 3), ('wavek_force_tail_g', 2)]),
        _case('wavek_by_cost_mid_batch', 'n32_wide', 5, [ROUND]),
        # ---- conv_igemm_x3h_kernel / _dma_kernel / _wide_kernel
        _case('x3h_splitk', 'n16', 3, X3H),
        _case('x3h_unsplit_tags', 'n16_five', 2, X3H + [('splitk_min_base_blocks', 0)]),
        _case('x3h_wide256', 'n8_wide', 1, X3H + [('splitk_min_base_blocks', 0), ('x3h_wide256_min_blocks', 1)]),
        # (three 256 x 256 x 6400 tiles in three fp16 products each: most of a minute on the emulator, microseconds on the hardware)
        _case('x3h_wide256_tags', 'n16_256', 1, X3H + [('splitk_min_base_blocks', 0), ('x3h_wide256_min_blocks', 1)], slow=True),
        _case('x3h_dma256', 'n16', 2, X3H + [('splitk_min_base_blocks', 0), ('x3h_wide_min_blocks', 1)]),
        _case('x3h_register_staged', 'n16', 2, X3H + [('splitk_min_base_blocks', 0), ('x3h_dma', 0)]),
        _case('x3h_splitk_register_staged', 'n16', 3, X3H + [('x3h_dma', 0)]),
        # ---- conv_direct_generic_kernel
        _case('generic_u8', 'n10_generic', 2, [ROUND]),
        _case('generic_f32', 'n10_generic', 2, [ROUND], f32_in=True),
        _case('generic_second_layer', 'n40_odd', 2, [ROUND], f32_in=True),
        # ---- dense_gemv_f32_kernel
        _case('gemv_two_launches', 'n16', 2, [ROUND, ('gemv_ticket', 0)]),
        _case('gemv_ticket_mq8', 'n24_bn', 7, [ROUND]),
        # ---- conv_wino_layer_kernel (aae_wino_launch.h) / conv_wino_phase_kernel
        _case('winograd_layer', 'wino64_bn', 3, WINO),
        _case('winograd_phases', 'wino64_bn', 3, WINO + [('winograd', 2)]),
    ]
    out += [_case('gemv_ticket_mq%d' % B, 'n16', B, [ROUND]) for B in (1, 2, 3, 4)]
    # ---- conv_first_f32_kernel: (3 | 1 channels) x (dword | byte | fp32 staging) x (group split | fp16 planes | plain)
    for net, ch in (('n16', 3), ('gray12_small', 1)):
        for staging, opts, f32 in (('vec4', [], False), ('u8', [('first_vec4', 0)], False), ('f32', [], True)):
            out.append(_case('first_c%d_%s_group_split' % (ch, staging), net, 2, [ROUND] + opts, f32_in=f32))
            out.append(_case('first_c%d_%s_planes' % (ch, staging), net, 2, X3H + opts, f32_in=f32))
            out.append(_case('first_c%d_%s_plain' % (ch, staging), net, 2, [ROUND, ('first_group_split_max_tiles', 0)] + opts, f32_in=f32))
    out.append(_case('first_gray_stride1_two_channel_blocks', 'gray12', 1, [ROUND]))
    # ---- detect_chain_kernel
    for shapes, B, narrow in (('000', 1, []), ('100', 2, CHAIN_NARROW), ('010', 3, CHAIN_NARROW),
                              ('210', 4, [('wavek_tiny_max_tiles', 2), ('wavek_narrow_max_tiles', 4)])):
        out.append(_case('chain_' + shapes, 'chain_' + shapes, B, CHAIN + narrow + [('detect_chain_blocks', 3), ('detect_chain', 1)], seed=31))
    return out


def decoder_cases():
    # (test_decoder_emu.py): phase-folded upconv on the matrix cores + the narrow output layer; the direct fallback; a stride-1 stage as a plain igemm
    return [{'name': 'decoder_phased_and_narrow', 'B': 2, 'seed': 3, 'config': dict(shape=[16, 16, 3], num_filter=[32, 64], strides=[2, 2])},
            {'name': 'decoder_direct', 'B': 2, 'seed': 9, 'config': dict(shape=[12, 12, 2], num_filter=[8, 24], strides=[3, 1], latent_space_size=20)},
            {'name': 'decoder_plain_igemm_stage', 'B': 1, 'seed': 11, 'config': dict(shape=[8, 8, 3], num_filter=[32, 32, 64], strides=[2, 1, 2])}]


E, P = 'experiments', 'product'
BOTH = (E, P)
# arm -> (builds whose record must show it, case, regular expression one label of the case's sequence matches)
ARMS = {
    'igemm split-K with LDS-DMA + reduce': (BOTH, 'igemm_splitk', r'^conv2:conv_igemm_f32_dma_splitk\d+ '),
    'igemm split-K reduce tail': (BOTH, 'igemm_splitk', r'^conv2:splitk_reduce$'),
    'igemm split-K register-staged': ((E,), 'igemm_splitk_register_staged', r'^conv2:conv_igemm_f32_splitk\d+ '),
    'igemm unsplit tag 0': (BOTH, 'igemm_breg_tags', r'^conv5:conv_igemm_f32_dma M='),
    'igemm unsplit tag 0 (dense)': (BOTH, 'igemm_breg_tags', r'^dense:conv_igemm_f32_dma M='),
    'igemm BREG tag 1': (BOTH, 'igemm_breg_tags', r'^conv2:conv_igemm_f32_dma_breg M='),
    'igemm BREG tag 2': (BOTH, 'igemm_breg_tags', r'^conv3:conv_igemm_f32_dma_breg M='),
    'igemm BREG tag 3': (BOTH, 'igemm_breg_tags', r'^conv4:conv_igemm_f32_dma_breg M='),
    'igemm BREG n256 tag 1': (BOTH, 'igemm_breg_n256', r'^conv2:conv_igemm_f32_dma_breg_n256 '),
    'igemm BREG n256 tag 2': (BOTH, 'igemm_breg_n256', r'^conv3:conv_igemm_f32_dma_breg_n256 '),
    'igemm DMA without BREG tag 1': ((E,), 'igemm_dma_tags', r'^conv2:conv_igemm_f32_dma M='),
    'igemm DMA without BREG tag 2': ((E,), 'igemm_dma_tags', r'^conv3:conv_igemm_f32_dma M='),
    'igemm DMA without BREG tag 3': ((E,), 'igemm_dma_tags', r'^conv4:conv_igemm_f32_dma M='),
    'igemm register-staged': ((E,), 'igemm_register_staged', r'^conv2:conv_igemm_f32 M='),
    'wave-split-K 242': (BOTH, 'wavek_242', r'^conv2:conv_wavek_f32_64x64_w4_d2_'),
    'wave-split-K 142': (BOTH, 'wavek_142', r'^conv2:conv_wavek_f32_64x32_w4_d2_'),
    'wave-split-K 1142': (BOTH, 'wavek_1142', r'^conv2:conv_wavek_f32_32x32_w4_d2_'),
    'wave-split-K 242 burst': ((E,), 'wavek_242_burst', r'^conv2:conv_wavek_f32_64x64_w4_d2_'),
    'wave-split-K 1142 burst': ((E,), 'wavek_1142_burst', r'^conv2:conv_wavek_f32_32x32_w4_d2_'),
    'wave-split-K 243': ((E,), 'wavek_243', r'^conv2:conv_wavek_f32_64x64_w4_d3_'),
    'wave-split-K 143': ((E,), 'wavek_143', r'^conv2:conv_wavek_f32_64x32_w4_d3_'),
    'wave-split-K 1143': ((E,), 'wavek_1143', r'^conv2:conv_wavek_f32_32x32_w4_d3_'),
    'wave-split-K 282': ((E,), 'wavek_282', r'^conv2:conv_wavek_f32_64x64_w8_d2_'),
    'wave-split-K 182': ((E,), 'wavek_182', r'^conv2:conv_wavek_f32_64x32_w8_d2_'),
    'wave-split-K 1182': ((E,), 'wavek_1182', r'^conv2:conv_wavek_f32_32x32_w8_d2_'),
    'wave-split-K tags 2, 3 and 0': (BOTH, 'wavek_242', r'^conv3:conv_wavek_f32_[\s\S]*\|conv4:conv_wavek_f32_[\s\S]*\|conv5:conv_wavek_f32_[\s\S]*\|dense:conv_wavek_f32_'),
    'wave-split-K tail cut': (BOTH, 'wavek_tail_cut', r'^conv2:conv_wavek_f32_64x64_w4_d2_g1t\d+x2 '),
    'f32x3h wide256 tag 1': (BOTH, 'x3h_wide256', r'^conv2:conv_igemm_x3h_wide256 '),
    'f32x3h wide256 tag 2': (BOTH, 'x3h_wide256_tags', r'^conv3:conv_igemm_x3h_wide256 '),
    'f32x3h wide256 tag 3': (BOTH, 'x3h_wide256_tags', r'^conv4:conv_igemm_x3h_wide256 '),
    'f32x3h 256 x 128': ((E,), 'x3h_dma256', r'^conv2:conv_igemm_x3h_dma256 '),
    'f32x3h DMA unsplit, fp32 out': (BOTH, 'x3h_unsplit_tags', r'^dense:conv_igemm_x3h_dma M='),
    'f32x3h DMA unsplit, planes tag 0': (BOTH, 'x3h_unsplit_tags', r'^conv5:conv_igemm_x3h_dma M='),
    'f32x3h DMA unsplit, planes tag 1': (BOTH, 'x3h_unsplit_tags', r'^conv2:conv_igemm_x3h_dma M='),
    'f32x3h DMA unsplit, planes tag 2': (BOTH, 'x3h_unsplit_tags', r'^conv3:conv_igemm_x3h_dma M='),
    'f32x3h DMA unsplit, planes tag 3': (BOTH, 'x3h_unsplit_tags', r'^conv4:conv_igemm_x3h_dma M='),
    'f32x3h register-staged, planes': ((E,), 'x3h_register_staged', r'^conv2:conv_igemm_x3h M='),
    'f32x3h register-staged, fp32 out': ((E,), 'x3h_register_staged', r'^dense:conv_igemm_x3h M='),
    'f32x3h split-K': (BOTH, 'x3h_splitk', r'^conv2:conv_igemm_x3h_dma_splitk\d+ [^|]*\|conv2:splitk_reduce'),
    'f32x3h split-K register-staged': ((E,), 'x3h_splitk_register_staged', r'^conv2:conv_igemm_x3h_splitk\d+ [^|]*\|conv2:splitk_reduce'),
    'generic kernel, uint8 input': (BOTH, 'generic_u8', r'^conv1:conv_direct_generic$'),
    'generic kernel, fp32 input': (BOTH, 'generic_f32', r'^conv1:conv_direct_generic$'),
    'two-launch GEMV + reduce tail': ((E,), 'gemv_two_launches', r'^dense:dense_gemv_f32 chunks=[^|]*\|dense:splitk_reduce$'),
    'Winograd layer launch': (BOTH, 'winograd_layer', r'^conv2:conv_wino_f32 layer [^|]*\|conv3:conv_wino_f32 layer '),
    'Winograd per-phase launches, regions of one image': ((E,), 'winograd_phases', r'^conv2:conv_wino_f32 phase 11 [^|]*\|conv2:conv_wino_f32 phase 10 [^|]*\|conv2:conv_wino_f32 phase 01 [^|]*\|conv2:conv_wino_f32 phase 00 '),
    'Winograd per-phase launches, four images per block': ((E,), 'winograd_phases', r'^conv3:conv_wino_f32 phase 11 [^|]*\|conv3:conv_wino_f32 phase 10 [^|]*\|conv3:conv_wino_f32 phase 01 [^|]*\|conv3:conv_wino_f32 phase 00 '),
    'decoder: phase-folded upconv igemm': (BOTH, 'decoder_phased_and_narrow', r'^up1:upconv2x_igemm_f32_dma 4 phases '),
    'decoder: narrow output layer': (BOTH, 'decoder_phased_and_narrow', r'^up\d:upconv2x_narrow '),
    'decoder: direct upconv': (BOTH, 'decoder_direct', r'^up\d:upconv_direct$'),
    'decoder: plain igemm stage': (BOTH, 'decoder_plain_igemm_stage', r'^up2:conv_igemm_f32'),
}
ARMS.update({'ticketed GEMV MQ %d' % mq: (BOTH, 'gemv_ticket_mq%d' % mq, r'^dense:dense_gemv_f32_ticket chunks=\d+ M=%d ' % B)
             for mq, B in ((1, 1), (2, 2), (3, 3), (4, 4), (8, 7))})
ARMS.update({'conv1 %d-channel %s %s' % (ch, staging, form): (BOTH, 'first_c%d_%s_%s' % (ch, staging, form.replace(' ', '_')),
                                                            r'^conv1:conv_first_f32_g4 ' if form == 'group split' else r'^conv1:conv_first_f32 ')
             for ch in (3, 1) for staging in ('vec4', 'u8', 'f32') for form in ('group split', 'planes', 'plain')})
ARMS.update({'chain variant ' + s: ((E,), 'chain_' + s, r'^chain:detect_chain_f32 B=\d blocks=3 shapes=%s phases=conv2\.\.conv4\+dense$' % s)
             for s in ('000', '100', '010', '210')})


def arm_reached(pattern, records):
    """does a label of the sequence match -- or, for a pattern that spans labels (it names the separator), the sequence joined with '|' from some label on?"""
    labels = [r[0] for r in records]
    if r'\|' not in pattern:
        return any(re.search(pattern, l) for l in labels)
    return any(re.search(pattern, '|'.join(labels[i:])) for i in range(len(labels)))


# ---------------------------------------------------------------------------------------------------------------- inputs
def encoder_config(case):
    return EncoderConfig(*NETS[case['net']])


def encoder_weights(case):
    cfg = encoder_config(case)
    return synth.make_weights(seed=case['seed'], shape=cfg.shape, num_filter=cfg.num_filter, strides=cfg.strides, latent=cfg.latent_space_size,
                              batch_norm=cfg.batch_norm, kernel_size=cfg.kernel_size)


def encoder_input(case):
    """(what the forward gets, the uint8 crops it stands for)"""
    x = synth.make_crops(case['B'], seed=case['seed'] + 1, shape=encoder_config(case).shape)
    return (ref.input_to_float(x).astype(np.float32) if case['f32_in'] else x), x


def decoder_config(case):
    return DecoderConfig(**case['config'])


def decoder_weights(case):
    c = case['config']
    return dref.make_decoder_weights(seed=case['seed'], out_shape=tuple(c['shape']), num_filter=c['num_filter'], strides=c['strides'],
                                     kernel_size=c.get('kernel_size', 5), latent=c.get('latent_space_size', 128), batch_norm=c.get('batch_norm', False))


def decoder_input(case):
    return (np.random.default_rng(case['seed'] + 1).standard_normal((case['B'], decoder_config(case).latent_space_size)) * 0.5).astype(np.float32)


# ------------------------------------------------------------------------------------------------ replay on an emulator build
def _aligned(nbytes, align=256):
    raw = np.full(nbytes + align, 0xA5, dtype=np.uint8)
    off = (-raw.ctypes.data) % align
    return raw[off:off + nbytes]


def _records(label, flops, h):
    out, i = [], 0
    while True:
        s = label(h, i)
        if not s:
            return out
        out.append([s.decode(), float(flops(h, i))])
        i += 1


def replay(L, case):
    """encoder case -> {'records': [[label, flops], ...]} or {'refused': [option, code]} on the library L (an _lib.declare'd emulator build)"""
    cfg = encoder_config(case)
    arrays = ordered_weight_arrays(encoder_weights(case), cfg)
    desc = cfg.to_desc()
    h = ctypes.c_void_p()
    _lib.check(L, L.aae_encoder_create(ctypes.byref(desc), as_pointer_array(arrays), len(arrays), ctypes.byref(h)), 'aae_encoder_create')
    try:
        for name, value in case['options']:
            rc = L.aae_encoder_set_option(h, name.encode(), int(value))
            if rc:
                return {'refused': [name, rc]}
        x = np.ascontiguousarray(encoder_input(case)[0])
        B = x.shape[0]
        n = L.aae_encoder_workspace_bytes(h, B)
        ws = _aligned(n)
        z = np.zeros((B, cfg.latent_space_size), dtype=np.float32)
        dt = _lib.AAE_DTYPE_U8 if x.dtype == np.uint8 else _lib.AAE_DTYPE_F32
        _lib.check(L, L.aae_encoder_forward(h, x.ctypes.data, dt, B, z.ctypes.data, ws.ctypes.data, n, None), case['name'])
        return {'records': _records(L.aae_encoder_kernel_label, L.aae_encoder_kernel_flops, h)}
    finally:
        L.aae_encoder_destroy(h)


def replay_decoder(L, case):
    cfg = decoder_config(case)
    arrays = ordered_decoder_weight_arrays(decoder_weights(case), cfg)
    desc = cfg.to_desc()
    h = ctypes.c_void_p()
    _lib.check(L, L.aae_decoder_create(ctypes.byref(desc), as_pointer_array(arrays), len(arrays), ctypes.byref(h)), 'aae_decoder_create')
    try:
        z = decoder_input(case)
        B = z.shape[0]
        n = L.aae_decoder_workspace_bytes(h, B)
        ws = _aligned(n)
        out = np.zeros((B,) + tuple(cfg.shape), dtype=np.float32)
        _lib.check(L, L.aae_decoder_forward(h, z.ctypes.data, B, out.ctypes.data, ws.ctypes.data, n, None), case['name'])
        return {'records': _records(L.aae_decoder_kernel_label, L.aae_decoder_kernel_flops, h)}
    finally:
        L.aae_decoder_destroy(h)


def replay_all(L):
    return {'encoder': [replay(L, c) for c in cases()], 'decoder': [replay_decoder(L, c) for c in decoder_cases()]}
