"""The Winograd layer kernel (csrc/kernels/conv_winograd_f32.h, launched by aae_encoder_launch.h: launch_winograd and aae_wino_launch.h) at the
shapes winograd_geometry() (aae_encoder_plan.h:98) accepts and no other test runs: non-square images (blocks_x != blocks_y), three
regions per image, region lists that leave XCD region groups empty or half full, 3 / 5 / 6 / 12 column blocks with every block order
they can take, an odd number of 32-channel stages, the four-image geometry at ragged batches, the BN epilogue -- and the layers next
to the eligibility edge, which must stay on the direct kernels.  One table, run on the CPU fiber emulator
(tests/test_emu_winograd_shapes.py: the host maps, the labels) and on the MI355X (tests/test_gpu_winograd_shapes.py: what the emulator
cannot see -- buffer-view reads outside the image, LDS-DMA, the packed-math asm, the XCD block order, the raised LDS ceilings of every
AAE_WINO_FORMS row).

A case is (name, shape, filters, strides, batch_norm, B, options, the layers expected in the Winograd form, gpu_only) plus the
winograd_xcd_cols values it must be bit-equal under and the lines of the table below it stands for.  Every case sets
winograd_min_batch = 1, winograd_min_blocks = 1 and wavek_target_blocks = 256: the plan is then the same on the emulator's three
compute units and on the hardware's 256.

run_case() checks, per case:
  a. exactly the expected layers carry 'conv_wino_f32 layer', with M = B Ho Wo, N = Cout, C = Cin;
  b. every layer, element by element, against the fp64 convolution of the backend's OWN input activation (upstream rounding is not
     charged to the layer): |got - want| <= ALLOWANCE u S, u = 2^-24, S = conv(|x|, |w|) + |b| (element_ratio below);
  c. the norms the project already uses (tests/test_gpu_parity.py: _check_layer; 5e-6 for the latent) against the whole-network oracle;
  d. the same bits under the four (winograd_static_halo, winograd_stage32) settings, under every listed winograd_xcd_cols, for a
     batch with its images permuted (a rotation by one: a derangement), and for every run given twice;
  e. GPU only: the same finite bits with the whole workspace buffer full of 0xFF (every float a NaN), 0x00 and 0xA5 before the call.

The bound of b is measured, not chosen: see ALLOWANCE."""
import collections
import functools
import re

import numpy as np

from augmentedautoencoder_amd.weights import EncoderConfig
from oracle import reference_cpu as ref
from oracle import synth

U = 2.0 ** -24

# The allowance of check b, in units of u S.  Yardstick: the float32 NumPy direct form of the same layer on the same inputs
# (ref.conv2d_same_relu_np(..., dtype=np.float32)) against its float64 twin -- yardstick_ratio() below; the code under test is not
# involved.  Its maximum over every conv layer of every case of this table is YARDSTICK_MAX (tests/test_wino_shape_checker.py:
# test_yardstick_passes_and_allowance_stays_below_the_direct_bound prints it per case; run of 2026-10-21, NumPy 2.2.6 on OpenBLAS 0.3.29,
# x86-64 with AVX-512: 5.956 at conv1 of bn_32x16_then_direct, 4.14 the largest of a second or third layer, 0.30 the smallest);
# the allowance is 4 x that, the factor tests/decoder_grad_reference.py allows over its float32 NumPy figure.  It stays far below the
# worst case (25 Cin + 8) u S of a direct sum (83 for conv1, 808 and more behind it), which would hide everything short of a dropped tap.
YARDSTICK_MAX = 5.956
ALLOWANCE = 4.0 * YARDSTICK_MAX

LAYER_TOL_MAX, LAYER_TOL_L2, LATENT_TOL = 2e-5, 1e-5, 5e-6       # tests/test_gpu_parity.py: _check_layer; tests/test_gpu_winograd.py (latent)

BASE_OPTIONS = {'winograd_min_batch': 1, 'winograd_min_blocks': 1, 'wavek_target_blocks': 256}
HALO_STAGE_SETTINGS = ((1, 1), (0, 1), (1, 0), (0, 0))          # (winograd_static_halo, winograd_stage32); the first is the default
WINO_FORMS = {(0, 16, False), (0, 32, False), (0, 16, True), (0, 32, True), (1, 16, True), (1, 32, True), (2, 16, False)}    # aae_wino_launch.h:21 AAE_WINO_FORMS

# the lines of the table ("Shapes pinned")
NON_SQUARE, ODD_REGIONS, RAGGED_GROUPS, NBN, XCD_COLS, ODD_STAGES, GEOM1, BN_MIXED, BN_SCALE, EDGE = (
    'blocks_x != blocks_y', 'odd region counts per image', 'region groups empty or ragged', 'nbn 3 5 6 12', 'winograd_xcd_cols',
    'odd stage counts', 'geometry 1', 'both geometries, BN epilogue', 'BN epilogue, non-trivial scale', 'eligibility edge')
TABLE_LINES = (NON_SQUARE, ODD_REGIONS, RAGGED_GROUPS, NBN, XCD_COLS, ODD_STAGES, GEOM1, BN_MIXED, BN_SCALE, EDGE)

Case = collections.namedtuple('Case', 'name shape filters strides bn B options wino gpu_only xcd lines seed')


def _case(name, shape, filters, B, wino, lines, strides=None, bn=False, xcd=(), gpu_only=False):
    strides = [2] * len(filters) if strides is None else strides
    return Case(name, tuple(shape), tuple(filters), tuple(strides), bn, B, dict(BASE_OPTIONS), tuple(wino), gpu_only, tuple(xcd), tuple(lines),
                2000 + sum(ord(ch) for ch in name))


def cases():
    """Sizes: the smallest that still reach the branch.  Cout >= 320 and the 16 x 32 output at Cout 192 get a third layer of 64 filters,
    so that the dense layer stays small (16 x 32 x 768 x 64 latent weights are 100 MB); behind a 16 x 16 output that layer is a
    Winograd layer of its own (8 x 8, Cin = the wide Cout: 10 ... 24 stages), behind 16 x 32 it is 8 x 16: direct.
    gpu_only: a minute and more on the emulator (each ran there once, bounds-checked, before its first GPU run)."""
    out = [
        # conv2 16 x 32: blocks_x = 2, blocks_y = 1; 2 / 6 / 10 regions over the 8 region groups of nbn = 1
        _case('wide_16x32_b1', (64, 128, 3), [32, 64], 1, ['conv2'], [NON_SQUARE]),
        _case('wide_16x32_b3', (64, 128, 3), [32, 64], 3, ['conv2'], [NON_SQUARE, RAGGED_GROUPS]),
        _case('wide_16x32_b5', (64, 128, 3), [32, 64], 5, ['conv2'], [NON_SQUARE, RAGGED_GROUPS]),
        # conv2 32 x 16: blocks_x = 1, blocks_y = 2
        _case('tall_32x16_b1', (128, 64, 3), [32, 64], 1, ['conv2'], [NON_SQUARE]),
        _case('tall_32x16_b3', (128, 64, 3), [32, 64], 3, ['conv2'], [NON_SQUARE, RAGGED_GROUPS]),
        # three regions per image (16 x 48: 1 x 3), six per image (48 x 32: 3 x 2)
        _case('wide_16x48_b2', (64, 192, 3), [32, 64], 2, ['conv2'], [NON_SQUARE, ODD_REGIONS, RAGGED_GROUPS]),
        _case('tall_48x32_b1', (192, 128, 3), [32, 64], 1, ['conv2'], [NON_SQUARE, ODD_REGIONS, RAGGED_GROUPS]),
        # nbn = 3: the default gives xcd_cols 3 (one column group, 8 region groups); 1 is invalid (3 column groups do not divide 8 XCDs): plain order
        _case('nbn3_16x16', (64, 64, 3), [32, 192], 2, ['conv2'], [NBN, XCD_COLS], xcd=(-1, 0, 1, 3)),
        _case('nbn3_16x32', (64, 128, 3), [32, 192, 64], 1, ['conv2'], [NBN, NON_SQUARE, XCD_COLS], xcd=(-1, 0, 1, 3), gpu_only=True),
        # nbn = 5: xcd_cols 5 only
        _case('nbn5_16x16', (64, 64, 3), [32, 320, 64], 1, ['conv2', 'conv3'], [NBN]),
        _case('nbn5_16x32', (64, 128, 3), [32, 320, 64], 2, ['conv2'], [NBN, NON_SQUARE], gpu_only=True),
        # nbn = 6: default 6 (one region: 6 live blocks of 48); 3 is valid (2 column groups x 4 region groups: one region leaves three groups empty, six fill
        # three and leave the fourth empty); 2 and 1 fall through to plain order
        _case('nbn6_16x16', (64, 64, 3), [32, 384, 64], 1, ['conv2', 'conv3'], [NBN, XCD_COLS, RAGGED_GROUPS], xcd=(-1, 0, 1, 2, 3)),
        _case('nbn6_16x32', (64, 128, 3), [32, 384, 64], 3, ['conv2'], [NBN, NON_SQUARE, XCD_COLS, RAGGED_GROUPS], xcd=(-1, 0, 1, 2, 3), gpu_only=True),
        # nbn = 12: the default starts at 4 and falls 4 -> 2 -> 1 -> 0: plain order
        _case('nbn12_16x16', (64, 64, 3), [32, 768, 64], 1, ['conv2', 'conv3'], [NBN], xcd=(-1, 0), gpu_only=True),
        _case('nbn12_16x32', (64, 128, 3), [32, 768, 64], 1, ['conv2'], [NBN, NON_SQUARE], xcd=(-1, 0), gpu_only=True),
        # three and five 32-channel stages (six and ten of 16 channels), both geometries
        _case('cin96_16x16', (64, 64, 3), [96, 64], 2, ['conv2'], [ODD_STAGES]),
        _case('cin160_16x16', (64, 64, 3), [160, 64], 1, ['conv2'], [ODD_STAGES]),
        _case('cin96_8x8', (32, 32, 3), [96, 64], 3, ['conv2'], [ODD_STAGES, GEOM1]),
        _case('cin160_8x8', (32, 32, 3), [160, 64], 5, ['conv2'], [ODD_STAGES, GEOM1]),
        # geometry 1: one image, three (one block with an empty slot), four (a whole block), five and nine (a block with ONE image)
        _case('geom1_b1', (32, 32, 3), [32, 64], 1, ['conv2'], [GEOM1]),
        _case('geom1_b3', (32, 32, 3), [32, 64], 3, ['conv2'], [GEOM1]),
        _case('geom1_b4', (32, 32, 3), [32, 64], 4, ['conv2'], [GEOM1]),
        _case('geom1_b5', (32, 32, 3), [32, 64], 5, ['conv2'], [GEOM1]),
        _case('geom1_b9', (32, 32, 3), [32, 64], 9, ['conv2'], [GEOM1], xcd=(-1, 0)),
        _case('geom1_nbn3_b5', (32, 32, 3), [32, 192], 5, ['conv2'], [GEOM1, NBN, XCD_COLS], xcd=(-1, 0, 1, 3)),
        # BN epilogue: conv2 32 x 16 (Winograd), conv3 16 x 8 (ineligible: direct)
        _case('bn_32x16_then_direct', (128, 64, 3), [32, 64, 64], 2, ['conv2'], [BN_MIXED, NON_SQUARE], bn=True),
        # BN epilogue on both geometries: conv2 16 x 16 with nbn 3, conv3 8 x 8 with Cin 192
        _case('bn_nbn3_then_geom1', (64, 64, 3), [96, 192, 64], 2, ['conv2', 'conv3'], [BN_SCALE, NBN, ODD_STAGES, GEOM1], bn=True),
        # the eligibility edge: no Winograd label
        _case('edge_8x16', (32, 64, 3), [32, 64], 2, [], [EDGE]),
        _case('edge_16x8', (64, 32, 3), [32, 64], 2, [], [EDGE]),
        _case('edge_24x24', (96, 96, 3), [32, 64], 1, [], [EDGE]),
        _case('edge_stride1_third', (64, 64, 3), [32, 64, 64], 1, ['conv2'], [EDGE], strides=[2, 2, 1]),
    ]
    names = [c.name for c in out]
    assert len(set(names)) == len(names), names
    return out


def case_id(c):
    return c.name


def config(c):
    return EncoderConfig(c.shape, list(c.filters), list(c.strides), 5, 64, c.bn)


# ---- the host rules, restated ----------------------------------------------------------------------------------------------------
def winograd_geometry(layer, shape, stride, kernel=5):
    """aae_encoder_plan.h:98 winograd_geometry: 0 = 16 x 16-pixel regions of one image, 1 = four 8 x 8 images per block, -1 = not eligible"""
    H, W, Cin, Ho, Wo, Cout = shape
    if layer < 1 or kernel != 5 or stride != 2 or H % 2 or W % 2 or H != 2 * Ho or W != 2 * Wo:
        return -1
    if Cin % 32 or Cout % 64:
        return -1
    if Ho % 16 == 0 and Wo % 16 == 0:
        return 0
    return 1 if (Ho, Wo) == (8, 8) else -1


def layer_static_halo(geom, blocks_x, blocks_y, option):
    """conv_winograd_f32.h:197 wino_layer_static_halo"""
    return bool(option) and (geom != 0 or (blocks_x == 1 and blocks_y == 1))


def layer_geom_tag(geom, static_halo):
    """conv_winograd_f32.h:194 wino_layer_geom_tag"""
    return 0 if geom == 0 else (1 if static_halo else 2)


def layer_stage_channels(geom, Cin, stage32, static_halo):
    """conv_winograd_f32.h:198 wino_layer_stage_channels"""
    return 32 if stage32 and (geom == 0 or static_halo) and Cin % 32 == 0 else 16


def xcd_cols(nbn, option):
    """aae_encoder_launch.h:581 wino_xcd_cols with conv_winograd_f32.h:75 wino_xcd_cols_valid"""
    s = option
    if s < 0:
        s = 4 if nbn >= 8 else nbn
    while s > 0 and not (nbn % s == 0 and nbn // s <= 8 and 8 % (nbn // s) == 0):
        s >>= 1
    return s


def wino_layers(c):
    """[(layer index, geometry, blocks_x, blocks_y, (H, W, Cin, Ho, Wo, Cout))] of the layers winograd_geometry() takes"""
    out = []
    for i, (sh, s) in enumerate(zip(config(c).layer_shapes(), c.strides)):
        g = winograd_geometry(i, sh, s)
        if g >= 0:
            out.append((i, g, sh[4] // 16 if g == 0 else 1, sh[3] // 16 if g == 0 else 1, sh))
    return out


def forms(c):
    """the AAE_WINO_FORMS rows (G, SC, ST) the four (static_halo, stage32) settings of a case launch"""
    rows = set()
    for _, g, bx, by, sh in wino_layers(c):
        for halo, stage32 in HALO_STAGE_SETTINGS:
            st = layer_static_halo(g, bx, by, halo)
            rows.add((layer_geom_tag(g, st), layer_stage_channels(g, sh[2], stage32, st), st))
    return rows


def check_coverage(cs):
    """what the table exists for; a case list that lost one of these fails at import"""
    for c in cs:
        assert [('conv%d' % (i + 1)) for i, _, _, _, _ in wino_layers(c)] == list(c.wino), (c.name, 'the stated Winograd layers are not what winograd_geometry gives')
        assert set(c.options.items()) >= set(BASE_OPTIONS.items()) and 2 <= len(c.filters) <= 3 and set(c.lines) <= set(TABLE_LINES), c.name
    for subset, what in ((cs, 'case'), ([c for c in cs if not c.gpu_only], 'case that runs on the emulator')):
        reached = set().union(*[forms(c) for c in subset])
        assert reached == WINO_FORMS, 'AAE_WINO_FORMS rows without a %s: %s' % (what, sorted(WINO_FORMS - reached))
        lines = {l for c in subset for l in c.lines}
        assert lines == set(TABLE_LINES), 'table lines without a %s: %s' % (what, sorted(set(TABLE_LINES) - lines))
    by_line = lambda line: [c for c in cs if line in c.lines]
    grids = {(bx, by) for c in by_line(NON_SQUARE) for _, g, bx, by, _ in wino_layers(c) if g == 0}
    assert {(2, 1), (1, 2), (3, 1), (2, 3)} <= grids, grids
    assert {c.B for c in by_line(NON_SQUARE) if c.filters == (32, 64) and c.shape[:2] in ((64, 128), (128, 64))} == {1, 3, 5}
    regions = {sum(bx * by for _, g, bx, by, _ in wino_layers(c) if g == 0) * c.B for c in by_line(RAGGED_GROUPS)}
    assert {6, 10} <= regions, regions
    nbn = collections.defaultdict(set)
    for c in by_line(NBN):
        for _, g, bx, by, sh in wino_layers(c):
            nbn[sh[5] // 64].add((sh[3], sh[4]))
    assert all({(16, 16), (16, 32)} <= nbn[n] for n in (3, 5, 6, 12)), dict(nbn)
    assert all(c.B == 1 for c in cs if 768 in c.filters)
    xcd = {(sh[5] // 64, v) for c in by_line(XCD_COLS) for _, _, _, _, sh in wino_layers(c) for v in c.xcd}
    assert xcd >= {(3, v) for v in (-1, 0, 1, 3)} | {(6, v) for v in (-1, 0, 1, 2, 3)}, xcd
    assert [xcd_cols(6, v) for v in (-1, 0, 1, 2, 3)] == [6, 0, 0, 0, 3] and [xcd_cols(3, v) for v in (-1, 0, 1, 3)] == [3, 0, 0, 3] and xcd_cols(12, -1) == 0
    stages = {(sh[2], sh[3]) for c in by_line(ODD_STAGES) for _, _, _, _, sh in wino_layers(c)}
    assert stages >= {(96, 16), (160, 16), (96, 8), (160, 8)}, stages
    assert {c.B for c in by_line(GEOM1) if c.filters == (32, 64)} == {1, 3, 4, 5, 9}
    assert any(sh[5] == 192 and g == 1 for c in by_line(GEOM1) for _, g, _, _, sh in wino_layers(c))
    assert all(c.bn for c in by_line(BN_MIXED) + by_line(BN_SCALE)) and any(len(c.wino) == 2 for c in by_line(BN_SCALE))
    edge = {config(c).layer_shapes()[1][3:5] for c in by_line(EDGE)}
    assert edge >= {(8, 16), (16, 8), (24, 24)} and any(c.strides[-1] == 1 and len(c.strides) == 3 for c in by_line(EDGE)), edge


check_coverage(cases())


# ---- inputs --------------------------------------------------------------------------------------------------------------------
Inputs = collections.namedtuple('Inputs', 'cfg w x z64 acts64')


def bn_vectors(w, cfg, layer):
    """(scale, shift) of a layer's batch norm as the host computes them (aae_abi_impl.h:63-66: float32 arithmetic), or None"""
    if not cfg.batch_norm:
        return None
    p = ref.layer_names(cfg.num_layers, True)[1][layer]
    g, be, mu, var = (np.asarray(w[p + '/' + n], dtype=np.float32) for n in ('gamma', 'beta', 'moving_mean', 'moving_variance'))
    inv = (np.float32(1.0) / np.sqrt(var + np.float32(ref.BN_EPS))) * g
    return inv, be - mu * inv


def layer_weights(w, cfg, layer):
    name = ref.layer_names(cfg.num_layers, cfg.batch_norm)[0][layer]
    return w[name + '/kernel'], w[name + '/bias']


@functools.lru_cache(maxsize=None)
def build_inputs(name):
    """Weights, crops and the whole-network fp64 expectation of a case (computed once, shared by every test of the process, read-only).
    Asserts that the comparison cannot be empty: every activation has at least a tenth of its entries non-zero."""
    c = {k.name: k for k in cases()}[name]
    cfg = config(c)
    w = synth.make_weights(seed=c.seed, shape=cfg.shape, num_filter=cfg.num_filter, strides=cfg.strides, latent=cfg.latent_space_size,
                           batch_norm=cfg.batch_norm, kernel_size=cfg.kernel_size)
    x = synth.make_crops(c.B, seed=c.seed + 1, shape=cfg.shape)
    z64, acts64 = ref.encoder_forward_np(ref.input_to_float(x), w, cfg.strides, cfg.batch_norm, return_activations=True)
    for i, a in enumerate(acts64):
        assert np.count_nonzero(a) >= a.size / 10.0, '%s: activation %d is dead' % (name, i)
    for a in [x, z64] + list(acts64) + list(w.values()):
        a.setflags(write=False)
    return Inputs(cfg, w, x, z64, tuple(acts64))


# ---- check b: one layer, element by element ------------------------------------------------------------------------------------------
LayerRef = collections.namedtuple('LayerRef', 'want S extra n')


def layer_reference(x_in, kernel, bias, stride, bn=None):
    """The fp64 expectation of ONE layer on the input x_in (any float dtype, widened to float64; NHWC) and the scale of its rounding
    errors: S = conv(|x|, |w|) + |b|, n = taps x Cin.  bn = (scale, shift): the kernels compute scale relu(conv) + shift; then S is
    |scale| S and `extra` the one rounding of that last operation, u (|scale relu(conv)| + |shift|)."""
    x64 = np.asarray(x_in, dtype=np.float64)
    want = ref.conv2d_same_relu_np(x64, kernel, bias, stride)
    S = ref.conv2d_same_relu_np(np.abs(x64), np.abs(np.asarray(kernel, dtype=np.float64)), np.abs(np.asarray(bias, dtype=np.float64)), stride, relu=False)
    extra = np.zeros_like(S)
    if bn is not None:
        scale, shift = (np.asarray(v, dtype=np.float64) for v in bn)
        extra = U * (np.abs(scale * want) + np.abs(shift))
        want = scale * want + shift
        S = np.abs(scale) * S
    assert S.min() > 0
    return LayerRef(want, S, extra, int(np.prod(np.shape(kernel)[:3])))


def element_ratio(got, lr):
    """(|got - want| - extra) / (u S) per element, not below 0: what check b holds against ALLOWANCE"""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == lr.want.shape, (got.shape, lr.want.shape)
    return np.maximum(np.abs(got - lr.want) - lr.extra, 0.0) / (U * lr.S)


def check_elements(got, lr, where):
    """check b; returns the largest ratio"""
    assert np.isfinite(got).all(), '%s: not finite' % where
    r = element_ratio(got, lr)
    worst = np.unravel_index(int(np.argmax(r)), r.shape)
    assert r[worst] <= ALLOWANCE, '%s: |got - want| = %.2f u S at %s (allowance %.2f)' % (where, r[worst], tuple(int(v) for v in worst), ALLOWANCE)
    return float(r[worst])


def check_norms(got, want, where, tol_max=LAYER_TOL_MAX, tol_l2=LAYER_TOL_L2):
    """check c: tests/test_gpu_parity.py's _check_layer, restated (the emulator test must not import the GPU module)"""
    g, a = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert g.shape == a.shape, (g.shape, a.shape)
    e_max = float(np.abs(g - a).max() / np.abs(a).max())
    e_l2 = float(np.linalg.norm((g - a).ravel()) / np.linalg.norm(a.ravel()))
    assert e_max < tol_max, '%s: max-norm rel err %.3e' % (where, e_max)
    assert tol_l2 is None or e_l2 < tol_l2, '%s: l2 rel err %.3e' % (where, e_l2)
    return e_max, e_l2


def yardstick_ratio(x_in, kernel, bias, stride):
    """The yardstick of ALLOWANCE: the float32 NumPy direct form of a layer (conv + bias + ReLU) against its float64 twin on the same
    float32 input, in units of u S, per element"""
    x32 = np.asarray(x_in, dtype=np.float32)
    return element_ratio(ref.conv2d_same_relu_np(x32, kernel, bias, stride, dtype=np.float32), layer_reference(x32, kernel, bias, stride))


def oracle_layer_input(inp, layer):
    """the input of a layer as a float32 array when nothing upstream is under test (the checker test, the yardstick): the crops through
    the float32 feed cast, or the oracle's previous activation rounded once"""
    if layer == 0:
        return ref.input_to_float(inp.x).astype(np.float32)
    return inp.acts64[layer - 1].astype(np.float32)


# ---- the adapters over EncoderEngine / EmuEncoder ---------------------------------------------------------------------------------
Run = collections.namedtuple('Run', 'z acts labels')


class GpuBackend(object):
    """engine.EncoderEngine; poison(): the whole workspace buffer filled with one byte value before the next call"""
    name = 'gpu'
    poison_bytes = (0xFF, 0x00, 0xA5)

    def create(self, cfg, w, B):
        from augmentedautoencoder_amd.engine import EncoderEngine
        return EncoderEngine(cfg, w, max_batch=B)

    def forward(self, enc, x):
        z, recs = enc.encode_timed(np.array(x))
        return Run(z.cpu().numpy(), [enc.activation(i).cpu().numpy() for i in range(enc.cfg.num_layers)], [l for l, _, _ in recs])

    def poison(self, enc, byte):
        buf, _ = enc.ws.get(0)                   # (grown to the case's size by the runs before)
        buf.fill_(byte)


class EmuBackend(object):
    """emu_backend.EmuEncoder: every forward() gets a fresh workspace full of 0xA5"""
    name = 'emu'
    poison_bytes = ()

    def create(self, cfg, w, B):
        import emu_backend
        return emu_backend.EmuEncoder(w, cfg)

    def forward(self, enc, x):
        z = enc.forward(np.array(x))
        return Run(z, [enc.activation(i) for i in range(enc.cfg.num_layers)], enc.labels())

    def poison(self, enc, byte):
        raise NotImplementedError


_NUMBER = re.compile(r'(\w+)=(\d+)')
WINO_LABEL = 'conv_wino_f32 layer'


def check_labels(case, labels):
    """check a"""
    wino = [l for l in labels if 'conv_wino_f32' in l]
    assert [l.split(':')[0] for l in wino] == list(case.wino) and all(WINO_LABEL in l for l in wino), (case.name, labels)
    shapes = config(case).layer_shapes()
    for l in wino:
        H, W, Cin, Ho, Wo, Cout = shapes[int(l.split(':')[0][4:]) - 1]
        got = dict(_NUMBER.findall(l))
        assert (got.get('M'), got.get('N'), got.get('C')) == (str(case.B * Ho * Wo), str(Cout), str(Cin)), (l, case.B, Ho, Wo, Cout, Cin)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same_bits(run, want, what, order=None):
    for i, (a, b) in enumerate(zip([run.z] + list(run.acts), [want.z] + list(want.acts))):
        b = b if order is None else b[order]
        assert a.shape == b.shape and np.array_equal(_bits(a), _bits(b)), '%s: %s differs' % (what, 'the latent' if i == 0 else 'activation %d' % (i - 1))


def run_case(case, backend, options=None, bit_checks=True):
    """One case on one backend (a fresh handle, closed here).  options: further encoder options (the emulator's experiments-only
    forms); bit_checks = False: checks a-c of ONE run only.  Prints and returns {layer name: (kind, largest |got - want| / (u S))}."""
    inp = build_inputs(case.name)
    cfg, nl = inp.cfg, inp.cfg.num_layers
    enc = backend.create(cfg, inp.w, case.B)
    try:
        for k, v in list(case.options.items()) + list((options or {}).items()):
            enc.set_option(k, v)
        base = backend.forward(enc, inp.x)
        # a. labels
        if (options or {}).get('winograd', 1) == 1:
            check_labels(case, base.labels)
        # b. every layer against the fp64 convolution of its own input
        ratios = {}
        for i in range(nl):
            kernel, bias = layer_weights(inp.w, cfg, i)
            x_in = ref.input_to_float(inp.x).astype(np.float32) if i == 0 else base.acts[i - 1]
            lr = layer_reference(x_in, kernel, bias, cfg.strides[i], bn_vectors(inp.w, cfg, i))
            name = 'conv%d' % (i + 1)
            kind = 'winograd' if any(l.startswith(name + ':') and 'conv_wino_f32' in l for l in base.labels) else 'direct'
            ratios[name] = (kind, check_elements(base.acts[i], lr, '%s %s (%s, %s)' % (case.name, name, kind, backend.name)))
        print('%s [%s]: max |got - want| / (u S): %s' % (case.name, backend.name, ', '.join('%s %s %.2f' % (n, k, r) for n, (k, r) in ratios.items())))
        # c. the project's norms against the whole-network oracle
        for i in range(nl):
            check_norms(base.acts[i], inp.acts64[i], '%s layer %d' % (case.name, i))
        check_norms(base.z, inp.z64, '%s latent' % case.name, LATENT_TOL, None)
        if not bit_checks:
            return ratios
        # d. bit equalities, every run twice
        def twice(what, x=inp.x, order=None, given=0):
            for rep in range(given + 1, 3):
                run = backend.forward(enc, x)
                assert [l for l in run.labels if 'wino' in l] == [l for l in base.labels if 'wino' in l], (what, run.labels)
                _same_bits(run, base, '%s, run %d' % (what, rep), order)
        for halo, stage32 in HALO_STAGE_SETTINGS:
            enc.set_option('winograd_static_halo', halo)
            enc.set_option('winograd_stage32', stage32)
            twice('(winograd_static_halo, winograd_stage32) = (%d, %d)' % (halo, stage32), given=int((halo, stage32) == HALO_STAGE_SETTINGS[0]))      # (the first run of the defaults is `base`)
        enc.set_option('winograd_static_halo', 1)
        enc.set_option('winograd_stage32', 1)
        for v in case.xcd:
            if v == -1:                          # (the default: `base` and the second run of the default settings above)
                continue
            enc.set_option('winograd_xcd_cols', v)
            twice('winograd_xcd_cols = %d' % v)
        enc.set_option('winograd_xcd_cols', -1)
        if case.B > 1:                           # (one image has no derangement)
            order = np.roll(np.arange(case.B), 1)
            twice('images permuted', inp.x[order], order)
        # e. poison in the workspace
        for byte in backend.poison_bytes:
            backend.poison(enc, byte)
            run = backend.forward(enc, inp.x)
            assert all(np.isfinite(a).all() for a in [run.z] + list(run.acts)), 'workspace full of %#04x: an output is not finite' % byte
            _same_bits(run, base, 'workspace full of %#04x' % byte)
        return ratios
    finally:
        enc.close()


# ---- the grouped frame (conv_wino_layer_multi_kernel at blocks_x = 2) ----------------------------------------------------------------
GROUPED = dict(config=((64, 128, 3), [32, 64], [2, 2], 5, 128, False), counts=[5, 7, 6], weight_seeds=[2301, 2302, 2303],
               codebook_rows=[36 * 8, 36 * 9 + 1, 36 * 10 + 2], crop_seed=2310,
               launches=4)                       # launches of the grouped part: the emulator's count, pinned by tests/test_emu_winograd_shapes.py
GROUPED_LATENT_TOL = 2e-5


def grouped_options():
    """multi_form_cases.WINO with the planner's round size pinned: the same plan on the emulator and on the MI355X"""
    import multi_form_cases
    return dict(multi_form_cases.WINO, wavek_target_blocks=256)
