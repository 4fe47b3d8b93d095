"""The element check of tests/wino_shape_cases.py (check b of run_case) would fail on a subtly wrong kernel: a CPU test, no GPU and no
emulator.  Per table case and layer under test (the layers expected in the Winograd form; conv2 where the case expects none), the
check is fed a correct float32 output -- the fp64 reference of the layer on the oracle's input, rounded once -- damaged the way a
kernel mistake would damage it, and must fail; undamaged, and for the float32 NumPy yardstick the allowance was measured with, it
must pass.  Each mistake states which cases it must trip and prints how many it trips."""
import functools

import numpy as np
import pytest

import wino_shape_cases as wsc

CASES = wsc.cases()


def layers_under_test(case):
    """[(layer index, geometry or -1, blocks_x, blocks_y)]"""
    wino = [(i, g, bx, by) for i, g, bx, by, _ in wsc.wino_layers(case)]
    return wino or [(1, -1, 1, 1)]


@functools.lru_cache(maxsize=None)
def _layer(name, layer):
    """(x_in float32, kernel, bias, stride, bn, LayerRef, the correct float32 output) of a case's layer"""
    inp = wsc.build_inputs(name)
    kernel, bias = wsc.layer_weights(inp.w, inp.cfg, layer)
    bn = wsc.bn_vectors(inp.w, inp.cfg, layer)
    x_in = wsc.oracle_layer_input(inp, layer)
    lr = wsc.layer_reference(x_in, kernel, bias, inp.cfg.strides[layer], bn)
    return x_in, kernel, bias, inp.cfg.strides[layer], bn, lr, lr.want.astype(np.float32)


def _fails(damaged, lr):
    return float(wsc.element_ratio(damaged, lr).max()) > wsc.ALLOWANCE


# ---- the seeded mistakes: (case, layer, geometry, blocks_x, blocks_y) -> damaged float32 output, or None where the mistake does not apply
def swapped_bx_by(case, layer, geom, bx, by):
    """wino_block_geometry<0> unpacking a region number with blocks_x and blocks_y exchanged: every block computes the window it believes
    it has and stores it there; a window outside the image is not stored, what no block stores stays zero"""
    if geom != 0 or bx == by:
        return None
    good = _layer(case.name, layer)[6]
    out = np.zeros_like(good)
    for local in range(bx * by):
        sbx, sby = local % by, (local // by) % bx
        if sbx < bx and sby < by:
            out[:, 16 * sby:16 * sby + 16, 16 * sbx:16 * sbx + 16] = good[:, 16 * sby:16 * sby + 16, 16 * sbx:16 * sbx + 16]
    return out


def padding_2_1_along_x(case, layer, geom, bx, by):
    """'SAME' padding of a 5 x 5 stride-2 layer on an even width is (1, 2); (2, 1) along x is the (1, 2) convolution of the image with a
    zero column on either side, without its last output column"""
    x_in, kernel, bias, stride, bn, lr, good = _layer(case.name, layer)
    if stride != 2:
        return None
    wider = np.pad(x_in, ((0, 0), (0, 0), (1, 1), (0, 0)))
    return wsc.layer_reference(wider, kernel, bias, stride, bn).want[:, :, :good.shape[2]].astype(np.float32)


def last_stage_dropped(case, layer, geom, bx, by):
    x_in, kernel, bias, stride, bn, lr, good = _layer(case.name, layer)
    if x_in.shape[3] < 64:
        return None
    x = x_in.copy()
    x[..., -32:] = 0
    return wsc.layer_reference(x, kernel, bias, stride, bn).want.astype(np.float32)


def last_column_block_with_block_0_vectors(case, layer, geom, bx, by):
    x_in, kernel, bias, stride, bn, lr, good = _layer(case.name, layer)
    if kernel.shape[3] < 128:
        return None
    def moved(v):
        v = np.array(v)
        v[-64:] = v[:64]
        return v
    return wsc.layer_reference(x_in, kernel, moved(bias), stride, None if bn is None else (moved(bn[0]), moved(bn[1]))).want.astype(np.float32)


def last_image_of_a_ragged_block_left_zero(case, layer, geom, bx, by):
    if case.B % 4 == 0:
        return None
    out = _layer(case.name, layer)[6].copy()
    out[-1] = 0
    return out


def _one_element_off(case, layer):
    """(damaged output, index): the element with the smallest S, moved by 8 x ALLOWANCE u S"""
    lr, good = _layer(case.name, layer)[5:7]
    at = np.unravel_index(int(np.argmin(lr.S)), lr.S.shape)
    out = good.copy()
    out[at] = np.float32(lr.want[at] + 8 * wsc.ALLOWANCE * wsc.U * lr.S[at])
    return out, at


def one_element_off(case, layer, geom, bx, by):
    return _one_element_off(case, layer)[0]


# (mistake, the cases it must trip -- a predicate on (case, layer shape (H, W, Cin, Ho, Wo, Cout), geometry, blocks_x, blocks_y) --, how many (case, layer) pairs that is)
MISTAKES = [
    (swapped_bx_by, lambda c, sh, g, bx, by: g == 0 and bx != by, 12),
    (padding_2_1_along_x, lambda c, sh, g, bx, by: True, 35),
    (last_stage_dropped, lambda c, sh, g, bx, by: sh[2] >= 64, 9),
    (last_column_block_with_block_0_vectors, lambda c, sh, g, bx, by: sh[5] >= 128, 10),
    (last_image_of_a_ragged_block_left_zero, lambda c, sh, g, bx, by: c.B % 4 != 0, 34),
    (one_element_off, lambda c, sh, g, bx, by: True, 35),
]


@pytest.mark.parametrize('mistake,must_trip,pairs', MISTAKES, ids=[m.__name__ for m, _, _ in MISTAKES])
def test_seeded_mistake_trips_the_element_check(mistake, must_trip, pairs):
    tripped, cases_tripped, missed = 0, set(), []
    for case in CASES:
        shapes = wsc.config(case).layer_shapes()
        for layer, geom, bx, by in layers_under_test(case):
            damaged = mistake(case, layer, geom, bx, by)
            applies = must_trip(case, shapes[layer], geom, bx, by)
            assert applies == (damaged is not None), (mistake.__name__, case.name, layer)
            if damaged is None:
                continue
            if _fails(damaged, _layer(case.name, layer)[5]):
                tripped += 1
                cases_tripped.add(case.name)
            else:
                missed.append((case.name, layer))
    print('%s: trips %d (case, layer) pairs in %d of %d cases' % (mistake.__name__, tripped, len(cases_tripped), len(CASES)))
    assert not missed, missed
    assert tripped == pairs, tripped


# The layers where even the SMALLEST S of the layer lies above 2e-5 / (8 ALLOWANCE u) = 1.76 times the layer's largest output: sums over
# 160 and more input channels that cancel to a small result.  There the max norm of check c is the tighter bound for that one element (and
# check b the tighter one for all the small outputs beside it); everywhere else check c passes the damaged output.
MAX_NORM_SEES_ONE_ELEMENT = {('nbn5_16x16', 2), ('nbn6_16x16', 2), ('nbn12_16x16', 2), ('cin160_16x16', 1), ('bn_nbn3_then_geom1', 2)}


def test_the_max_norm_checks_alone_pass_the_one_element_mistake():
    """what check b adds to check c: an element off by 8 x ALLOWANCE u S -- some hundred times what the kernels miss by -- passes the 2e-5
    max norm and the 1e-5 2-norm of tests/test_gpu_parity.py, in every case but the wide-Cin layers listed above"""
    seen = set()
    for case in CASES:
        for layer, _, _, _ in layers_under_test(case):
            damaged, at = _one_element_off(case, layer)
            lr = _layer(case.name, layer)[5]
            assert _fails(damaged, lr)
            try:
                wsc.check_norms(damaged, lr.want, '%s layer %d' % (case.name, layer))
            except AssertionError:
                seen.add((case.name, layer))
                assert lr.S.min() > 2e-5 / (8 * wsc.ALLOWANCE * wsc.U) * np.abs(lr.want).max() and lr.S.shape[-1] >= 64 and _layer(case.name, layer)[0].shape[3] >= 160
    assert seen == MAX_NORM_SEES_ONE_ELEMENT, seen


def test_correct_output_passes():
    for case in CASES:
        for layer, _, _, _ in layers_under_test(case):
            lr, good = _layer(case.name, layer)[5:7]
            assert wsc.check_elements(good, lr, case.name) <= 1.0          # (one rounding of |want| <= S; with BN, of the last operation: `extra`)


def test_yardstick_passes_and_allowance_stays_below_the_direct_bound():
    """the float32 NumPy direct form of every conv layer of every case: within ALLOWANCE (a quarter of it on the machine the constant was
    measured on), and ALLOWANCE below the (n + 8) u S of a direct sum of n = 25 Cin terms, for every layer"""
    assert wsc.ALLOWANCE == 4.0 * wsc.YARDSTICK_MAX
    worst = 0.0
    for case in CASES:
        inp = wsc.build_inputs(case.name)
        figures = []
        for layer in range(inp.cfg.num_layers):
            kernel, bias = wsc.layer_weights(inp.w, inp.cfg, layer)
            assert wsc.ALLOWANCE < int(np.prod(kernel.shape[:3])) + 8, (case.name, layer)
            figures.append(float(wsc.yardstick_ratio(wsc.oracle_layer_input(inp, layer), kernel, bias, inp.cfg.strides[layer]).max()))
        print('%s: yardstick %s u S' % (case.name, ' '.join('%.3f' % f for f in figures)))
        worst = max(worst, max(figures))
    print('yardstick maximum %.3f u S, allowance %.3f' % (worst, wsc.ALLOWANCE))
    assert worst <= wsc.ALLOWANCE
