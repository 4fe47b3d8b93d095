"""tests/scan_form_cases.py on the CPU fiber emulator: proves without a GPU that every case's inputs satisfy the gap condition
(exact comparison with the fp64 oracle is legitimate) and that the launch counts written in the table are the ones the host
code queues.  Runs on the product build of the emulator library (libaae_emu_product.so): the launch counts are those of the
host code the product library compiles -- the experiments build sends a masked upright query of B <= 4 to stream-kernel
variants the product does not have (one launch instead of three).  The hardware twin is tests/test_gpu_scan_forms.py."""
import ctypes
import fcntl
import os
import subprocess

import numpy as np
import pytest

import emu_backend as eb
import scan_form_cases as sfc
from augmentedautoencoder_amd import _lib
from augmentedautoencoder_amd.weights import to_bf16_bits

CASES = [c for c in sfc.cases() if not c.gpu_only]
_PRODUCT = None


def _product_lib():
    global _PRODUCT
    if _PRODUCT is None:
        with open(os.path.join(eb.HERE, 'emu', '.build.lock'), 'w') as lock:      # pytest -n: one worker builds, the others wait
            fcntl.flock(lock, fcntl.LOCK_EX)
            subprocess.check_call(['make', '-s', '-C', os.path.join(eb.HERE, 'emu'), 'libaae_emu_product.so'])
        _PRODUCT = _lib.declare(ctypes.CDLL(os.path.join(eb.HERE, 'emu', 'libaae_emu_product.so')))
    return _PRODUCT


class ProductEmuCodebook(eb.EmuCodebook):
    """emu_backend.EmuCodebook on the product build of the emulator library"""

    def __init__(self, E, dtype='f32'):
        self.L = _product_lib()
        self.E = np.ascontiguousarray(E, dtype=np.float32)
        src, dt = (to_bf16_bits(self.E), _lib.AAE_DTYPE_BF16) if dtype == 'bf16' else (self.E, _lib.AAE_DTYPE_F32)
        h = ctypes.c_void_p()
        _lib.check(self.L, self.L.aae_codebook_create(src.ctypes.data, self.E.shape[0], self.E.shape[1], dt, 0, ctypes.byref(h)), 'aae_codebook_create')
        self.h = h


@pytest.fixture(scope='module')
def engines():
    made = {}

    def make(E, dtype, key):
        if key is None:
            return ProductEmuCodebook(E, dtype)
        if key not in made:
            made[key] = ProductEmuCodebook(E, dtype)
        return made[key]
    try:
        yield make
    finally:
        for cb in made.values():
            cb.close()


@pytest.mark.parametrize('case', CASES, ids=sfc.case_id)
def test_scan_form(engines, case):
    sfc.run_case(case, engines)


@pytest.mark.parametrize('case', [c for c in sfc.cases() if c.gpu_only], ids=sfc.case_id)
def test_inputs_of_a_gpu_only_case(case):
    """the cases the emulator does not run: their inputs are built here all the same -- the gap condition, the planted ties and
    the last row among the answers are asserted by the builder, on the CPU"""
    inp = sfc.build_inputs(case.dtype, case.N, case.J, case.B, case.k, case.col_stride)
    assert inp.z.shape == (case.B, case.J) and inp.want.shape == (case.B, case.k)


def test_bf16_codebook_with_a_narrow_latent_is_refused(engines):
    sfc.check_narrow_bf16_refused(engines)


def test_every_axis_of_the_table_is_populated():
    """the classes the table exists for: a case list that lost one of them fails here, not silently"""
    cs = sfc.cases()
    assert {c.J for c in cs} == {4, 64, 124, 128} and {c.dtype for c in cs} == {'f32', 'bf16'}
    assert {c.mode for c in cs} == set(sfc.MODE_NAMES)
    assert {c.B for c in cs} >= {1, 2, 3, 4, 5, 32, 33, 70, 128, 129, 256, 257, 9, 130}
    assert {c.N for c in cs} >= {1, 8, 63, 64, 65, 127, 128, 129, 255, 256, 257, 401, 2049, sfc.LADDER_N, sfc.BIG}
    assert {c.k for c in cs if c.call == 'nn'} >= {1, 2, 3, 5, 8, 9, 60, 400}
    assert any(c.col_stride > 1 and c.upright_copy for c in cs) and any(c.col_stride > 1 and not c.upright_copy for c in cs)
    assert any(c.z_offset_floats for c in cs) and any(c.call == 'similarity' for c in cs)
    assert all(c.dtype == 'f32' for c in cs if c.J != 128)
