"""tests/decoder_form_cases.py on the CPU fiber emulator: proves without a GPU that every case reaches the launch forms its row
states (the labels of aae_decoder_create / launch_stage / launch_igemm), that its fp64 expectation is sound (no dead layer,
no saturated output: asserted by the builder, for the gpu_only cases too) and that the kernels' arithmetic agrees with fp64
at these sizes.  Runs on the product build of the emulator library (libaae_emu_product.so): the host code the GPU library
compiles, so the labels are the ones tests/test_gpu_decoder_forms.py must see."""
import ctypes
import fcntl
import os
import subprocess

import pytest

import decoder_form_cases as dfc
import emu_backend as eb
from augmentedautoencoder_amd import _lib

_PRODUCT = None


def _product_lib():
    global _PRODUCT
    if _PRODUCT is None:
        with open(os.path.join(eb.HERE, 'emu', '.build.lock'), 'w') as lock:      # pytest -n: one worker builds, the others wait
            fcntl.flock(lock, fcntl.LOCK_EX)
            subprocess.check_call(['make', '-s', '-C', os.path.join(eb.HERE, 'emu'), 'libaae_emu_product.so'])
        _PRODUCT = _lib.declare(ctypes.CDLL(os.path.join(eb.HERE, 'emu', 'libaae_emu_product.so')))
    return _PRODUCT


class ProductEmuDecoder(eb.EmuDecoder):
    """emu_backend.EmuDecoder on the product build of the emulator library"""

    def __init__(self, weights, cfg):
        from augmentedautoencoder_amd.weights import as_pointer_array, ordered_decoder_weight_arrays
        self.cfg = cfg
        self.L = _product_lib()
        self._arrays = ordered_decoder_weight_arrays(weights, cfg)
        h = ctypes.c_void_p()
        desc = cfg.to_desc()
        _lib.check(self.L, self.L.aae_decoder_create(ctypes.byref(desc), as_pointer_array(self._arrays), len(self._arrays), ctypes.byref(h)), 'aae_decoder_create')
        self.h = h


@pytest.mark.parametrize('case', [c for c in dfc.cases() if not c.gpu_only], ids=dfc.case_id)
def test_decoder_form(case):
    dfc.run_case(case, dfc.EmuBackend(ProductEmuDecoder))


@pytest.mark.parametrize('case', [c for c in dfc.cases() if c.gpu_only], ids=dfc.case_id)
def test_inputs_of_a_gpu_only_case(case):
    """the cases the emulator does not run: their weights, codes and fp64 expectation are built here all the same -- a dead
    layer or a saturated output is found on the CPU -- and the handle is created: its workspace plan is the host's"""
    inp = dfc.build_inputs(case.name)
    assert inp.x64.shape == (case.B,) + case.out and len(inp.acts64) == len(case.F)
    dec = ProductEmuDecoder(inp.w, inp.cfg)
    try:
        assert dec.L.aae_decoder_workspace_bytes(dec.h, case.B) > 0
    finally:
        dec.close()


def test_the_table_covers_what_it_exists_for():
    dfc.check_coverage(dfc.cases())
    assert all(len(c.launches) >= 1 + len(c.F) for c in dfc.cases())
