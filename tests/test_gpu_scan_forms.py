"""tests/scan_form_cases.py on the MI355X: every launch form of the codebook scan -- the stream kernels, the query-resident
kernel in its three geometries and with its in-scan top-k lists, the tile-resident MFMA and bf16 kernels, masked and compacted
upright queries, narrow latents, unaligned queries -- at row counts on and next to every tile edge, each against the fp64
oracle with exact row indices (the table's docstring says why that is legitimate).  The emulator twin
(tests/test_emu_scan_forms.py) pins the same launch counts on the CPU; what only the hardware shows is the out-of-range part
of an LDS-DMA tile, the raised dynamic-LDS ceilings, the real MFMA paths and the 256-CU row-block split."""
import pytest

import parity_report
import scan_form_cases as sfc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def engines():
    """one CodebookEngine per (dtype, N, J, with / without the compacted upright copy), shared by the cases on that book"""
    from augmentedautoencoder_amd.engine import CodebookEngine
    made = {}

    def make(E, dtype, key):
        if key is None:
            return CodebookEngine(E, dtype=dtype)
        if key not in made:
            made[key] = CodebookEngine(E, dtype=dtype)
        return made[key]
    try:
        yield make
    finally:
        for cb in made.values():
            cb.close()


@pytest.mark.parametrize('case', sfc.cases(), ids=sfc.case_id)
def test_scan_form(engines, case):
    err = sfc.run_case(case, engines)
    parity_report.record('scan_forms', sfc.case_id(case), dtype=case.dtype, max_cos_err=err, cos_tol=sfc.COS_TOL)


def test_bf16_codebook_with_a_narrow_latent_is_refused(engines):
    sfc.check_narrow_bf16_refused(engines)
