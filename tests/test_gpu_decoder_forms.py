"""tests/decoder_form_cases.py on the MI355X: every stage form of the decoder -- plain igemm split and un-split, the phased
(SCATTER) igemm at ragged M, two N tiles, one K slab and 1 ... 6 taps per axis, the narrow kernel hidden and last, ragged,
multi-chunk and above the default LDS ceiling, the direct kernel at 1x, 2x, 3x and 7 -> 15, the dense layer split, un-split
and generic -- each against the fp64 restatement of the reference decoder, the output handed in full of NaN and the
workspace full of 0xA5.  The emulator twin (tests/test_emu_decoder_forms.py) pins the same labels on the CPU; what only the
hardware shows is the bounds-checked buffer views and the LDS DMA of the igemm at these geometries, the LDS ceiling and the
scalar weight loads of the narrow kernel."""
import numpy as np
import pytest

import decoder_form_cases as dfc
import parity_report

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('case', dfc.cases(), ids=dfc.case_id)
def test_decoder_form(case):
    out_err, hidden_err = dfc.run_case(case, dfc.GpuBackend())
    parity_report.record('decoder_forms', case.name, max_out_err=out_err, out_tol=dfc.OUT_TOL, max_hidden_rel=hidden_err, hidden_tol=dfc.HIDDEN_TOL_GPU)


def test_two_engines_taking_turns_keep_their_lds_ceilings():
    """the narrow kernel's LDS ceiling is set per launch, from the stage being launched: an engine whose last stage needs
    73 216 B (k = 11) and one that needs 50 688 B (k = 5, hidden and last) decode alternately, three times each -- both stay
    equal to their first result bit for bit, and that result is the fp64 one"""
    backend = dfc.GpuBackend()
    by_name = {c.name: c for c in dfc.cases()}
    pair = [by_name['k11_lds'], by_name['hidden_narrow']]
    inputs = [dfc.build_inputs(c.name) for c in pair]
    engines = [backend.create(i.cfg, i.w) for i in inputs]
    try:
        first = [None, None]
        for turn in range(3):
            for j, (dec, inp) in enumerate(zip(engines, inputs)):
                x = backend.forward(dec, inp.z)
                assert not np.isnan(x).any(), (turn, pair[j].name)
                if turn == 0:
                    assert np.abs(x - inp.x64).max() <= dfc.OUT_TOL, pair[j].name
                    first[j] = x
                else:
                    assert np.array_equal(x.view(np.uint32), first[j].view(np.uint32)), (turn, pair[j].name)
                dfc.check_labels(pair[j], backend.labels(dec))
    finally:
        for dec in engines:
            dec.close()


def test_decode_checks_the_callers_output_tensor():
    """DecoderEngine.decode(z, out=): shape, dtype, device and contiguity are checked before anything is launched"""
    import torch
    case = {c.name: c for c in dfc.cases()}['dense_generic']
    inp = dfc.build_inputs(case.name)
    dec = dfc.GpuBackend().create(inp.cfg, inp.w)
    try:
        B, shape, z = case.B, (case.B,) + case.out, np.array(inp.z)
        good = torch.full(shape, float('nan'), dtype=torch.float32, device=dec.device)
        assert dec.decode(z, out=good) is good and np.array_equal(good.cpu().numpy(), dec.decode(z).cpu().numpy())
        with pytest.raises(ValueError, match='shape'):
            dec.decode(z, out=torch.empty((B + 1,) + case.out, dtype=torch.float32, device=dec.device))
        with pytest.raises(ValueError, match='shape'):
            dec.decode(z, out=torch.empty((B, case.out[0] * case.out[1] * case.out[2]), dtype=torch.float32, device=dec.device))
        with pytest.raises(ValueError, match='dtype'):
            dec.decode(z, out=torch.empty(shape, dtype=torch.float64, device=dec.device))
        with pytest.raises(ValueError, match='lives on'):
            dec.decode(z, out=torch.empty(shape, dtype=torch.float32))
        with pytest.raises(ValueError, match='contiguous'):
            dec.decode(z, out=torch.empty((B, case.out[1], case.out[0], case.out[2]), dtype=torch.float32, device=dec.device).transpose(1, 2))
        with pytest.raises(ValueError, match='torch tensor'):
            dec.decode(z, out=np.empty(shape, dtype=np.float32))
    finally:
        dec.close()
