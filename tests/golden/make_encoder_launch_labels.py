"""Records tests/golden/encoder_launch_labels.json: per case of tests/encoder_launch_cases.py the complete sequence of (kernel label,
flops) of one encoder forward, and of one decoder forward for the decoder's cases, in commit c0553b5 ("Grouped query: every launch
form checked on the GPU against fp64") -- BEFORE the per-class launch code got one form list per kernel family and one launch tail.
Once from the experiments build of the emulator and once from the product build, where an option the build refuses is recorded as
the refusal code.

From the root of a checkout of that commit, with tests/encoder_launch_cases.py and this file copied in:

    make -C tests/emu libaae_emu.so libaae_emu_product.so
    python tests/golden/make_encoder_launch_labels.py > encoder_launch_labels.json

tests/test_encoder_launch_labels.py replays the cases on the working tree's two emulator builds and compares every record;
tests/test_gpu_launch_forms.py runs the product half on the hardware."""
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))]

import encoder_launch_cases as elc                            # noqa: E402
from augmentedautoencoder_amd import _lib                     # noqa: E402


def main():
    out = {'parent': 'c0553b5', 'cases': elc.cases(), 'decoder_cases': elc.decoder_cases()}
    for build, name in (('experiments', 'libaae_emu.so'), ('product', 'libaae_emu_product.so')):
        L = _lib.declare(ctypes.CDLL(os.path.join(os.path.dirname(HERE), 'emu', name)))
        assert L.aae_has_experiments() == (build == 'experiments')
        out[build] = elc.replay_all(L)
    text = json.dumps(out, separators=(',', ':'))
    print(text.replace('{"records"', '\n{"records"').replace('{"refused"', '\n{"refused"').replace('{"name"', '\n{"name"'))


if __name__ == '__main__':
    main()
