"""Records tests/golden/multi_plans.json: what the host planner of the grouped multi-object query (csrc/aae_multi_impl.h) decides
per frame -- which objects aae_multi_workspace_bytes prepares Winograd-domain weights for, the size it returns, and every field of
the MultiPlan the launches are built from -- in commit 9689de6 ("Depth ICP refinement on the GPU behind icp_refinement, estimator
hook"), BEFORE the planner's rules and the launch tables' builders were brought down to one copy each.

From the root of a checkout of that commit, with tests/emu/aae_emu_lib.cpp (the export aae_emu_multi_plan_dump compiles against
that commit's sources unchanged), tests/emu/Makefile, tests/multi_plan_frames.py and this file copied in:

    make -C tests/emu libaae_emu.so libaae_emu_product.so
    python tests/golden/make_multi_plans.py > multi_plans.json

tests/test_multi_plans.py replays the same frames on the working tree's two emulator builds and compares every field."""
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))]

import multi_plan_frames as mpf                               # noqa: E402
from augmentedautoencoder_amd import _lib                     # noqa: E402


def main():
    out = {'parent': '9689de6', 'frames': mpf.frames()}
    for build, name in (('experiments', 'libaae_emu.so'), ('product', 'libaae_emu_product.so')):
        L = _lib.declare(ctypes.CDLL(os.path.join(os.path.dirname(HERE), 'emu', name)))
        assert L.aae_has_experiments() == (build == 'experiments')
        out[build] = [mpf.replay(L, f) for f in out['frames']]
    text = json.dumps(out, separators=(',', ':'))
    print(text.replace('{"before"', '\n{"before"').replace('{"counts"', '\n{"counts"'))


if __name__ == '__main__':
    main()
