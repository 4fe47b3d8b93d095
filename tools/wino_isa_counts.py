#!/usr/bin/env python3
"""Instruction counts of the Winograd layer kernels from the compiler's assembly listing.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC --cuda-device-only --no-gpu-bundle-output -S \
        augmentedautoencoder_amd/csrc/aae_wino.hip -o wino.s
    hipcc (the same flags) -c augmentedautoencoder_amd/csrc/aae_wino.hip -o wino.o
    python tools/wino_isa_counts.py wino.s [wino.o]

Per kernel: the instructions the K loop's price list cares about, registers and spills from the listing's metadata, and the
code size from the object file's symbol table when one is given."""
import collections
import re
import subprocess
import sys

WATCH = ['v_mfma_f32_32x32x2_f32', 'v_pk_add_f32', 'v_pk_fma_f32', 'v_add_f32', 'v_sub_f32', 'v_mov_b32', 'v_accvgpr', 's_barrier',
         's_and_saveexec_b64', 'v_cndmask_b32', 'v_cmp', 'ds_write_b128', 'ds_read_b128', 'buffer_load_dwordx4', 's_waitcnt', 's_cbranch', 's_nop']


def main():
    text = open(sys.argv[1]).read().splitlines()
    sizes = {}
    if len(sys.argv) > 2:
        for line in subprocess.check_output(['/opt/rocm/lib/llvm/bin/llvm-readelf', '-s', '--wide', sys.argv[2]]).decode().splitlines():
            f = line.split()
            if len(f) >= 8 and f[3] == 'FUNC':
                sizes[f[7]] = int(f[2])
    kernel, counts, meta = None, {}, {}
    for line in text:
        m = re.match(r'^(_ZN3aae\w+):', line)
        if m:
            kernel = m.group(1)
            counts[kernel] = collections.Counter()
            continue
        if line.startswith('.Lfunc_end'):
            kernel = None
        s = line.strip()
        if kernel and s and not s.startswith(('.', ';')) and not s.endswith(':'):
            op = s.split()[0]
            for w in WATCH:
                if op.startswith(w):
                    counts[kernel][w] += 1
        m = re.match(r'\s*\.name:\s+(\S+)', line)
        if m:
            meta_k = m.group(1)
        for key in ('.vgpr_count', '.vgpr_spill_count', '.sgpr_count', '.sgpr_spill_count', '.group_segment_fixed_size'):
            m = re.match(r'\s*%s:\s+(\d+)' % re.escape(key), line)
            if m:
                meta.setdefault(key, []).append(int(m.group(1)))
    names = [re.match(r'\s*\.name:\s+(\S+)', l).group(1) for l in text if re.match(r'\s*\.name:\s+_ZN3aae', l)]
    for n, k in enumerate(names):
        print(k)
        print('   ' + '  '.join('%s %d' % (w, counts[k][w]) for w in WATCH))
        print('   vgprs %d  vgpr spills %d  sgprs %d  sgpr spills %d  code bytes %s' % (
            meta['.vgpr_count'][n], meta['.vgpr_spill_count'][n], meta['.sgpr_count'][n], meta['.sgpr_spill_count'][n], sizes.get(k, 'n/a')))


if __name__ == '__main__':
    main()
