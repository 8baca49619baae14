#!/usr/bin/env python3
"""Did a change move any existing kernel?  Compares the code-object metadata (VGPRs, AGPRs, SGPRs, LDS, scratch, spills, workgroup size) of
every kernel symbol of a BASE libsca_hip.so with the same symbol in a NEW one; symbols only the new library has are listed apart.
Needs no GPU.  Usage: python tools/kernel_resources_diff.py base/libsca_hip.so [new/libsca_hip.so]   (exit status 1: something moved)"""
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_regs  # noqa: E402

FIELDS = ('vgpr', 'agpr', 'sgpr', 'lds', 'scratch', 'spill', 'wg')


def demangle(names):
    out = subprocess.check_output(['c++filt'], input='\n'.join(names), text=True).splitlines()
    return dict(zip(names, (o.split('(')[0] for o in out)))


def main():
    base = sys.argv[1]
    new = sys.argv[2] if len(sys.argv) > 2 else os.path.join(kernel_regs.ROOT, 'sca_amd', 'lib', 'libsca_hip.so')
    kb = {k['name']: k for k in kernel_regs.kernels(base)}
    kn = {k['name']: k for k in kernel_regs.kernels(new)}
    nice = demangle(sorted(set(kb) | set(kn)))
    moved = gone = 0
    print(f'{"kernel":64s} ' + ' '.join(f'{f:>7s}' for f in FIELDS) + '  verdict')
    for name in sorted(kb, key=lambda s: nice[s]):
        b = kb[name]
        if name not in kn:
            gone += 1
            print(f'{nice[name][:64]:64s} ' + ' '.join(f'{b[f]:>7s}' for f in FIELDS) + '  MISSING in the new library')
            continue
        n = kn[name]
        same = all(b[f] == n[f] for f in FIELDS)
        moved += not same
        print(f'{nice[name][:64]:64s} ' + ' '.join(f'{b[f]:>7s}' if b[f] == n[f] else f'{b[f]}>{n[f]}'.rjust(7) for f in FIELDS) + ('  same' if same else '  MOVED'))
    added = sorted((s for s in kn if s not in kb), key=lambda s: nice[s])
    print(f'\nnew kernels ({len(added)}):')
    for name in added:
        n = kn[name]
        print(f'{nice[name][:64]:64s} ' + ' '.join(f'{n[f]:>7s}' for f in FIELDS))
    print(f'\n{len(kb)} kernels in the base library: {len(kb) - moved - gone} same, {moved} moved, {gone} missing; {len(added)} new')
    return 1 if moved or gone else 0


if __name__ == '__main__':
    sys.exit(main())
