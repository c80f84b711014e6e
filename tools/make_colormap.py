#!/usr/bin/env python3
"""Regenerate ``biscuit_amd.render.PRGN_TRUNC``, the heatmap's default colour table, with matplotlib.

The reference draws its heatmaps with ``truncate_colormap(plt.get_cmap('PRGn'), 0.1, 0.9)`` (results.py:216).  The call is restated
here with matplotlib's public API: ``LinearSegmentedColormap.from_list(name, PRGn(np.linspace(0.1, 0.9, 100)))``, evaluated at the
integer indices 0..255 with ``bytes=True``.

    python tools/make_colormap.py            # print the literal
    python tools/make_colormap.py --check    # compare with the committed table (exit 1 when they differ)
    python tools/make_colormap.py --write    # rewrite the literal in biscuit_amd/render.py
"""
import argparse
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BEGIN, END = '# --- PRGN_TRUNC begin (tools/make_colormap.py) ---\n', '# --- PRGN_TRUNC end ---\n'


def prgn_trunc(minval=0.1, maxval=0.9, n=100):
    import matplotlib
    from matplotlib.colors import LinearSegmentedColormap
    base = matplotlib.colormaps['PRGn']
    cmap = LinearSegmentedColormap.from_list(f'trunc({base.name},{minval:.2f},{maxval:.2f})', base(np.linspace(minval, maxval, n)))
    return np.ascontiguousarray(cmap(np.arange(256), bytes=True)[:, :3], np.uint8)


def literal(lut):
    rows = ['    ' + ', '.join('(%3d, %3d, %3d)' % tuple(int(v) for v in rgb) for rgb in lut[i:i + 6]) + ',' for i in range(0, 256, 6)]
    return BEGIN + 'PRGN_TRUNC = np.array([\n' + '\n'.join(rows) + '\n], np.uint8)\n' + END


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--check', action='store_true')
    ap.add_argument('--write', action='store_true')
    args = ap.parse_args()
    lut = prgn_trunc()
    if args.check:
        sys.path.insert(0, ROOT)
        from biscuit_amd.render import PRGN_TRUNC
        same = np.array_equal(PRGN_TRUNC, lut)
        print('PRGN_TRUNC', 'matches' if same else 'DIFFERS from', 'matplotlib')
        return 0 if same else 1
    if args.write:
        path = os.path.join(ROOT, 'biscuit_amd', 'render.py')
        src = open(path).read()
        new, n = re.subn(re.escape(BEGIN) + '.*?' + re.escape(END), lambda m: literal(lut), src, flags=re.S)
        if n != 1:
            sys.exit(f'{path}: the PRGN_TRUNC markers were not found')
        open(path, 'w').write(new)
        return 0
    sys.stdout.write(literal(lut))
    return 0


if __name__ == '__main__':
    sys.exit(main())
