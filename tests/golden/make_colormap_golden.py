"""Writes tests/golden/colormap_luts.npz: the [256, 3] float32 colour tables of the listed matplotlib colormaps nerfstudio's
apply_float_colormap can index (`matplotlib.colormaps[name].colors`), so that the GPU tests of mtgs_amd.present do not need
matplotlib where they run.

    python tests/golden/make_colormap_golden.py
"""
from pathlib import Path

import numpy as np

NAMES = ("turbo", "viridis", "magma", "inferno", "cividis", "plasma")
OUT = Path(__file__).resolve().parent / "colormap_luts.npz"


def main():
    import matplotlib
    tables = {}
    for name in NAMES:
        table = np.asarray(matplotlib.colormaps[name].colors, dtype=np.float32)
        assert table.shape == (256, 3), (name, table.shape)
        tables[name] = table
    np.savez_compressed(OUT, **tables)
    print(f"{OUT}: {sorted(tables)} from matplotlib {matplotlib.__version__}, {OUT.stat().st_size} bytes")


if __name__ == "__main__":
    main()
