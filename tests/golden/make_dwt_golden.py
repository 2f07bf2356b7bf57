"""Writes dwt_db4_periodization.npz: PyWavelets' multilevel db4 transform in mode "periodization", in the in-place Mallat
layout of pywt.coeffs_to_array, for the shapes the wavelet tests pin (tests/test_wavelet_cpu.py).  Needs PyWavelets (1.1.1
made the committed file); the tests read only the .npz.

    python tests/golden/make_dwt_golden.py
"""
import os

import numpy as np
import pywt

SHAPES = [(16, 8), (32, 24), (128, 128), (8, 8, 4), (16, 16, 8), (9, 7)]


def levels(n):
    m, L = int(min(n)), 0
    while m > 0 and m % 2 == 0:
        m //= 2
        L += 1
    return L


def main():
    rng = np.random.default_rng(20261015)
    out = {"pywt_version": np.array(pywt.__version__)}
    for n in SHAPES:
        x = rng.standard_normal(n)
        L = levels(n)
        if L == 0:
            c = x.copy()
        else:
            c, _ = pywt.coeffs_to_array(pywt.wavedecn(x, "db4", mode="periodization", level=L))
        key = "x".join(str(v) for v in n)
        out["x_" + key] = x
        out["c_" + key] = c
    np.savez(os.path.join(os.path.dirname(os.path.abspath(__file__)), "dwt_db4_periodization.npz"), **out)


if __name__ == "__main__":
    main()
