#!/usr/bin/env python3
"""Pins the mean pyramid (--pyramid-method mean) against the library call the reference makes.

The reference's zarr_stitcher.py:614-719 (generate_pyramid_levels -> downsample_block) stores, level after level,
``da.coarsen(np.mean, previous, {y: 2, x: 2}, trim_excess=True)`` of the STORED level before, assigned into a dataset of the
input's integer dtype (the float64 mean of four integers is exact; the assignment truncates).  This script makes exactly that
call with the reference's own library (dask 2021.10 in the authoring container, under /opt/conda/bin/python3.9) on a handful
of small planes and writes inputs and every level to tests/golden/pyramid_mean_vectors.npz:

    /opt/conda/bin/python3.9 tests/golden/make_golden_pyramid_mean.py

Keys: ``in_<case>`` and ``l<k>_<case>`` for k = 1 ... while the level before has at least 2 rows and 2 columns.  The dask chunks
are even (with odd chunks coarsen trims per chunk, which is dask's business, not the definition).
tests/test_pyramid_mean_cpu.py restates the formula in numpy against these vectors; tests/test_pyramid_mean_gpu.py runs the
device kernel on them.
"""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def cases():
    rng = np.random.default_rng(20240611)

    def rand(shape, dtype):
        return rng.integers(0, np.iinfo(dtype).max + 1, shape).astype(dtype)

    return {
        'odd_odd_u16': rand((37, 53), 'uint16'),
        'even_odd_u16': rand((32, 49), 'uint16'),
        'odd_even_u8': rand((45, 96), 'uint8'),
        'side2_u16': rand((2, 21), 'uint16'),
        'side3_u8': rand((19, 3), 'uint8'),
        'narrow_u16': rand((5, 2), 'uint16'),          # sides below one 16-byte vector
        'narrow_u8': rand((7, 6), 'uint8'),
        'all_65535': np.full((34, 41), 65535, 'uint16'),   # the 18-bit sum
        'all_255': np.full((33, 70), 255, 'uint8'),
        'random_u16': rand((32, 48), 'uint16'),
        'random_u8': rand((45, 70), 'uint8'),
        'five_levels_u16': rand((67, 40), 'uint16'),
        'five_levels_u8': rand((99, 163), 'uint8'),
    }


def main():
    import dask.array as da
    out = {}
    for name, img in cases().items():
        out['in_' + name] = img
        level, k = img, 0
        while level.shape[0] >= 2 and level.shape[1] >= 2:
            k += 1
            d = da.from_array(level, chunks=(16, 32))
            mean = da.coarsen(np.mean, d, {0: 2, 1: 2}, trim_excess=True).compute()
            stored = np.zeros(mean.shape, dtype=img.dtype)
            stored[...] = mean                                  # what ``ds[0, c, z0:z1] = downsampled`` does
            out[f'l{k}_{name}'] = stored
            level = stored
    path = os.path.join(HERE, 'pyramid_mean_vectors.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes,', len(out), 'arrays')


if __name__ == '__main__':
    main()
