"""Pillow's 8-bit resampling tables on the host: the one ctypes caller of ldetr_resample_coeffs_filter (csrc/pil_resample.hpp holds the rule).
`render` pools the bilinear tables of a snapshot grid, `training.dataset_layoutganpp.resample_coeffs` uploads the Lanczos tables of the page resize."""
import ctypes

import numpy as np

from . import _lib

FILTER_BILINEAR, FILTER_LANCZOS = 0, 1   # include/ldetr_hip.h LDETR_FILTER_*

_cache = {}   # (in, out, filter) -> (bounds, weights, ksize)


def coeff_table(in_size, out_size, filter):
    """(bounds [out, 2], weights [ksize, out] tap-major, ksize) of the window `filter` for in_size -> out_size: host int32 arrays, computed once
    per key, shared between callers and therefore read-only."""
    key = (int(in_size), int(out_size), int(filter))
    hit = _cache.get(key)
    if hit is None:
        lib, ks = _lib.load(), ctypes.c_int(0)
        _lib.check(lib.ldetr_resample_coeffs_filter(key[2], key[0], key[1], None, None, 0, ctypes.byref(ks)), 'resample_coeffs_filter')
        bounds = np.zeros((key[1], 2), np.int32)
        weights = np.zeros((ks.value, key[1]), np.int32)
        _lib.check(lib.ldetr_resample_coeffs_filter(key[2], key[0], key[1], bounds.ctypes.data_as(ctypes.c_void_p), weights.ctypes.data_as(ctypes.c_void_p),
                                                    weights.size, ctypes.byref(ks)), 'resample_coeffs_filter')
        bounds.setflags(write=False)
        weights.setflags(write=False)
        hit = _cache[key] = (bounds, weights, ks.value)
    return hit
