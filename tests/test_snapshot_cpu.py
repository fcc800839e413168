"""Snapshot grids, the parts that need no GPU: the bilinear coefficient entry against the restated rule and Pillow, the restated rule
(tests/snapshot_common.py) against the fixture made by the reference's own convert_layout_to_image (tests/golden/snapshot.npz,
tools/gen_snapshot_golden.py), grid_indices, and the host-side validation of the raster entry."""
import ctypes
import os

import numpy as np
import pytest
import torch

import snapshot_common as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(50, 16), (30, 9), (30, 16), (24, 32), (37, 16), (23, 8), (800, 128), (560, 88), (1200, 128), (628, 66), (1, 5), (1000, 7), (48, 48), (80, 128), (56, 88)]


@pytest.fixture(scope='module')
def fx():
    d = np.load(os.path.join(ROOT, 'tests', 'golden', 'snapshot.npz'), allow_pickle=False)
    return {k: d[k] for k in d.files}


def _coeffs(lib, filt, i, o):
    ks = ctypes.c_int(0)
    assert lib.ldetr_resample_coeffs_filter(filt, i, o, None, None, 0, ctypes.byref(ks)) == 0
    b = np.zeros((o, 2), np.int32); k = np.zeros((ks.value, o), np.int32)
    assert lib.ldetr_resample_coeffs_filter(filt, i, o, b.ctypes.data_as(ctypes.c_void_p), k.ctypes.data_as(ctypes.c_void_p), k.size, ctypes.byref(ks)) == 0
    return b, k, ks.value


def test_bilinear_coefficients_match_the_restated_rule_and_the_lanczos_entry_is_unchanged():
    from layoutdetr_amd import _lib
    lib = _lib.load()
    for i, o in SIZES:
        b, k, ks = _coeffs(lib, 0, i, o)
        rb, rk, rks = SC.bilinear_coeffs(i, o)
        assert ks == rks and np.array_equal(b, rb) and np.array_equal(k.T, rk), (i, o)
        # the filter-selecting entry with LANCZOS is the existing entry
        lb, lk, lks = _coeffs(lib, 1, i, o)
        ks0 = ctypes.c_int(0)
        assert lib.ldetr_resample_coeffs(i, o, None, None, 0, ctypes.byref(ks0)) == 0 and ks0.value == lks
        b0 = np.zeros((o, 2), np.int32); k0 = np.zeros((lks, o), np.int32)
        assert lib.ldetr_resample_coeffs(i, o, b0.ctypes.data_as(ctypes.c_void_p), k0.ctypes.data_as(ctypes.c_void_p), k0.size, ctypes.byref(ks0)) == 0
        assert np.array_equal(lb, b0) and np.array_equal(lk, k0), (i, o)
    ks = ctypes.c_int(0)
    assert lib.ldetr_resample_coeffs_filter(2, 8, 4, None, None, 0, ctypes.byref(ks)) != 0 and b'unknown filter' in lib.ldetr_last_error()
    assert lib.ldetr_resample_coeffs_filter(0, 50, 16, b.ctypes.data_as(ctypes.c_void_p), k.ctypes.data_as(ctypes.c_void_p), 3, ctypes.byref(ks)) != 0
    assert b'too small' in lib.ldetr_last_error()


def test_pillow_bilinear_resize_equals_the_restated_rule():
    import PIL.Image
    rng = np.random.RandomState(1)
    for (W, H), (Wn, Hn) in [((50, 30), (16, 8)), ((30, 50), (8, 16)), ((24, 24), (32, 32)), ((16, 16), (16, 16)), ((37, 23), (16, 8)), ((800, 560), (128, 88)),
                             ((80, 56), (128, 88)), ((50, 30), (50, 8)), ((50, 30), (16, 30))]:
        img = rng.randint(0, 256, (H, W, 3)).astype(np.uint8)
        ref = np.array(PIL.Image.fromarray(img, 'RGB').resize((Wn, Hn), resample=PIL.Image.BILINEAR))
        assert np.array_equal(SC.resize_bilinear_u8(img, Hn, Wn), ref), ((W, H), (Wn, Hn))


def test_cell_size_entry_is_python_double_arithmetic():
    from layoutdetr_amd import _lib, render
    lib = _lib.load()
    rng = np.random.RandomState(2)
    cases = [(50, 30, 16), (30, 50, 16), (24, 24, 32), (37, 23, 16), (800, 560, 128), (1200, 628, 128), (1200, 628, 256), (1000, 1, 16), (3, 7, 2)]
    cases += [(int(w), int(h), int(s) * 2) for w, h, s in zip(rng.randint(1, 3000, 200), rng.randint(1, 3000, 200), rng.randint(1, 200, 200))]
    for W, H, S in cases:
        wn, hn = ctypes.c_int(0), ctypes.c_int(0)
        assert lib.ldetr_layout_raster_cell_size(W, H, S, ctypes.byref(wn), ctypes.byref(hn)) == 0
        assert (wn.value, hn.value) == SC.cell_size(W, H, S) == render.cell_size(W, H, S), (W, H, S)
    assert SC.cell_size(37, 23, 16) == (16, 8)


def test_restated_rule_reproduces_the_reference_fixture(fx):
    """Rules 1-6 against the reference's convert_layout_to_image (white pages and the same Pillow calls over random pages), rule 7's grids."""
    pal = [tuple(int(v) for v in c) for c in fx['palette']]
    n = 0
    for name, (W, H, S) in zip(fx['cases'], fx['case_whs']):
        W, H, S = int(W), int(H), int(S)
        for k in range(5):
            args = (fx[f'{name}_bbox'][k], fx[f'{name}_valid'][k], fx[f'{name}_labels'][k], pal, W, H, S)
            assert np.array_equal(SC.cell(*args), fx[f'{name}_white'][k]), (name, k)
            assert np.array_equal(SC.cell(*args, fx[f'{name}_pages'][k]), fx[f'{name}_over'][k]), (name, k, 'over')
            n += 2
        for j, k in enumerate((2, 3, 4)):
            assert np.array_equal(SC.cell(fx[f'{name}_bbox'][k], fx[f'{name}_valid'][k], fx[f'{name}_labels'][k], pal, W, H, S, fx[f'{name}_pages'][0]), fx[f'{name}_shared'][j])
    tp = [tuple(int(v) for v in c) for c in fx['tiny_palette']]
    for k in range(3):
        W, H = [int(v) for v in fx['tiny_wh'][k]]
        assert (W, H) == (800, 560)
        assert np.array_equal(SC.cell(fx['tiny_bbox'][k], fx['tiny_valid'][k], fx['tiny_labels'][k], tp, W, H, 128), fx['tiny_white'][k]), ('tiny', k)
        pg = fx['tiny_pages'][k]
        assert np.array_equal(SC.cell(fx['tiny_bbox'][k], fx['tiny_valid'][k], fx['tiny_labels'][k], tp, pg.shape[1], pg.shape[0], 128, pg), fx['tiny_over'][k]), ('tiny over', k)
        n += 2
    assert n == 56
    assert [int(v.sum()) for v in fx['land_valid']][:3] == [0, 1, 9]
    g = SC.grid(fx['land_bbox'], fx['land_valid'], fx['land_labels'], pal, (50, 30), 16, nrow=3)
    assert g.shape == (2 * 18 + 2, 3 * 18 + 2, 3) and np.array_equal(g, fx['grid_b5_nrow3'])
    assert np.array_equal(SC.grid(fx['land_bbox'], fx['land_valid'], fx['land_labels'], pal, (50, 30), 16), fx['grid_b5_default'])
    assert np.array_equal(SC.grid(fx['land_bbox'][2:3], fx['land_valid'][2:3], fx['land_labels'][2:3], pal, (50, 30), 16), fx['grid_b1']) and fx['grid_b1'].shape == (16, 16, 3)


def test_grid_indices_follow_the_random_state_rule():
    from layoutdetr_amd.training.snapshot_images import grid_indices
    for n, b, seed in [(3, 2, 0), (3, 8, 0), (100, 16, 0), (7, 7, 5), (1, 4, 0)]:
        rnd = np.random.RandomState(seed)
        idx = list(range(n))
        rnd.shuffle(idx)
        assert grid_indices(n, b, seed) == [idx[i % n] for i in range(b)]
    assert grid_indices(3, 2) == grid_indices(3, 2, 0)


def test_layout_grid_has_no_cpu_fallback():
    from layoutdetr_amd import render
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        render.layout_grid(torch.zeros(1, 9, 4), torch.ones(1, 9), torch.zeros(1, 9), [(1, 2, 3)], (50, 30))


def test_raster_entry_validates_before_any_launch():
    """null pointers, N <= 16, S even, resized sizes >= 1, the page table against the buffer, labels against the palette; B == 0 returns 0."""
    from layoutdetr_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(64)
    dp = (ctypes.addressof(buf) + 15) & ~15                      # stands for device memory: never dereferenced on the host
    B, N = 2, 9
    valid = np.ones((B, N), np.uint8); labels = np.zeros((B, N), np.int32); labels[1, 3] = 2
    pal = np.asarray([[1, 2, 3], [4, 5, 6], [7, 8, 9]], np.uint8)
    wh = np.asarray([[50, 30], [50, 30]], np.int32)
    cc = np.asarray([[0, 9, 100, 9]] * B, np.int64)
    table = np.asarray([[0, 50, 30], [4500, 50, 30]], np.int64)
    pidx = np.asarray([1, -1], np.int32)
    keep = [valid, labels, pal, wh, cc, table, pidx]

    def block(**ch):
        a = _lib.LayoutRasterArgs()
        a.struct_bytes = ctypes.sizeof(_lib.LayoutRasterArgs)
        a.B, a.N, a.S, a.nrow, a.n_colors, a.n_pages = B, N, 16, 0, 3, 2
        a.bbox = a.pages = a.coeffs = a.cells_dev = a.out = dp
        a.valid, a.labels, a.palette, a.page_wh, a.cell_coeffs = valid.ctypes.data, labels.ctypes.data, pal.ctypes.data, wh.ctypes.data, cc.ctypes.data
        a.page_table, a.page_index = table.ctypes.data, pidx.ctypes.data
        a.pages_bytes, a.coeffs_len = 9000, 4096
        for k, v in ch.items():
            setattr(a, k, v)
        return ctypes.byref(a)
    assert lib.ldetr_layout_raster_u8(block(B=0), None) == 0
    rc = lib.ldetr_layout_raster_u8(None, None)
    assert rc != 0 and b'null argument block' in lib.ldetr_last_error()
    wh_bad = np.asarray([[1000, 1], [50, 30]], np.int32)
    pidx_bad = np.asarray([2, -1], np.int32)
    for changes, message in [(dict(struct_bytes=8), b'argument block of 8 bytes'), (dict(N=17), b'1 <= N <= 16'), (dict(N=0), b'1 <= N <= 16'), (dict(S=15), b'must be even'),
                             (dict(bbox=None), b'null pointer'), (dict(out=None), b'null pointer'), (dict(valid=None), b'null pointer'), (dict(cells_dev=None), b'null pointer'),
                             (dict(pages=None), b'pages given without'), (dict(page_wh=wh_bad.ctypes.data), b'leaves no pixel'),
                             (dict(pages_bytes=8999), b'reaches past the page buffer'), (dict(page_index=pidx_bad.ctypes.data), b'outside the page table'),
                             (dict(n_colors=2), b'outside the palette'), (dict(coeffs_len=100), b'coefficient table'), (dict(B=-1), b'negative B')]:
        rc = lib.ldetr_layout_raster_u8(block(**changes), None)
        assert rc != 0 and message in lib.ldetr_last_error(), (changes, lib.ldetr_last_error())
    # the page a cell names must have the cell's size
    table[1] = [4500, 30, 50]
    rc = lib.ldetr_layout_raster_u8(block(), None)
    assert rc != 0 and b'the cell says 50 x 30' in lib.ldetr_last_error()
    del keep
